"""The plain torch restatement of DynamicRoutingLayer (MIND behaviour-to-interest capsule routing,
layers/ctr/dynamic_routing.py) that the routing tests compare against (CPU, any floating dtype, explicit noise):
    pri[b,n,:] = x[b,n,:] @ S                                   the same for every capsule k
    c[b,k,n] = 0
    num_iter - 1 times:  w = softmax_k(noise[b,k,n,r] + c[b,k,n]);  z[b,k,r] = sum_n w pri;  v = squash(z)
                         c[b,k,n] += sum_r pri[b,n,r] v[b,k,r]
    w = softmax_k(noise + c);  z = sum_n w pri;  out = squash(z)                    (B, K', R)
    squash(z) = n2 / (1 + n2) * z / (sqrt(n2) + 1e-8),  n2 = sum_r z^2
The loop runs on detached priors: gradient flows through the last ``w * pri`` only, with w a constant.
tests/test_dynamic_routing_host.py pins it to the reference's own outputs and gradients
(tests/golden/dynamic_routing.npz); the GPU tests run it in fp64 at sizes the fixture does not hold.  Also the case lists
shared by the generator (tests/golden/make_golden_dynamic_routing.py) and the tests."""
import math

import torch

# (B, N, E, R, max_num_caps, num_iter): cases of dynamic_routing.npz
ROUTING_SHAPES = [(3, 1, 8, 8, 4, 2), (4, 2, 8, 8, 4, 3), (8, 4, 16, 16, 4, 3), (5, 7, 8, 5, 3, 1), (6, 12, 16, 16, 3, 2),
                  (4, 50, 16, 32, 8, 3)]
# GPU cases beyond the fixture: cap binds + vector path, K' = 6 (the largest state), odd sizes, element path without a loop,
# more samples than one grid pass
EXTRA_SHAPES = [(16, 50, 64, 64, 4, 3), (3, 64, 16, 128, 8, 3), (7, 33, 24, 40, 8, 2), (5, 7, 8, 5, 3, 1),
                (4099, 12, 16, 16, 3, 2)]
FIVE_ITER_SHAPE = (8, 50, 64, 64, 8, 5)
X_SCALE = 0.3          # inputs are X_SCALE * randn


def shape_tag(s):
    return "%d_%d_%d_%d_c%d_i%d" % tuple(s)


def num_caps(N, max_num_caps):
    """K' = max(1, min(K, log2 N)), truncated (dynamic_routing.py:79-89)"""
    return int(max(1, min(max_num_caps, math.log2(N))))


def squash(z):
    n2 = (z * z).sum(dim=-1, keepdim=True)
    return (n2 / (1 + n2)) * (z / (torch.sqrt(n2) + 1e-8))


def routing_state(pri, noise, num_iter):
    """the routing sum c (B, K', N) after num_iter - 1 iterations over priors (B, N, R) and noise (B, K', N, R)"""
    pri = pri.detach()
    c = pri.new_zeros(noise.shape[:3])
    for _ in range(num_iter - 1):
        w = torch.softmax(noise + c.unsqueeze(-1), dim=1)
        v = squash((w * pri.unsqueeze(1)).sum(dim=2))
        c = c + torch.einsum("bnr,bkr->bkn", pri, v)
    return c


def dynamic_routing(x, S, noise, num_iter):
    """(B, N, E), (E, R), (B, K', N, R) -> (B, K', R); differentiable in x and S"""
    pri = x @ S
    c = routing_state(pri, noise, num_iter)
    w = torch.softmax(noise.detach() + c.unsqueeze(-1), dim=1)
    return squash((w * pri.unsqueeze(1)).sum(dim=2))


def dynamic_routing_grads(x, S, noise, num_iter, gout):
    """out, gx, gS of the restatement in the operands' dtype"""
    x = x.detach().clone().requires_grad_()
    S = S.detach().clone().requires_grad_()
    out = dynamic_routing(x, S, noise, num_iter)
    gx, gS = torch.autograd.grad(out, (x, S), gout)
    return out.detach(), gx, gS


def make_inputs(shape, dtype=torch.float32, seed=None):
    """x, S, noise, gout for a case, drawn in fp32 from a generator of their own and rounded to ``dtype`` (returned in
    fp32: values representable in ``dtype``)"""
    B, N, E, R, caps, _ = shape
    K = num_caps(N, caps)
    g = torch.Generator().manual_seed(7700 + B + 3 * N + 5 * E + 7 * R + caps if seed is None else seed)
    ts = (X_SCALE * torch.randn(B, N, E, generator=g), torch.randn(E, R, generator=g),
          torch.randn(B, K, N, R, generator=g), torch.randn(B, K, R, generator=g))
    return tuple(t.to(dtype).float() for t in ts)

"""The plain torch restatement of ComposeExcitationNetworkLayer (SENET / CEN) and of the two models built on it that the
SENET tests compare against (CPU):  z = mean_E x;  h = act(W1 z + b1);  a = act(W2 h + b2);  out = x * a[..., None].
tests/test_senet_host.py pins it to the reference's own outputs and gradients (tests/golden/senet.npz); the GPU tests use
it at sizes the fixture does not hold."""
import torch
import torch.nn.functional as F

SENET_SHAPES = [(8, 4, 128, 2, False), (16, 6, 64, 3, False), (32, 12, 8, 4, False), (32, 10, 16, 2, False),
                (8, 39, 64, 3, False), (6, 4, 16, 2, True), (8, 6, 8, 3, True), (6, 5, 10, 2, False)]  # (B, N, E, reduction, squared)
PARAM_KEYS = ["fc.ReductionLinear.weight", "fc.ReductionLinear.bias", "fc.AdditionLinear.weight", "fc.AdditionLinear.bias"]
# model cases of senet.npz: name -> constructor arguments of the reference model (batch 16)
FIBINET_ARGS = dict(embed_size=16, num_fields=6, senet_reduction=3, deep_output_size=1, deep_layer_sizes=[32, 16])
FIBINET_TYPES = ["all", "each"]
FAT_ARGS = dict(embed_size=8, num_fields=4, deep_output_size=1, deep_layer_sizes=[16], reduction=2)
MODEL_BATCH = 16
NEAR_MARGIN = 1e-5          # |pre-activation| below this: the ReLU derivative is decided by fp32 summation noise
NEAR_CAP = 0.01             # share of samples that may be left out of a gradient comparison for that reason


def shape_tag(s):
    return "%d_%d_%d_%d_%s" % (s[0], s[1], s[2], s[3], "sq" if s[4] else "pl")


def fields(N, squared):
    return N * N if squared else N


def make_x(g, B, M, E):
    """The per-field offset makes the means differ between samples (with plain randn every gate is decided by the bias)."""
    return 0.5 * torch.randn(B, M, E, generator=g) + torch.randn(B, M, 1, generator=g)


def pre_activations(x, W1, b1, W2, b2, act=torch.relu):
    z = x.mean(dim=2)
    u = F.linear(z, W1, b1)
    v = F.linear(act(u), W2, b2)
    return z, u, v


def compose(x, W1, b1, W2, b2, act=torch.relu):
    """(B, M, E) -> (B, M, E); compose_excitation_network.py:85-107 written out"""
    _, _, v = pre_activations(x, W1, b1, W2, b2, act)
    return x * act(v).unsqueeze(-1)


def near_boundary(x, W1, b1, W2, b2, margin=NEAR_MARGIN):
    """(B,) bool: samples with a pre-activation of either layer within ``margin`` of the ReLU's kink"""
    _, u, v = pre_activations(x.double(), W1.double(), b1.double(), W2.double(), b2.double())
    near = v.abs().amin(dim=1) < margin
    if u.shape[1]:
        near = near | (u.abs().amin(dim=1) < margin)
    return near


def compose_chunked(x, W1, b1, W2, b2, gout, chunk=4096, dtype=torch.float64, margin=NEAR_MARGIN):
    """ReLU layer, forward and backward written out, a chunk of samples at a time in ``dtype`` with no autograd graph.
    Returns out, gx, the four parameter gradients (W1, b1, W2, b2), for each of them T = sum_b |term_b| (the magnitude of
    what was summed), and the (B,) mask of samples left out (``near_boundary``): their rows of gx are not comparable and
    they contribute to NO parameter gradient here (the caller zeroes their upstream gradient on the device side)."""
    W1d, b1d, W2d, b2d = (t.detach().to(dtype) for t in (W1, b1, W2, b2))
    E = x.shape[2]
    outs, gxs, nears = [], [], []
    grads = [torch.zeros_like(t) for t in (W1d, b1d, W2d, b2d)]
    terms = [torch.zeros_like(t) for t in (W1d, b1d, W2d, b2d)]
    for b0 in range(0, x.shape[0], chunk):
        xc, gc = x[b0:b0 + chunk].to(dtype), gout[b0:b0 + chunk].to(dtype)
        z = xc.mean(dim=2)
        u = F.linear(z, W1d, b1d)
        h = torch.relu(u)
        v = F.linear(h, W2d, b2d)
        a = torch.relu(v)
        near = v.abs().amin(dim=1) < margin
        if u.shape[1]:
            near = near | (u.abs().amin(dim=1) < margin)
        outs.append(xc * a.unsqueeze(-1))
        gc = gc * (~near).to(dtype)[:, None, None]
        ga = (gc * xc).sum(dim=2)
        gv = ga * (v > 0)
        gu = (gv @ W2d) * (u > 0)
        gz = gu @ W1d
        gxs.append(gc * a.unsqueeze(-1) + gz.unsqueeze(-1) / E)
        for k, (l, r) in enumerate(((gu, z), (gu, None), (gv, h), (gv, None))):
            if r is None:
                grads[k] += l.sum(0)
                terms[k] += l.abs().sum(0)
            else:
                grads[k] += l.t() @ r
                terms[k] += l.abs().t() @ r.abs()
        nears.append(near)
    return torch.cat(outs), torch.cat(gxs), grads, terms, torch.cat(nears)


def pair_indices(N):
    r = [i for i in range(N - 1) for _ in range(i + 1, N)]
    c = [j for i in range(N - 1) for j in range(i + 1, N)]
    return torch.tensor(r), torch.tensor(c)


def bilinear(x, W, b, kind):
    r, c = pair_indices(x.shape[1])
    p, q = x[:, r], x[:, c]
    if kind == "all":
        return torch.matmul(p, W) * q + b
    return torch.einsum("bpe,peh->bph", p, W) * q + b


def mlp(x, P, prefix):
    """Linear_i + ReLU ... LinearOutput (multilayer_perceptron.py:53-61), parameters by state_dict key"""
    i = 0
    while f"{prefix}.model.Linear_{i}.weight" in P:
        x = torch.relu(F.linear(x, P[f"{prefix}.model.Linear_{i}.weight"], P[f"{prefix}.model.Linear_{i}.bias"]))
        i += 1
    return F.linear(x, P[f"{prefix}.model.LinearOutput.weight"], P[f"{prefix}.model.LinearOutput.bias"])


def senet_of(x, P, prefix):
    return compose(x, *(P[f"{prefix}.{k}"] for k in PARAM_KEYS))


def fibinet(x, P, kind):
    """feature_importance_and_bilinear_feature_interaction_network.py:83-111: (B, N, E) -> (B, 1)"""
    emb = bilinear(x, P["emb_bilinear.bilinear.weight"], P["emb_bilinear.bilinear.bias"], kind)
    sen = bilinear(senet_of(x, P, "senet"), P["senet_bilinear.bilinear.weight"], P["senet_bilinear.bilinear.bias"], kind)
    return mlp(torch.cat([emb, sen], dim=1).flatten(1), P, "deep")


def fat_deep_ffm(x, P, N):
    """fat_deep_ffm.py:82-109: (B, N*N, E) -> (B, 1)"""
    aem = senet_of(x, P, "cen")
    first = aem.sum(dim=(1, 2)).unsqueeze(1)
    x4 = aem.reshape(aem.shape[0], N, N, aem.shape[2])
    r, c = pair_indices(N)
    second = (x4[:, r, c] * x4[:, c, r]).flatten(1)
    return first + mlp(second, P, "deep")

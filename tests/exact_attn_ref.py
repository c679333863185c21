"""Operands and float64 references that make the MFMA path of csrc/self_attn.hip comparable BIT FOR BIT.

With Wq = 0 and bq = 0 every score is 0 and P = 1 / L exactly for L in {16, 32, 64}.  The rest is chosen so that every
value the kernel rounds to bf16 on its way into a matrix-core product survives the rounding, and every fp32 sum is exact in
any order (all terms are multiples of one power of two, and the sums of their magnitudes stay far below 2**24 of it):

  X      two list positions per sample carry one entry of +-1, every other row is zero;
  Wk, Wv, Wout   signed permutations;   bk, bv, bout in {-1, 0, 1};   G in {-1, 0, 1}, dense.

Then K and V are small integers, O = mean_l V and dV = mean_l dO are integers / L, dP = u_r + delta with delta in
{-1, 0, 1} at the two live columns, dS = (L delta - sum delta) / L**2 has a numerator below 2**8, and dQ = dS K / 4
(d = 16 in every case) a numerator of at most 132.  dK = dS^T Q = 0.  The query rows of dWin = dQ^T X are NOT zero although
Wq is.  tests/test_exact_attn_host.py asserts all of this in float64; tests/test_gpu_exact_self_attn.py then demands the
float64 result, rounded once to bf16, from the kernel.  Nothing here imports torecsys_amd."""
import math
from types import SimpleNamespace as NS

import torch

from exact_ref import F64, gen, ints, signed_rows

# (E, H, L), B = 33: d = 16 everywhere, so 1 / sqrt(d) = 1 / 4 is exact
EXACT_ATTN_CASES = [(E, H, L) for (E, H) in [(64, 4), (32, 2), (16, 1)] for L in (16, 32, 64)]
EXACT_ATTN_B = 33


def attn_tag(c):
    return "E%d_H%d_L%d" % tuple(c)


def make_case(E, H, L, B=EXACT_ATTN_B):
    g = gen(E, H, L, B)
    x = torch.zeros(B, L, E, dtype=F64)
    for b in range(B):
        rows = torch.randperm(L, generator=g)[:2]
        cols = torch.randint(0, E, (2,), generator=g)
        x[b, rows, cols] = (torch.randint(0, 2, (2,), generator=g) * 2 - 1).to(F64)
    w_in = torch.cat([torch.zeros(E, E, dtype=F64), signed_rows(E, E, 1, g), signed_rows(E, E, 1, g)])
    b_in = torch.cat([torch.zeros(E, dtype=F64), ints(E, g), ints(E, g)])
    return NS(E=E, H=H, L=L, B=B, x=x, w_in=w_in, b_in=b_in, w_out=signed_rows(E, E, 1, g), b_out=ints(E, g),
              gout=ints((B, L, E), g))


def reference(c):
    """float64: the outputs {y, dx, dw_in, db_in, dw_out, db_out} by autograd on the formula, and every tensor the kernel
    rounds to bf16 between its products, by the backward formulas of csrc/self_attn.hip"""
    B, L, E, H = c.B, c.L, c.E, c.H
    d = E // H
    leaves = [t.clone().requires_grad_() for t in (c.x, c.w_in, c.b_in, c.w_out, c.b_out)]
    x, w_in, b_in, w_out, b_out = leaves
    qkv = x @ w_in.t() + b_in
    q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(B, L, H, d).transpose(1, 2) for i in range(3))
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), dim=-1)
    o = (P @ v).transpose(1, 2).reshape(B, L, E)
    y = x + o @ w_out.t() + b_out
    (y * c.gout).sum().backward()
    out = dict(y=y.detach(), dx=x.grad, dw_in=w_in.grad, db_in=b_in.grad, dw_out=w_out.grad, db_out=b_out.grad)
    with torch.no_grad():
        dO = c.gout @ c.w_out
        dOh = dO.reshape(B, L, H, d).transpose(1, 2)
        dV = P.transpose(-1, -2) @ dOh
        dP = dOh @ v.transpose(-1, -2)
        dS = P * (dP - (dP * P).sum(-1, keepdim=True))
        dQ = dS @ k / math.sqrt(d)
        dK = dS.transpose(-1, -2) @ q / math.sqrt(d)
    mid = dict(x=c.x, w_in=c.w_in, w_out=c.w_out, gout=c.gout, qkv=qkv.detach(), P=P.detach(), O=o.detach(), dO=dO, dS=dS,
               dQ=dQ, dK=dK, dV=dV)
    return out, mid

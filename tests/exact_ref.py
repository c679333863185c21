"""Integer operands and float64 references that make the bf16 matrix-core kernels comparable BIT FOR BIT.

Every kernel in csrc/cross_mfma.hip, pairx_mfma.hip, cin_mfma.hip, mlp_fused.hip / mlp_ro.hpp, wgrad_rows.hip and the
rows-gemm kernel multiplies bf16 operands, accumulates in fp32 and rounds once on store.  With inputs and output gradients
in {-1,0,1} and weight matrices that hold ``k`` entries of +-1 per row, every product is a small integer, every fp32 sum
of them is exact (an integer below 2**24, in any order of summation), and every tensor the kernels keep in bf16 between
their stages is an integer of at most 256 in magnitude, i.e. unchanged by the rounding.  The result of a correct kernel
is then ``expect(ref, dtype)`` -- the float64 value rounded once -- and a missing, doubled or misplaced term changes it.

``assert_exact_domain`` is the guard that makes that a fair demand; tests/test_exact_ref_host.py runs it over every case
list below, and tests/test_gpu_exact_mfma.py takes its cases from the same lists.  Nothing here imports torecsys_amd.

tests/exact_ipn_ref.py builds on ``gen``, ``ints``, ``expect``, ``assert_exact_domain``, ``mismatch`` and ``pair_index``
from here for the inner-product network kernels of csrc/pair.hip (tests/test_exact_ipn_host.py, tests/test_gpu_exact_ipn.py).
"""
import functools
import os
import re
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torecsys_amd", "csrc")
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# generators (all seeded)
# ---------------------------------------------------------------------------------------------------------------------
def gen(*key):
    s = 12345
    for v in key:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def ints(shape, g):
    """values in {-1, 0, 1}, float64"""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.randint(-1, 2, shape, generator=g).to(F64)


def signed_rows(out_f, in_f, k, g):
    """(out_f, in_f) float64 with ``k`` entries of +-1 per row at distinct random columns, zeros elsewhere.  Square with
    k = 1: a signed permutation, so every input column is used exactly once."""
    if k == 1 and out_f == in_f:
        cols = torch.randperm(in_f, generator=g).view(out_f, 1)
    else:
        cols = torch.rand(out_f, in_f, generator=g).topk(k, dim=1).indices
    sgn = (torch.randint(0, 2, (out_f, k), generator=g) * 2 - 1).to(F64)
    return torch.zeros(out_f, in_f, dtype=F64).scatter_(1, cols, sgn)


def pair_stack(P, E, g):
    """(P, E, E): one signed permutation per pair (the per-pair weights of the bilinear kernels, [e][h])"""
    return torch.stack([signed_rows(E, E, 1, g) for _ in range(P)])


def row_structure(W):
    """(cols (out,k) int64, signs (out,k)) of a matrix with the same number of nonzeros in every row"""
    out_f = W.shape[0]
    nz = W.nonzero()
    k = nz.shape[0] // out_f
    assert nz.shape[0] == k * out_f and torch.equal(nz[:, 0], torch.arange(out_f).repeat_interleave(k))
    cols = nz[:, 1].view(out_f, k)
    return cols, W.gather(1, cols)


# ---------------------------------------------------------------------------------------------------------------------
# the guard, and what a kernel that is exact must return
# ---------------------------------------------------------------------------------------------------------------------
def expect(ref, dtype):
    """an exact fp32 result rounded once (to nearest even) into ``dtype``"""
    return ref.detach().to(torch.float32).to(dtype)


def assert_exact_domain(intermediates, outputs, term_sums=None):
    """``intermediates``: name -> tensor the kernels keep in bf16 between stages (inputs, per-layer activations and their
    gradients, CIN / pair outputs): must survive a round trip through bf16.  ``outputs``: name -> fp32 accumulation:
    integers below 2**24 in magnitude.  ``term_sums``: name -> sum of |terms| of a sum the kernels build from bf16 PARTIAL
    sums (the pair kernels' contribution rows): at most 256, so every partial sum of those integer terms is bf16-exact
    whatever its grouping.  No exceptions: a case that fails here is changed, not excused."""
    for name, t in intermediates.items():
        t = t.detach().to(F64)
        back = t.to(torch.bfloat16).to(F64)
        assert torch.equal(back, t), f"{name}: {int((back != t).sum())} values change in a bf16 round trip (max |v| {float(t.abs().max())})"
    for name, t in outputs.items():
        t = t.detach().to(F64)
        assert torch.equal(t, t.round()), f"{name}: not integer"
        assert float(t.abs().max()) < 2 ** 24 if t.numel() else True, f"{name}: |v| reaches 2**24"
    for name, t in (term_sums or {}).items():
        t = t.detach().to(F64)
        assert torch.equal(t, t.round()) and float(t.max()) <= 256, f"{name}: sum of |terms| {float(t.max())} > 256"


def mismatch(name, got, want):
    """None when equal, else a message that locates the first differing element"""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{name}: got {tuple(got.shape)} {got.dtype}, want {tuple(want.shape)} {want.dtype}"
    if torch.equal(got, want):
        return None
    bad = (got != want) | (got.isnan() != want.isnan())
    first = tuple(int(v) for v in bad.nonzero()[0])
    return (f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, first at {first}: got {float(got[first])}, "
            f"want {float(want[first])}")


# ---------------------------------------------------------------------------------------------------------------------
# thresholds of the kernel sources the case lists sit on
# ---------------------------------------------------------------------------------------------------------------------
_CONST_SITES = {
    "B3_CHAIN": ("cross_mfma.hip", r"static constexpr int CHAIN = (\d+);"),
    "B3_ROWS_IS_CHAIN_TILES": ("cross_mfma.hip", r"static constexpr int ROWS = CHAIN \* (16);"),
    "BW_MAX_BLOCKS": ("cross_mfma.hip", r"constexpr int BW_MAX_BLOCKS = (\d+);"),
    "MF_ROWS": ("mlp_fused.hip", r"constexpr int MF_ROWS = (\d+);"),
    "MF_GRID": ("mlp_fused.hip", r"constexpr int MF_GRID = (\d+);"),
    "RO_ROWS": ("mlp_ro.hpp", r"constexpr int RO_ROWS = (\d+);"),
    "WG_KS": ("wgrad_rows.hip", r"constexpr int WG_KS = (\d+);"),
    "WG_KR": ("wgrad_rows.hip", r"constexpr int WG_KR = (\d+);"),
    "WG_TC": ("wgrad_rows.hip", r"constexpr int WG_TC = (\d+);"),
    "PB_PPT": ("pairx_mfma.hip", r"constexpr int PB_PPT = (\d+);"),
    "DW_NG": ("cin_mfma.hip", r"constexpr int DW_NG = (\d+);"),
}


def source_constants():
    out = {}
    for name, (fname, pat) in _CONST_SITES.items():
        with open(os.path.join(CSRC, fname)) as f:
            m = re.findall(pat, f.read())
        assert len(m) == 1, (name, fname, m)
        out[name] = int(m[0])
    out["B3_ROWS"] = out["B3_CHAIN"] * out.pop("B3_ROWS_IS_CHAIN_TILES")
    return out


TILE, B3_ROWS, BW_MAX_BLOCKS = 16, 96, 256
MF_ROWS, MF_GRID, RO_ROWS = 128, 256, 256
WG_KS, WG_KR, WG_TC, PB_PPT = 32, 64, 7, 3
CROSS_FWD_UNIT, CROSS_FWD_GRID_RESIDENT = 8 * TILE, 3 * 256      # csrc/cross_mfma.hip, cross_mfma_fwd: grid


def cross_nparts(rows):
    """partials the backward hands to cross_reduce_partials_kernel (cross_bwd_launch: its grid)"""
    return min((rows + B3_ROWS - 1) // B3_ROWS, BW_MAX_BLOCKS)


def cross_fwd_resident(E, L):
    """cross_mfma_fwd: the packed weights and fp32 biases of all layers fit in 64 KiB of LDS"""
    return L * E * E * 2 + L * E * 4 <= 64 * 1024


def wgrad_splits(M, N, rows):
    """csrc/wgrad_rows.hip, wgrad_plan restated for what trs_wgrad_rows_splits returns (0: not taken).  Below 2**20 rows
    the two-block DMA form is never chosen, so the slots are 32 / (MB * NB)."""
    if M < 8 or N < 8 or M % 8 or N % 8 or rows < 4 * WG_KR:
        return 0
    assert rows < 1 << 20
    Mt, Nt = (M + 15) // 16, (N + 15) // 16
    if (Mt <= 4 * WG_TC and Nt <= WG_TC and Mt + Nt <= 32 and Mt >= Nt) or (Mt <= WG_TC and Nt <= 4 * WG_TC and Mt + Nt <= 32):
        MB = NB = 1
    else:
        MB, NB = -(-Mt // (2 * WG_TC)), -(-Nt // (2 * WG_TC))
        while MB & (MB - 1):
            MB += 1
        while NB & (NB - 1):
            NB += 1
        if MB * NB > 32:
            return 0
    slots = 32 // (MB * NB)
    stages = (rows + WG_KR - 1) // WG_KR
    while slots > 1 and stages // (8 * slots) < 4:
        slots >>= 1
    return 8 * slots


def pair_tasks(N):
    """the (i, j0, count <= PB_PPT) and (j, i0, count) task lists of the per-pair kernels (functional._pair_tasks)"""
    ti = [(i, j0, min(PB_PPT, N - j0)) for i in range(N) for j0 in range(i + 1, N, PB_PPT)]
    tj = [(j, i0, min(PB_PPT, j - i0)) for j in range(N) for i0 in range(0, j, PB_PPT)]
    return ti, tj


def pair_index(N):
    I = [i for i in range(N - 1) for _ in range(i + 1, N)]
    J = [j for i in range(N - 1) for j in range(i + 1, N)]
    return torch.tensor(I), torch.tensor(J)


# ---------------------------------------------------------------------------------------------------------------------
# float64 references, layer by layer
# ---------------------------------------------------------------------------------------------------------------------
def cross_ref(x, W, b, gout, detach_first):
    """x (rows,E), W (L,E,E), b (L,E): x_{l+1} = x0 * (x_l W_l^T + b_l) + x0 (oracle.cpu_ref.cross_network); the running
    value starts from x0.detach() with ``detach_first``.  Intermediates: every x_l, u_l, u_l + 1 and their gradients."""
    L = W.shape[0]
    x0 = x.clone().requires_grad_()
    Wl = [W[l].clone().requires_grad_() for l in range(L)]
    bl = [b[l].clone().requires_grad_() for l in range(L)]
    cur = x0.detach() if detach_first else x0
    xs, us = [cur], []
    for l in range(L):
        u = F.linear(cur, Wl[l], bl[l])
        u.retain_grad()
        cur = x0 * u + x0
        cur.retain_grad()
        us.append(u)
        xs.append(cur)
    cur.backward(gout)
    inter = {"x": x, "gout": gout, "W": W, "b": b}
    for l in range(L):
        inter[f"x{l + 1}"], inter[f"u{l}"], inter[f"u{l}+1"] = xs[l + 1], us[l], us[l] + 1
        inter[f"g{l + 1}"], inter[f"du{l}"] = xs[l + 1].grad, us[l].grad
    return NS(out=cur.detach(), dx=x0.grad, dW=torch.stack([w.grad for w in Wl]), db=torch.stack([v.grad for v in bl]),
              inter=inter)


class _RowsLinear(torch.autograd.Function):
    """F.linear(h, W, b) for W with k nonzeros per row: forward and dL/dh through the structure (gathers / index_add_),
    dL/dW = g^T h dense (it is dense whatever W holds)."""

    @staticmethod
    def forward(ctx, h, W, b):
        cols, sgn = row_structure(W)
        ctx.save_for_backward(h, cols, sgn)
        u = b.expand(h.shape[0], -1).clone()
        for t in range(cols.shape[1]):
            u += h[:, cols[:, t]] * sgn[:, t]
        return u

    @staticmethod
    def backward(ctx, g):
        h, cols, sgn = ctx.saved_tensors
        gh = torch.zeros_like(h)
        for t in range(cols.shape[1]):
            gh.index_add_(1, cols[:, t], g * sgn[:, t])
        return gh, g.t() @ h, g.sum(0)


def rows_linear(h, W, b):
    return _RowsLinear.apply(h, W, b)


def mlp_ref(x, Ws, bs, gout, input_relu=False):
    """Linear/ReLU stack, no activation behind the last layer, plain relu (no kernel masks).  ``input_relu``: x is itself
    relu(z) and the gradient wanted is dL/dz (the raw backward's mask_in form) with its column sums."""
    L = len(Ws)
    z_in = x.clone().requires_grad_()
    h = torch.relu(z_in) if input_relu else z_in
    Wl = [w.clone().requires_grad_() for w in Ws]
    bl = [v.clone().requires_grad_() for v in bs]
    zs, hs = [], []
    for l in range(L):
        z = rows_linear(h, Wl[l], bl[l])
        z.retain_grad()
        zs.append(z)
        if l < L - 1:
            h = torch.relu(z)
            hs.append(h)
    zs[-1].backward(gout)
    gz = [z.grad for z in zs]
    inter = {"x": x, "gout": gout}
    for l in range(L):
        inter[f"W{l}"], inter[f"b{l}"], inter[f"z{l}"], inter[f"gz{l}"] = Ws[l], bs[l], zs[l], gz[l]
    return NS(y=zs[-1].detach(), hidden=[v.detach() for v in hs], gz=gz[:-1], gx=z_in.grad, gb_in=z_in.grad.sum(0),
              dW=[w.grad for w in Wl], db=[v.grad for v in bl], inter=inter,
              alive=[float((v > 0).double().mean()) for v in hs])


def pair_ref(x, W, bias, gout, mode):
    """x (B,N,E), W (P,E,E) [e][h], bias (P,E) | None: T = x_i W_p; mode 0: out[b,p] = sum_h T x_j; mode 1:
    out[b,p,:] = T * x_j + bias_p."""
    B, N, E = x.shape
    I, J = pair_index(N)
    xr = x.clone().requires_grad_()
    Wr = W.clone().requires_grad_()
    br = None if bias is None else bias.clone().requires_grad_()
    T = torch.einsum("bpe,peh->bph", xr[:, I], Wr)
    T.retain_grad()
    out = (T * xr[:, J]).sum(-1) if mode == 0 else T * xr[:, J] + (0 if br is None else br)
    out.backward(gout)
    gT = T.grad
    # the per-pair terms of dL/dx_i and dL/dx_j: the kernels add them up in bf16 rows of up to PB_PPT pairs
    ti = torch.einsum("bph,peh->bpe", gT, W).abs()
    tj = ((gout.unsqueeze(-1) if mode == 0 else gout) * T.detach()).abs()
    sums = torch.zeros(B, N, E, dtype=F64).index_add_(1, I, ti).index_add_(1, J, tj)
    inter = {"x": x, "gout": gout, "W": W, "T": T.detach(), "gT": gT, "out": out.detach(), "gx": xr.grad}
    if bias is not None:
        inter["bias"] = bias
    return NS(out=out.detach(), gx=xr.grad, gW=Wr.grad, gbias=None if br is None else br.grad, inter=inter,
              term_sums={"contribution rows": sums})


def cin_ref(x0, xk, W, bias, gy, same=False, chunk=64):
    """x0 (B,N,E), xk (B,H,E), W (C, N*H) with k nonzeros per row, bias (C), gy (B,C,E):
    y[b,c,e] = bias[c] + sum_{n,h} W[c, n*H+h] x0[b,n,e] xk[b,h,e].  ``same``: xk IS x0 (first layer) -- dx0 is then the
    sum of both gradients.  dW is dense: gy (C, b*E) @ Z (b*E, N*H) over chunks of samples."""
    B, N, E = x0.shape
    a = x0.clone().requires_grad_()
    kk = a if same else xk.clone().requires_grad_()
    H = kk.shape[1]
    C = W.shape[0]
    cols, sgn = row_structure(W)
    br = bias.clone().requires_grad_()
    y = br.view(1, C, 1).expand(B, C, E).clone()
    for t in range(cols.shape[1]):
        y = y + sgn[:, t].view(1, C, 1) * a[:, cols[:, t] // H] * kk[:, cols[:, t] % H]
    y.backward(gy)
    dW = torch.zeros(C, N * H, dtype=F64)
    for s in range(0, B, chunk):
        z = (x0[s:s + chunk].unsqueeze(2) * (x0 if same else xk)[s:s + chunk].unsqueeze(1)).reshape(-1, N * H, E)
        dW += torch.einsum("bce,bke->ck", gy[s:s + chunk], z)
    inter = {"x0": x0, "xk": x0 if same else xk, "W": W, "bias": bias, "gy": gy, "y": y.detach(), "dx0": a.grad}
    if same:
        W3 = W.view(C, N, N)
        inter["W folded"] = torch.tril(W3) + torch.triu(W3, 1).transpose(1, 2)
    else:
        inter["dxk"] = kk.grad
    return NS(y=y.detach(), dx0=a.grad, dxk=None if same else kk.grad, dW=dW, db=br.grad, inter=inter)


def wgrad_ref(g, inp, out_f, in_f):
    """dW = g^T inp over the rows, the first out_f / in_f columns of operands that may be kept wider"""
    return g[:, :out_f].t() @ inp[:, :in_f]


def rows_gemm_ref(g, W, out_f):
    return g[:, :out_f] @ W[:out_f]


# ---------------------------------------------------------------------------------------------------------------------
# case lists (the GPU file runs exactly these; the host file holds each to assert_exact_domain) and their builders
# ---------------------------------------------------------------------------------------------------------------------
# cross: (E, L, rows).  Rows round the 16-row tile, the forward's 8-tile unit, the backward's 96-row group; E = 96 / 128
# (NT = 6 / 8; 128 x 1 resident, 128 x 2 not: backward on the generic kernel); row counts that put nparts at the edges of
# the `p + 48 < nparts` unrolling and one either side of the 256-workgroup cap; one above the resident forward's grid
CROSS_SMALL_ROWS = [1, 15, 16, 17, 95, 96, 97, 127, 128, 129, 191, 193]
CROSS_NPARTS = [1, 16, 17, 49, 64, 65, 256]
CROSS_CASES = ([(E, L, r) for E in (32, 64) for L in (1, 2, 6) for r in CROSS_SMALL_ROWS]
               + [(E, L, r) for E in (96, 128) for L in (1, 2, 4) for r in (1, 16, 17, 127, 128, 129)]
               + [(E, L, B3_ROWS * p) for (E, L) in ((64, 6), (32, 2)) for p in CROSS_NPARTS if p > 1]
               + [(E, L, BW_MAX_BLOCKS * B3_ROWS + d) for (E, L) in ((64, 6), (32, 2)) for d in (-1, 1)]
               + [(64, 2, CROSS_FWD_GRID_RESIDENT * CROSS_FWD_UNIT + 1)])


@functools.lru_cache(maxsize=2)
def cross_case(E, L, rows):
    g = gen(1, E, L, rows)
    x, gout, b = ints((rows, E), g), ints((rows, E), g), ints((L, E), g)
    W = torch.stack([signed_rows(E, E, 1, g) for _ in range(L)])
    return NS(x=x, W=W, b=b, gout=gout, ref={d: cross_ref(x, W, b, gout, d) for d in (True, False)})


# per-pair bilinear: (N, E, B).  N = 2: one pair; 4: a task of exactly PB_PPT; 5: PB_PPT + 1; 39: the last task of a
# field short.  2049 samples: 65 K-steps of 32, more than one split of pair_bilinear_bwd_w
PAIR_TAIL_B = [16, 17, 31, 32, 33, 47, 48, 49, 65, 257, 1000]
PAIR_CASES = ([(N, E, B) for N in (2, 4, 5) for E in (32, 64) for B in PAIR_TAIL_B]
              + [(N, E, 2049) for N in (2, 5) for E in (32, 64)]
              + [(39, 32, B) for B in (17, 49)])
PAIR_FORMS = [(0, False), (1, False), (1, True)]      # (mode, bias)


@functools.lru_cache(maxsize=2)
def pair_case(N, E, B):
    g = gen(2, N, E, B)
    P = N * (N - 1) // 2
    x, W, bias = ints((B, N, E), g), pair_stack(P, E, g), ints((P, E), g)
    gout = {0: ints((B, P), g), 1: ints((B, P, E), g)}
    return NS(x=x, W=W, bias=bias, gout=gout,
              ref={(m, hb): pair_ref(x, W, bias if hb else None, gout[m], m) for m, hb in PAIR_FORMS})


# CIN, channels-last: (form, N, H, C, E, B, k).  'plain': distinct xk; 'fold': xk IS x0, N > 32 (weights folded onto
# h <= n); 'live': last layer, gy zero on the channels [C/2, C); 'live_same': a single layer that is first and last, xk IS
# x0 with N <= 32 (not folded) and the dead half left out
CIN_SHAPES = [(10, 10, 64, 32), (39, 128, 256, 64), (6, 32, 32, 16), (33, 64, 128, 64)]
CIN_SMALL_B = [1, 7, 8, 9, 63, 64, 65]
CIN_FOLD_SHAPES = [(33, 128, 64), (39, 256, 64), (64, 128, 32)]           # (N, C, E)
CIN_CASES = ([("plain", N, H, C, E, B, 2) for (N, H, C, E) in CIN_SHAPES for B in CIN_SMALL_B]
             + [("plain", 10, 10, 64, 32, 300, 2), ("plain", 6, 32, 32, 16, 300, 2)]      # nsplit at its cap of 32
             + [("fold", N, N, C, E, B, 2) for (N, C, E) in CIN_FOLD_SHAPES for B in (1, 9, 65)]
             + [("fold", 33, 33, 128, 64, 520, 2)]                                         # nsplit at its cap of 64
             + [("live", N, H, C, E, B, 2) for (N, H, C, E) in ((39, 128, 256, 64), (33, 64, 128, 64)) for B in (9, 65)]
             + [("live_same", 10, 10, 128, 32, B, 2) for B in (9, 65)])
# the weight gradient of C = 32 / E = 16 is the generic kernel's (the C / E sets of functional.cin_cl_backward_route)
CIN_GENERIC_DW = [(6, 32, 32, 16)]


@functools.lru_cache(maxsize=2)
def cin_case(form, N, H, C, E, B, k):
    g = gen(3, len(form), N, H, C, E, B)
    same = form in ("fold", "live_same")
    x0 = ints((B, N, E), g)
    xk = x0 if same else ints((B, H, E), g)
    W, bias, gy = signed_rows(C, N * H, k, g), ints(C, g), ints((B, C, E), g)
    live = C // 2 if form in ("live", "live_same") else None
    if live:
        gy[:, live:] = 0
    return NS(x0=x0, xk=xk, W=W, bias=bias, gy=gy, live=live, same=same, ref=cin_ref(x0, xk, W, bias, gy, same))


# fused MLP: (widths, k) x rows.  256 * 128 + 1 / 256 * 256 + 1: one row into the second pass of the tile / row-owner
# family's persistent loop
MLP_STACKS = [([64, 400, 400, 400, 64], 2), ([416, 400, 400, 8], 2), ([16, 72, 8], 4), ([64, 512, 64], 4),
              ([32, 104, 200, 40], 4), ([128, 96, 96, 96, 96, 96, 24], 1)]
MLP_RO_STACKS = [[64, 400, 400, 400, 64], [416, 400, 400, 8]]            # covered by the row-owner family
MLP_ROWS = [1, 127, 128, 129, 255, 256, 257, MF_GRID * MF_ROWS + 1, MF_GRID * RO_ROWS + 1]
MLP_CASES = [(tuple(w), k, r) for (w, k) in MLP_STACKS for r in MLP_ROWS]
MLP_MASK_IN_CASES = [(tuple(w), k, r) for (w, k) in MLP_STACKS[:3] for r in (257, MF_GRID * MF_ROWS + 1)]


def _mlp_operands(widths, k, rows, salt):
    g = gen(salt, k, rows, *widths)
    Ws = [signed_rows(o, i, k, g) for i, o in zip(widths[:-1], widths[1:])]
    bs = [ints(o, g) for o in widths[1:]]
    return g, Ws, bs


@functools.lru_cache(maxsize=2)
def mlp_case(widths, k, rows):
    g, Ws, bs = _mlp_operands(widths, k, rows, 4)
    x, gout = ints((rows, widths[0]), g), ints((rows, widths[-1]), g)
    return NS(x=x, Ws=Ws, bs=bs, gout=gout, ref=mlp_ref(x, Ws, bs, gout))


@functools.lru_cache(maxsize=2)
def mlp_mask_in_case(widths, k, rows):
    """the stack behind an upstream ReLU: x = relu(z) in {0, 1}"""
    g, Ws, bs = _mlp_operands(widths, k, rows, 5)
    z, gout = ints((rows, widths[0]), g), ints((rows, widths[-1]), g)
    return NS(x=torch.relu(z), Ws=Ws, bs=bs, gout=gout, ref=mlp_ref(z, Ws, bs, gout, input_relu=True))


# wgrad_rows alone: (out_f, in_f, rows).  Rows round one 32-row step, the 128-row unit of a range, the 256 rows below
# which the kernel is not taken, and 4 * WG_KR * S -+ 1 for S = 8, 16 (> 8); operands kept in pad32 columns with
# nonzero values behind the weight's columns
WGRAD_SHAPES = [(400, 400), (64, 416), (8, 400), (72, 16)]
WGRAD_ROWS = [31, 32, 33, 127, 128, 129, 255, 256, 257, 287, 288, 289, 383, 384, 385,
              4 * WG_KR * 8 - 1, 4 * WG_KR * 8 + 1, 4 * WG_KR * 16 - 1, 4 * WG_KR * 16 + 1]
WGRAD_CASES = [(o, i, r) for (o, i) in WGRAD_SHAPES for r in WGRAD_ROWS]


def pad32(v):
    return (v + 31) // 32 * 32


@functools.lru_cache(maxsize=2)
def wgrad_case(out_f, in_f, rows):
    g = gen(6, out_f, in_f, rows)
    gz, inp = ints((rows, pad32(out_f)), g), ints((rows, pad32(in_f)), g)
    return NS(g=gz, inp=inp, dW=wgrad_ref(gz, inp, out_f, in_f), db=gz[:, :out_f].sum(0))


# rows_gemm: (out_f, in_f, rows, k): y = g[:, :out_f] @ W[:out_f], W with k nonzeros per COLUMN (rows of W^T)
ROWS_GEMM_CASES = [(o, i, r, 4) for o in (64, 400) for i in (1024, 2496) for r in (4096, 4097, 4223, MF_GRID * MF_ROWS + 1)]


@functools.lru_cache(maxsize=2)
def rows_gemm_case(out_f, in_f, rows, k):
    g = gen(7, out_f, in_f, rows)
    Wt = signed_rows(in_f, out_f, k, g)                       # (in_f, out_f): k entries per output column
    x = ints((rows, pad32(out_f) + 32), g)                    # 32 columns of other values behind the operand
    x[:, out_f:pad32(out_f)] = 0                              # the kernel's contract: zeros up to the next multiple of 32
    cols, sgn = row_structure(Wt)
    y = torch.zeros(rows, in_f, dtype=F64)
    for t in range(k):
        y += x[:, cols[:, t]] * sgn[:, t]
    return NS(x=x, W=Wt.t().contiguous(), y=y)

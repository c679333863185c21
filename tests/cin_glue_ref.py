"""Operands, float64 references, the dispatch arithmetic and the case lists that make the CIN glue kernels of
csrc/cin_glue.hip (seven ``trs_cin_glue_*`` entries: BatchNorm1d + ReLU + the direct / hidden split + the pooled sum over
E, forward and backward, with their channels-first by-products) comparable BIT FOR BIT.

The raw entries take scale, shift, mean, invstd, c1 and c2 as plain fp32 vectors, so a test can pick values for which every
product and every sum is exact in fp32 in any order:

    y                  integers in [-4, 4] (bf16)
    scale              {-2, -1, -0.5, 0.5, 1, 2}, negative values in every case (a negative scale flips the side ReLU keeps)
    shift              multiples of 1/2 in [-2, 2]
    mean               integers in [-2, 2]
    invstd             {0.5, 1, 2}
    c1, c2             multiples of 1/4 in [-1, 1]
    g_hidden, g_pooled integers in [-2, 2] (bf16)

z = relu(y * scale + shift) is a multiple of 1/2 of at most 10, gz an integer of at most 4, xhat = (y - mean) * invstd a
multiple of 1/2 of at most 12, gy = scale * (gz * [z > 0] - c1 - xhat * c2) a multiple of 1/16 of at most 34.  About one
pre-activation in twenty is exactly zero, so the strict ``>`` of the mask is exercised.  ``assert_exact_domain`` is the
guard that checks all of that, value by value and sum by sum, on the very operands of a case; tests/test_cin_glue_host.py
runs it over every case below and tests/test_gpu_cin_glue_exact.py takes its cases from the same lists.  A kernel result
is ``expect(ref, dtype)``: the float64 value rounded once.  Nothing here imports torecsys_amd.

Every reference works on tensors of any device: the GPU file computes the float64 references of the large cases on the
device, the host file walks them in chunks of samples."""
import functools
import os
from types import SimpleNamespace as NS

import torch

from exact_ref import CSRC, F64, expect, gen, mismatch      # noqa: F401 (re-exported)

BF16, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch arithmetic of csrc/cin_glue.hip, one line per site (tests/test_cin_glue_host.py pins them to the source)
# ---------------------------------------------------------------------------------------------------------------------
GLUE_THREADS, GLUE_GRID_CAP = 256, 1024
LEGAL_C = [8 << k for k in range(9)]                # 8 times a divisor of 256
LDS_MOST = 160 * 1024                               # what a workgroup of the MI355X can have
PLAIN_LDS = GLUE_THREADS * 8 * 4                    # the block reduction: [rpp][C] fp32 = 8 KiB at every C


def vpr(C):
    """16-byte column vectors per row"""
    return C // 8


def rpp(C):
    """rows a workgroup takes per pass"""
    return GLUE_THREADS // vpr(C)


def glue_grid(B):
    return min(B, GLUE_GRID_CAP)


def glue_shape_ok(C, D, Hs):
    v = C // 8
    return (C % 8 == 0 and 1 <= v <= GLUE_THREADS and GLUE_THREADS % v == 0 and D % 8 == 0 and Hs % 8 == 0
            and 0 <= D <= C and 0 <= Hs <= C)


def glue_cf_ok(C, E):
    return glue_shape_ok(C, 0, 0) and E == 8 * (GLUE_THREADS // (C // 8))


def fwd_cf_lds(C, E, Hs):
    """trs_cin_glue_fwd_cf: the block reduction's 8 KiB and the tile [C - Hs][E + 8] bf16 behind it"""
    return GLUE_THREADS * 8 * 4 + (C - Hs) * (E + 8) * 2


def bwd_cf_lds(C, E):
    """trs_cin_glue_bwd_apply_cf: the tile [C][E + 8] bf16, re-used by the column-sum reduction ([rpp][C] fp32)"""
    return max(C * (E + 8) * 2, (GLUE_THREADS // (C // 8)) * C * 4)


CF_SHAPES = [(8 * rpp(C), C) for C in LEGAL_C]      # (E, C): (2048, 8), (1024, 16), ... (64, 256), (32, 512), ... (8, 2048)

_SITES = [
    "constexpr int GLUE_THREADS = 256;",
    "g.vpr = C / 8;",
    "g.rpp = GLUE_THREADS / g.vpr;",
    "static int glue_grid(int64_t B) { return (int)std::min<int64_t>(B, 1024); }",
    "static bool glue_cf_ok(int C, int E) { return glue_shape_ok(C, 0, 0) && E == 8 * (GLUE_THREADS / (C / 8)); }",
    "return C % 8 == 0 && vpr >= 1 && vpr <= GLUE_THREADS && GLUE_THREADS % vpr == 0 && D % 8 == 0 && Hs % 8 == 0 &&",
    "D >= 0 && D <= C && Hs >= 0 && Hs <= C;",
    "(size_t)GLUE_THREADS * 8 * 4 + (size_t)(C - Hs) * (E + 8) * 2, (hipStream_t)stream,",
    "const size_t lds = std::max((size_t)C * (E + 8) * 2, (size_t)(GLUE_THREADS / (C / 8)) * C * 4);",
]


def source_sites():
    """[(line, matches)]: the host test wants exactly one each"""
    with open(os.path.join(CSRC, "cin_glue.hip")) as f:
        src = f.read()
    return [(line, src.count(line)) for line in _SITES]


def split_kind(C, D, Hs):
    """the six ways [0, D) (pooled) and [Hs, C) (passed on) can lie in [0, C)"""
    if D < Hs:
        return "gap"                    # channels [D, Hs) are neither: no output, exact zeros in the backward
    if D == Hs:
        return "direct_only" if D == C else "hidden_only" if D == 0 else "halves"
    return "all_both" if (D == C and Hs == 0) else "overlap"       # Hs < D: channels [Hs, D) are both


PATTERNS = ("both", "no_hidden", "no_pooled", "none")               # which of g_hidden / g_pooled reach the backward


def dead_channels(C, D, Hs, pattern):
    """bool (C): channels no gradient reaches -- the kernels do not read y there and write exact zeros"""
    c = torch.arange(C)
    return ~((c < D) & (pattern in ("both", "no_hidden"))) & ~((c >= Hs) & (pattern in ("both", "no_pooled")))


# ---------------------------------------------------------------------------------------------------------------------
# operands (seeded, CPU) and the float64 references (any device)
# ---------------------------------------------------------------------------------------------------------------------
def _pick(values, n, g):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), (n,), generator=g)]


def _ints(lo, hi, shape, g):
    """integers in [lo, hi] drawn as int8 (the large cases hold 33 million of them), returned in float64"""
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8).to(F64)


def operands(B, E, C, D, Hs):
    g = gen(71, B, E, C, D, Hs)
    o = NS(B=B, E=E, C=C, D=D, Hs=Hs)
    o.scale = _pick([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], C, g)
    o.scale[torch.randperm(C, generator=g)[:max(1, C // 4)]] *= -1.0          # and then make sure of both signs
    o.scale[0], o.scale[C - 1] = -abs(o.scale[0]), abs(o.scale[C - 1])
    o.shift = _ints(-4, 4, (C,), g) / 2
    o.mean = _ints(-2, 2, (C,), g)
    o.invstd = _pick([0.5, 1.0, 2.0], C, g)
    o.c1, o.c2 = _ints(-4, 4, (C,), g) / 4, _ints(-4, 4, (C,), g) / 4
    o.y = _ints(-4, 4, (B, E, C), g)
    o.g_hidden = _ints(-2, 2, (B, E, C - Hs), g)
    o.g_pooled = _ints(-2, 2, (B, D), g)
    return o


def identity_operands(B, E, C, D, Hs):
    """what F_.cin_glue passes without a BatchNorm module: scale 1, shift 0, mean 0, invstd 1, c1 = c2 = 0"""
    o = operands(B, E, C, D, Hs)
    one, zero = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)
    o.scale, o.shift, o.mean, o.invstd, o.c1, o.c2 = one, zero, zero, one, zero, zero
    return o


def to_device(o, dev):
    return NS(**{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in vars(o).items()})


def samples(o, lo, hi):
    """the operands of samples [lo, hi)"""
    s = NS(**vars(o))
    s.B, s.y, s.g_hidden, s.g_pooled = hi - lo, o.y[lo:hi], o.g_hidden[lo:hi], o.g_pooled[lo:hi]
    return s


def stats_ref(y):
    """(2, C): column sums and sums of squares over (b, e)"""
    return torch.stack([y.sum((0, 1)), (y * y).sum((0, 1))])


def fwd_ref(o):
    pre = o.y * o.scale + o.shift
    z = torch.relu(pre)
    return NS(pre=pre, z=z, hidden=z[..., o.Hs:], pooled=z[..., :o.D].sum(1))


def bwd_ref(o, pattern):
    """sums (2, C) = [dbeta, dgamma]; gy (B, E, C); colsum (C) of gy AS STORED in bf16.  The intermediates ride along for
    the guard."""
    B, E, C = o.y.shape
    gz = torch.zeros_like(o.y)
    if pattern in ("both", "no_hidden"):
        gz[..., :o.D] += o.g_pooled.unsqueeze(1)
    if pattern in ("both", "no_pooled"):
        gz[..., o.Hs:] += o.g_hidden
    m = torch.where(o.y * o.scale + o.shift > 0, gz, torch.zeros_like(gz))
    xc = o.y - o.mean
    xhat = xc * o.invstd
    mx = m * xhat
    t2 = xhat * o.c2
    d1 = m - o.c1
    inner = d1 - t2
    gy = o.scale * inner
    gy[..., dead_channels(C, o.D, o.Hs, pattern).to(gy.device)] = 0.0
    stored = gy.to(BF16).to(F64)
    return NS(gz=gz, m=m, xc=xc, xhat=xhat, mx=mx, t2=t2, d1=d1, inner=inner, gy=gy, stored=stored,
              sums=torch.stack([m.sum((0, 1)), mx.sum((0, 1))]), colsum=stored.sum((0, 1)))


# ---------------------------------------------------------------------------------------------------------------------
# the guard
# ---------------------------------------------------------------------------------------------------------------------
def _multiples(name, t, q):
    """every value is an integer multiple of q below 2**24 q: exact in fp32"""
    u = t / q
    assert torch.equal(u, u.round()), f"{name}: not multiples of {q}"
    assert float(u.abs().max()) < 2 ** 24 if u.numel() else True, f"{name}: reaches 2**24 x {q}"


def _bf16_exact(name, t):
    assert torch.equal(t.to(BF16).to(F64), t), f"{name}: changes in a bf16 round trip"


def assert_exact_domain(o, pattern="both", both_signs=True):
    """Shows for one case that (1) every fp32 value the kernels form is an integer multiple of a fixed power of two with
    fewer than 24 bits, (2) every fp32 accumulation -- the pooled sum of a sample and, per workgroup and column, the two
    statistics, dbeta, dgamma and the column sums of the stored gy -- is of such multiples with a sum of MAGNITUDES below
    2**24 quanta, so every partial sum in any order is exact, (3) every tensor stored in bf16 is therefore the single
    rounding of an exact fp32 value, and (4) the fp32 sums do equal the float64 ones.  A workgroup takes the samples
    b = blk, blk + grid, ...; the case is walked in chunks of ``grid`` samples.  -> the largest magnitude sum in quanta."""
    B, E, C, G = o.B, o.E, o.C, glue_grid(o.B)
    for name in ("scale", "shift", "mean", "invstd", "c1", "c2"):
        t = getattr(o, name)
        assert torch.equal(t.to(F32).to(F64), t), name
    assert not both_signs or (bool((o.scale < 0).any()) and bool((o.scale > 0).any())), "scale: both signs"
    acc = {k: torch.zeros(G, C, dtype=F64) for k in ("sum y", "sum y^2", "dbeta", "dgamma", "colsum")}
    quantum = {"sum y": 1.0, "sum y^2": 1.0, "dbeta": 1.0, "dgamma": 0.5, "colsum": 1.0 / 16}
    worst, zeros, total = 0.0, 0, 0
    for lo in range(0, B, G):
        s = samples(o, lo, min(B, lo + G))
        n = s.B
        for name in ("y", "g_hidden", "g_pooled"):
            _bf16_exact(name, getattr(s, name))
        f = fwd_ref(s)
        _multiples("y * scale", s.y * s.scale, 0.5)
        _multiples("z", f.z, 0.5)
        zeros, total = zeros + int((f.pre == 0).sum()), total + f.pre.numel()
        pooled_mag = f.z.abs().sum(1) / 0.5                                          # (n, C): one sample's sum over E
        worst = max(worst, float(pooled_mag.max()))
        r = bwd_ref(s, pattern)
        for name, q in (("gz", 1.0), ("m", 1.0), ("xc", 1.0), ("xhat", 0.5), ("mx", 0.5), ("t2", 0.125), ("d1", 0.25),
                        ("inner", 0.125), ("gy", 1.0 / 16), ("stored", 1.0 / 16)):
            _multiples(name, getattr(r, name), q)
        acc["sum y"][:n] += s.y.abs().sum(1)
        acc["sum y^2"][:n] += (s.y * s.y).sum(1)
        acc["dbeta"][:n] += r.m.abs().sum(1)
        acc["dgamma"][:n] += r.mx.abs().sum(1) / 0.5
        acc["colsum"][:n] += r.stored.abs().sum(1) / (1.0 / 16)
        # (4) on this chunk: fp32 sums, forwards and over a shuffled order, have the bits of the float64 sums
        # (the serial sum in a shuffled order only up to 2**21 values: the bound on the magnitudes is the proof)
        perm = torch.randperm(n * E, generator=gen(72, lo)) if n * E * C <= 1 << 21 else None
        for name, t in (("y", s.y), ("y^2", s.y * s.y), ("m", r.m), ("mx", r.mx), ("stored gy", r.stored)):
            rows = t.reshape(n * E, C)
            want = rows.sum(0)
            assert torch.equal(rows.to(F32).sum(0).to(F64), want), f"fp32 sum of {name}"
            if perm is not None:
                assert torch.equal(rows[perm].to(F32).cumsum(0)[-1].to(F64), want), f"shuffled serial fp32 sum of {name}"
        assert torch.equal(f.z.to(F32).sum(1).to(F64), f.z.sum(1)), "fp32 pooled sum"
    for name, a in acc.items():
        worst = max(worst, float(a.max()))
        assert float(a.max()) < 2 ** 24, f"{name}: magnitude sum {float(a.max())} quanta of {quantum[name]}"
    assert worst < 2 ** 24
    return NS(worst=worst, zeros=zeros, values=total, zero_fraction=zeros / max(total, 1))


# ---------------------------------------------------------------------------------------------------------------------
# case lists: (B, E, C, D, Hs)
# ---------------------------------------------------------------------------------------------------------------------
# thread layouts: all nine C; rpp > E (idle row groups feed the block reduction), E no multiple of rpp above it, E a
# multiple, rpp = 1; all six split kinds.  C = 8 admits (D, Hs) in {0, 8}^2 only: one case each
LAYOUT_CASES = [
    (3, 3, 8, 8, 0),              # rpp 256 > E;            all_both
    (2, 5, 8, 8, 8),              #                         direct_only: no hidden tensor
    (2, 5, 8, 0, 0),              #                         hidden_only: no pooled tensor
    (2, 5, 8, 0, 8),              #                         gap over every channel: no output at all, gy all zeros
    (3, 300, 16, 8, 8),           # rpp 128, E = 2 rpp + 44; halves
    (5, 70, 32, 24, 8),           # rpp 64,  E = rpp + 6;    overlap
    (4, 33, 64, 16, 40),          # rpp 32,  E = rpp + 1;    gap
    (3, 7, 128, 64, 64),          # rpp 16 > E
    (3, 17, 256, 256, 0),         # rpp 8,   E = 2 rpp + 1
    (3, 16, 256, 128, 128),       # rpp 8,   E = 2 rpp
    (3, 5, 512, 256, 264),        # rpp 4,   E = rpp + 1;    gap of one vector
    (2, 3, 1024, 512, 8),         # rpp 2,   E = rpp + 1;    overlap
    (2, 3, 2048, 1024, 1024),     # rpp 1
    (2, 1, 2048, 2048, 0),        # rpp 1, E = 1
]
# the grid-stride loop: 1025 gives workgroup 0 a second sample, above 2048 a third
STRIDE_CASES = [(1025, 3, 8, 8, 0), (2049, 3, 16, 8, 8), (2500, 2, 64, 40, 24), (1025, 5, 512, 256, 256)]
PLAIN_CASES = LAYOUT_CASES + STRIDE_CASES
# trs_cin_glue_stats as the column sum of a (B, P, E) gradient (functional._pair_bias_grad): 741 pairs of 8
STATS_PAIR_CASES = [(5, 741, 8, 0, 0), (1030, 45, 16, 0, 0)]


def _cf_hs(C):
    return sorted({h for h in (0, 8, C // 2) if h % 8 == 0})


def _cf_d(C, Hs, i):
    """a D for the i-th channels-first case: halves, overlap, all pooled and a gap in turn"""
    return [Hs, min(C, Hs + 8), C, max(0, Hs - 8)][i % 4]


# every channels-first shape with Hs in {0, 8, C / 2} (those that are multiples of 8); the swizzle depends on rpp, Hs and E / 8
CF_SMALL_CASES = [(3, E, C, _cf_d(C, Hs, i + j), Hs) for i, (E, C) in enumerate(CF_SHAPES) for j, Hs in enumerate(_cf_hs(C))]
# the second and third pass re-use the LDS tile behind barriers.  Every channels-first shape has 16 384 values per sample
CF_STRIDE_CASES = [(1025, 8, 2048, 1024, 1024), (1025, 2048, 8, 8, 0), (2049, 64, 256, 128, 128)]
CF_CASES = CF_SMALL_CASES + CF_STRIDE_CASES
ALL_CASES = PLAIN_CASES + STATS_PAIR_CASES + CF_CASES
BIG = 1 << 22                     # cases above this many values run the "both" pattern only


def case_patterns(case):
    B, E, C, D, Hs = case
    return PATTERNS if B * E * C <= BIG else ("both",)


def case_id(c):
    return "B{}-E{}-C{}-D{}-Hs{}".format(*c)


@functools.lru_cache(maxsize=2)
def glue_case(B, E, C, D, Hs):
    return operands(B, E, C, D, Hs)


# F_.cin_glue end to end: (B, E, C, D, Hs)
E2E_NOBN_CASES = [(1025, 32, 512, 256, 256), (1030, 5, 64, 40, 24)]           # channels-first and not, B > 1024
E2E_BN_CASES = [(16, 64, 256, 128, 128), (8, 4, 64, 64, 0)]                    # R = B E = 1024 and 32


def bn_operands(B, E, C, D, Hs):
    """a training-mode BatchNorm1d(C, eps=0) is exact when every channel takes the values mu_c +- 1, half of the R = B E
    rows each (R a power of two): mean = mu, variance = 1, invstd = 1, and c1 = dbeta / R, c2 = dgamma / R are dyadic.
    weight in {-2, -1, -0.5, 0.5, 1, 2}, bias a multiple of 1/2; every fourth channel has bias = -weight or +weight, so one
    side's pre-activation is exactly zero."""
    R = B * E
    assert R & (R - 1) == 0
    g = gen(73, B, E, C, D, Hs)
    o = NS(B=B, E=E, C=C, D=D, Hs=Hs)
    mu = _ints(-2, 2, (C,), g)
    side = torch.stack([torch.randperm(R, generator=g) for _ in range(C)], 1) < R // 2        # (R, C): half on each side
    o.y = (mu + torch.where(side, 1.0, -1.0).to(F64)).view(B, E, C)
    o.weight = _pick([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], C, g)
    o.weight[0], o.weight[C - 1] = -abs(o.weight[0]), abs(o.weight[C - 1])
    o.bias = _ints(-4, 4, (C,), g) / 2
    o.bias[::4] = o.weight[::4] * torch.where(torch.arange(0, C, 4) % 8 == 0, 1.0, -1.0).to(F64)
    o.running_mean0 = _ints(-2, 2, (C,), g)
    o.running_var0 = _pick([0.5, 1.0, 2.0], C, g)
    o.mean, o.invstd = mu, torch.ones(C, dtype=F64)
    o.scale, o.shift = o.weight * o.invstd, o.bias - mu * o.weight * o.invstd
    o.g_hidden = _ints(-2, 2, (B, E, C - Hs), g)
    o.g_pooled = _ints(-2, 2, (B, D), g)
    o.c1 = o.c2 = torch.zeros(C, dtype=F64)
    r = bwd_ref(o, "both")                              # the sums do not depend on c1 / c2
    o.c1, o.c2 = r.sums[0] / R, r.sums[1] / R
    return o


def assert_bn_exact(o):
    """the premises of ``bn_operands`` and the exactness of what follows from them in fp32"""
    R, C = o.B * o.E, o.C
    rows = o.y.reshape(R, C)
    _bf16_exact("y", o.y)
    assert torch.equal(rows.sum(0) / R, o.mean)
    assert torch.equal((rows * rows).sum(0) / R - o.mean * o.mean, torch.ones(C, dtype=F64))
    f = fwd_ref(o)
    assert int((f.pre == 0).sum()) > 0 and bool((o.weight < 0).any())
    _multiples("z", f.z, 0.5)
    assert float(f.z.abs().sum(1).max()) / 0.5 < 2 ** 24
    r = bwd_ref(o, "both")
    q = 1.0 / (16 * R)
    for name, t, qq in (("c1", o.c1, 1.0 / R), ("c2", o.c2, 0.5 / R), ("d1", r.d1, 1.0 / R), ("t2", r.t2, 0.5 / R),
                        ("inner", r.inner, 0.5 / R), ("gy", r.gy, q)):
        _multiples(name, t, qq)
        assert torch.equal(t.to(F32).to(F64), t), name
    assert o.B <= GLUE_GRID_CAP                          # one sample per workgroup: its sums run over E rows
    for name, t, qq in (("dbeta", r.m, 1.0), ("dgamma", r.mx, 1.0), ("colsum", r.stored, q)):
        _multiples(name, t, qq)
        assert float(t.abs().sum(1).max()) / qq < 2 ** 24, name
    return r

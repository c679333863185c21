"""Operands and float64 references that make csrc/moe.hip, csrc/senet.hip and the loss half of csrc/rank.hip comparable
BIT FOR BIT, the case lists the three GPU files run, and the dispatch arithmetic of the three sources restated.

MoE gate.  A row (b, g) has ``n`` live columns whose logits + bias are one small integer c_row and dead columns at -20000:
expf(z - max) is 1 or 0, the sum is n, P is 1 / n or 0 (n a power of two).  experts and gout are integers in [-2, 2], so
out = P e, glogits = P (t - sum P t) and gexperts = sum_g gout P are dyadic rationals with short numerators: exact in fp32
in any order of summation, and the bf16 results are those values rounded once.  A wrong bias or logits index makes the
live columns of a row unequal, which no longer gives 1 / n.

SENET.  x and gout are sparse integers in [-2, 2], the four parameters integers in [-1, 1].  With E a power of two every
value of the layer is a multiple of 1 / E; for other E the row sums of x are made multiples of E and W1 holds multiples
of E, so that S * fl(1 / E) and gz * fl(1 / E) round to integers.  ``senet_guard`` holds every sum the kernels take below
2**24 quanta and checks that fp32 reaches the float64 bits in three summation orders.  Pre-activations of exactly 0
occur by themselves; torch.relu has derivative 0 there, as the kernels (``a > 0.f``, ``hv > 0.f``, the ``hh == 0.f`` skip).

Ranking losses.  Scores are multiples of 1 / 4 in [-4, 4]; with margin 0.625 no hinge argument is 0, with margin 1.0 many
are.  tests/rank_ref.py is the reference (``clamp``: derivative 1 at exactly 0).

tests/test_gate_exact_host.py proves the operands exact and the coverage complete on the CPU; tests/test_gpu_moe_exact.py,
tests/test_gpu_senet_exact.py and tests/test_gpu_rank_loss_exact.py run the lists.  Nothing here imports torecsys_amd."""
import functools
import os
import re
from types import SimpleNamespace as NS

import torch

from exact_ref import CSRC, expect, gen, mismatch  # noqa: F401  (re-exported for the three GPU files)
from rank_ref import rank_loss_ref, rank_terms
from senet_ref import compose, pre_activations

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = [F32, BF16]


def dt_tag(d):
    return "fp32" if d == F32 else "bf16"


def size_of(dtype):
    return 4 if dtype == F32 else 2


class Diffs(list):
    """collects ``mismatch`` messages; ``done`` fails with all of them"""

    def check(self, where, name, got, ref):
        want = ref if got.dtype == F64 else expect(ref, got.dtype)
        if got.shape == want.shape and torch.equal(got, want.to(got.device)):
            return
        self.append(mismatch(f"{where} {name}", got, want))

    def done(self):
        assert not self, "\n".join(self)


# ---------------------------------------------------------------------------------------------------------------------
# constants of the three sources the case lists sit on
# ---------------------------------------------------------------------------------------------------------------------
_CONST_SITES = {
    "MOE_LANE_COLS": ("moe.hip", r"constexpr int MOE_LANE_COLS = (\d+);"),
    "MOE_TILE_COLS": ("moe.hip", r"constexpr int MOE_TILE_COLS = (\d+);"),
    "MOE_GRID_VEC": ("moe.hip", r"const int grid = stream_grid\(B << lg, 256, 256 \* (\d+)\);"),
    "MOE_GRID_FWD_ELEM": ("moe.hip", r"dim3\(stream_grid\(B \* G \* 64, 256, 256 \* (\d+)\)\)"),
    "MOE_GRID_BWD_ELEM": ("moe.hip", r"dim3\(stream_grid\(B \* 64, 256, 256 \* (\d+)\)\)"),
    "SENET_MAX_M": ("senet.hip", r"constexpr int SENET_MAX_M = (\d+);"),
    "SENET_MAX_VEC": ("senet.hip", r"constexpr int SENET_MAX_VEC = (\d+);"),
    "SENET_MAX_BLOCKS": ("senet.hip", r"constexpr int SENET_MAX_BLOCKS = (\d+);"),
    "SENET_FIN_SEG": ("senet.hip", r"constexpr int SENET_FIN_SEG = (\d+);"),
    "SENET_LDS_KIB": ("senet.hip", r"senet_bwd_lds\(M, H, nvec, nw\) > (\d+) \* 1024\) nw >>= 1;"),
    "SENET_ROW_GRID": ("senet.hip", r"const int grid = stream_grid\(rows << lg, 256, 256 \* (\d+)\);"),
    "SENET_SCALE_GRID": ("senet.hip", r"const int grid = stream_grid\(rows \* units, 256, 256 \* (\d+)\);"),
    "RANK_BLOCK": ("rank.hip", r"constexpr int RANK_BLOCK = (\d+);"),
    "RANK_MAX_BLOCKS": ("rank.hip", r"constexpr int RANK_MAX_BLOCKS = (\d+);"),
    "RANK_FINISH_LANES": ("rank.hip", r"for \(int i = threadIdx.x; i < n; i \+= (\d+)\) \{\n    acc \+= partial\[i\];"),
}
_TEXT_SITES = {
    "SENET_STEPS": ("senet.hip", r"static const int steps\[\] = \{([0-9, ]+)\};"),
    "SENET_DISPATCH": ("senet.hip", r"dispatch_int<([0-9, ]+)>\(senet_vec_per_lane"),
    "MOE_DISPATCH_LG": ("moe.hip", r"if \(lg < 6\) dispatch_int<([0-9, ]+)>\(lg,"),
}


def source_constants():
    """every constant above as the sources spell it (an assertion error when a site is gone or doubled)"""
    out = {}
    for sites, conv in ((_CONST_SITES, int), (_TEXT_SITES, lambda s: [int(v) for v in s.split(",")])):
        for name, (fname, pat) in sites.items():
            with open(os.path.join(CSRC, fname)) as f:
                m = re.findall(pat, f.read())
            assert len(m) == 1, (name, fname, m)
            out[name] = conv(m[0])
    return out


MOE_LANE_COLS, MOE_TILE_COLS, STREAM_GRID_CAP = 16, 8, 256 * 16
MOE_MAX_K = 64 * MOE_LANE_COLS
SENET_MAX_M, SENET_MAX_VEC, SENET_MAX_BLOCKS, SENET_FIN_SEG, SENET_LDS_CAP = 64, 16, 1024, 8, 64 * 1024
SENET_STEPS = [1, 2, 4, 5, 8, 10, 16]
RANK_BLOCK, RANK_MAX_BLOCKS, RANK_FINISH_LANES = 256, 256, 64
CUS, FWD_BLOCKS_PER_CU = 256, 8           # an upper bound on what is resident: 2048 threads per CU, 256 per workgroup


def stream_grid(work_items, block=256, cap=STREAM_GRID_CAP):
    """trs_common.hpp"""
    return max(1, min(-(-work_items // block), cap))


def log2_group(units):
    """the smallest lg <= 6 with 2**lg >= units (moe_gate_launch, senet_log2_group)"""
    lg = 0
    while (1 << lg) < units and lg < 6:
        lg += 1
    return lg


# ---------------------------------------------------------------------------------------------------------------------
# MoE gate
# ---------------------------------------------------------------------------------------------------------------------
VECTOR, ELEMENT = 1, 2                     # functional.MOE_PATH_VECTOR / MOE_PATH_ELEMENT


def moe_vector_shape(K, dtype):
    return K >= 1 and K % 4 == 0 and (K * size_of(dtype)) % 16 == 0 and K <= MOE_MAX_K


def moe_path(K, dtype, aligned=True):
    return VECTOR if moe_vector_shape(K, dtype) and aligned else ELEMENT


def moe_group(K, dtype):
    """(lg, R, NV) of the vector path's instantiation: moe_gate_launch restated"""
    assert moe_vector_shape(K, dtype)
    NV = K * size_of(dtype) // 16
    lg = log2_group(NV)
    per_lane = -(-NV // (1 << lg))
    R = 1 if lg < 6 else {1: 1, 2: 2, 3: 4, 4: 4}[per_lane]
    return lg, R, NV


def moe_fill(K, dtype):
    """'full': every lane of a group owns a vector in every round; 'part': the last lanes of the last round own none"""
    lg, R, NV = moe_group(K, dtype)
    return "full" if NV == R << lg else "part"


def moe_bwd_tiles(K):
    """column tiles of moe_gate_bwd_elem_kernel"""
    return -(-K // (64 * MOE_TILE_COLS))


def moe_trips(path, B, G, K, dtype, bwd):
    """passes of the kernel's grid-stride loop"""
    if path == VECTOR:
        lg = moe_group(K, dtype)[0]
        groups = stream_grid(B << lg) * 256 >> lg
        return -(-B // groups)
    owners = B if bwd else B * G
    waves = stream_grid(owners * 64) * 256 >> 6
    return -(-owners // waves)


MOE_B, MOE_GS = 67, (1, 3, 4)
MOE_VECTOR_K = {F32: [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 768, 772, 1024],
                BF16: [8, 16, 24, 32, 40, 64, 72, 128, 136, 256, 264, 512, 520, 1024]}
MOE_ELEMENT_K = {F32: [1, 2, 3, 15, 63, 65, 511, 513, 1028, 2051],
                 BF16: [1, 2, 3, 15, 63, 65, 511, 513, 1028, 2051, 4, 12, 20]}
MOE_UNALIGNED_K = 64
# (dtype, K, G, B): the grid-stride loop's second trip
MOE_TRIP_VECTOR = [(F32, 256, 1, 16389), (BF16, 512, 1, 16389), (F32, 4, 1, 1048581)]
MOE_TRIP_ELEMENT = [(F32, 3, 1, 16389), (BF16, 3, 1, 16389)]


def moe_case_id(c):
    return "%s_K%d" % (dt_tag(c[0]), c[1]) + ("" if len(c) == 2 else "_G%d_B%d" % (c[2], c[3]))


MOE_VECTOR_CASES = [(d, K) for d in DTYPES for K in MOE_VECTOR_K[d]]
MOE_ELEMENT_CASES = [(d, K) for d in DTYPES for K in MOE_ELEMENT_K[d]]
MOE_DEAD = -20000.0


def moe_operands(B, G, K, bias, salt=0):
    """float64 operands on the CPU (n in {1, 2, 4, 8}, at most the largest power of two in K): logits (B, G*K) WITHOUT the bias, bias (G*K) | None, experts (B, K), gout (B, G, K),
    live (B, G, K) bool, n (B, G).  Row 0 keeps its first n columns (column 0), the last row its last n (column K - 1);
    for a power-of-two K every fifth row has all K columns live."""
    g = gen(31, B, G, K, int(bias), salt)
    rows = B * G
    n = (2 ** torch.randint(0, 4, (rows,), generator=g)).clamp(max=1 << (K.bit_length() - 1))      # a power of two <= K
    if K & (K - 1) == 0:
        n[2::5] = K
    r = torch.rand(rows, K, generator=g)
    r[0] = torch.arange(K) / K
    r[-1] = torch.arange(K - 1, -1, -1) / K
    thr = r.sort(dim=1).values.gather(1, (n - 1).view(-1, 1))
    live = r <= thr
    assert torch.equal(live.sum(1), n) and bool(live[:, 0].any()) and bool(live[:, K - 1].any())
    c = ((torch.arange(rows) * 5) % 7 - 3).to(F64).view(-1, 1)
    z = torch.where(live, c, torch.full((), MOE_DEAD, dtype=F64)).view(B, G * K)
    b = torch.randint(-2, 3, (G * K,), generator=g).to(F64) if bias else None
    logits = z - b if bias else z
    e = torch.randint(-2, 3, (B, K), generator=g).to(F64)
    gout = torch.randint(-2, 3, (B, G, K), generator=g).to(F64)
    return NS(B=B, G=G, K=K, logits=logits, bias=b, experts=e, gout=gout, live=live.view(B, G, K), n=n.view(B, G))


def moe_ref(o):
    """the float64 reference: a plain softmax of logits + bias, autograd for the two gradients"""
    lg = o.logits.clone().requires_grad_()
    e = o.experts.clone().requires_grad_()
    z = lg if o.bias is None else lg + o.bias
    P = torch.softmax(z.view(o.B, o.G, o.K), dim=2)
    out = P * e.unsqueeze(1)
    out.backward(o.gout)
    return NS(P=P.detach(), out=out.detach(), glogits=lg.grad, gexperts=e.grad)


def assert_moe_exact(o, r):
    """what the docstring claims, on the operands themselves: fp32-exact logits and sums, P = 1 / n or 0, results that
    fp32 holds exactly"""
    for name in ("logits", "experts", "gout") + (("bias",) if o.bias is not None else ()):
        t = getattr(o, name)
        assert torch.equal(t.to(F32).to(F64), t), name
    z = o.logits if o.bias is None else (o.logits.to(F32) + o.bias.to(F32)).to(F64)
    zz = z.view(o.B, o.G, o.K)
    assert torch.equal(zz == MOE_DEAD, ~o.live) and bool((zz[o.live].abs() <= 3).all())
    want = o.live.to(F64) / o.n.to(F64).unsqueeze(-1)
    assert torch.equal(r.P, want), "the float64 softmax is not 1 / n on the live columns"
    assert bool(((o.n & (o.n - 1)) == 0).all())
    for name in ("out", "glogits", "gexperts"):
        t = getattr(r, name)
        assert torch.equal(t.to(F32).to(F64), t), f"{name} is not exact in fp32"
        q = t * float(o.n.max()) ** 2
        assert torch.equal(q, q.round()) and float(q.abs().max()) < 2 ** 24, name
    # the sums a lane group folds: sum_k |P t| in quanta of 1 / n stays far below 2**24
    t = (o.gout * o.experts.unsqueeze(1)).abs()
    assert float((t * o.live).sum(2).max()) < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------------
# ranking losses
# ---------------------------------------------------------------------------------------------------------------------
RANK_SIZES = [(B, K) for B in (1, 255, 256, 257, 16384, 16385, 65536, 65537, 70001) for K in (1, 3)] + [(257, 33)]
RANK_POW2_SIZES = [(B, K) for B in (257, 16385, 65537) for K in (1, 2, 4)]
RANK_MARGINS = (0.625, 1.0)
RANK_EXACT_KINDS = ("hinge", "adaptive_hinge")
RANK_SMOOTH_KINDS = ("pointwise", "bpr")
RANK_MASKS = ("none", "all", "drop_block", "last_only")
RANK_GOUTS = (1.0, 0.5, 2.0)


def rank_id(c):
    return "B%d_K%d" % c


def rank_partials(B):
    """workgroups of rank_loss_partial_kernel = partials the finish kernel adds"""
    return min(RANK_MAX_BLOCKS, -(-B // RANK_BLOCK))


def rank_finish_trips(B):
    return -(-rank_partials(B) // RANK_FINISH_LANES)


def rank_partial_trips(B):
    return -(-B // (rank_partials(B) * RANK_BLOCK))


@functools.lru_cache(maxsize=4)
def rank_scores(B, K):
    """float64 (B, 1 + K) multiples of 1 / 4 in [-4, 4].  Sample 0 is p = 1, n = 0: at margin 1.0 every hinge argument
    of it is exactly 0 and all its negatives tie for the maximum."""
    g = gen(41, B, K)
    s = torch.randint(-16, 17, (B, 1 + K), generator=g).to(F64) / 4
    s[0, 0] = 1.0
    s[0, 1:] = 0.0
    return s


def rank_mask(B, pattern):
    """None | (B,) bool"""
    if pattern == "none":
        return None
    m = torch.ones(B, dtype=torch.bool)
    if pattern == "drop_block":          # the second workgroup's samples, or the first's where there is one only
        lo = RANK_BLOCK if B > RANK_BLOCK else 0
        m[lo:lo + RANK_BLOCK] = False
        if not m.any():
            m[-1] = True
    elif pattern == "last_only":
        m[:-1] = False
    else:
        assert pattern == "all"
    return m


def rank_pow2_mask(B, j, salt=0):
    """(B,) bool that keeps 2**j samples, sample 0 and the last among them"""
    keep = 1 << j
    assert 2 <= keep <= B
    g = gen(43, B, j, salt)
    m = torch.zeros(B, dtype=torch.bool)
    m[0] = m[-1] = True
    rest = torch.randperm(B - 2, generator=g)[:keep - 2] + 1
    m[rest] = True
    assert int(m.sum()) == keep
    return m


def rank_ref(s, kind, margin, mask, reduction, gout=1.0):
    """float64 loss, kept count, gradient (B, 1 + K) of ``gout * loss``"""
    sr = s.clone().requires_grad_()
    loss = rank_loss_ref(sr[:, 0], sr[:, 1:], kind, margin, mask, reduction)
    (loss * gout).backward()
    kept = s.shape[0] if mask is None else int(mask.sum())
    return NS(loss=loss.detach(), kept=kept, grad=sr.grad)


def rank_divisor(kind, K, kept, reduction):
    """rank_denominator restated"""
    if reduction == "sum":
        return 1
    if reduction == "mean":
        return kept if kind == "adaptive_hinge" else kept * K
    return kept


def rank_hinge_args(s, kind, margin):
    """the arguments of the clamp: (B, K), or (B, 1) for the adaptive hinge"""
    p, n = s[:, :1], s[:, 1:]
    return margin - p + (n.max(dim=1, keepdim=True)[0] if kind == "adaptive_hinge" else n)


def rank_tied_first(s):
    """(B,) bool: several negatives share the maximum"""
    n = s[:, 1:]
    return (n == n.max(dim=1, keepdim=True)[0]).sum(1) > 1


def rank_term_quanta(s, kind, margin):
    """sum of |terms| in eighths: what the partial and finish kernels add up in fp32"""
    t = rank_terms(s[:, 0], s[:, 1:], kind, margin) * 8
    assert torch.equal(t, t.round())
    return float(t.abs().sum())


# ---------------------------------------------------------------------------------------------------------------------
# SENET, fused family
# ---------------------------------------------------------------------------------------------------------------------
def senet_vec_per_lane(M, E, dtype):
    """the K step of senet_dispatch_k"""
    nvec = M * (E * size_of(dtype) // 16)
    k = -(-nvec // 64)
    return next(s for s in SENET_STEPS if k <= s)


def senet_fused_ok(M, H, E, dtype):
    rb = E * size_of(dtype)
    return 0 < M <= SENET_MAX_M and 1 <= H <= M and rb % 16 == 0 and M * rb <= SENET_MAX_VEC * 64 * 16


def senet_quad_floats(M, H):
    return 4 * (-(-M // 4) * H + -(-H // 4) * M)


def senet_bwd_lds(M, H, nvec, nw):
    P = 2 * M * H + M + H
    return 4 * (senet_quad_floats(M, H) + nw * P + nw * (2 * nvec + 128))


def senet_bwd_waves(M, H, E, dtype):
    nvec = M * (E * size_of(dtype) // 16)
    nw = 4
    while nw > 1 and senet_bwd_lds(M, H, nvec, nw) > SENET_LDS_CAP:
        nw >>= 1
    return nw


def senet_slabs(B, M, H, E, dtype):
    """workgroups of the backward when the device holds at least SENET_MAX_BLOCKS of them, else an upper bound"""
    nw = senet_bwd_waves(M, H, E, dtype)
    return max(1, min(-(-B // nw), SENET_MAX_BLOCKS))


# (dtype, M, H, E, B).  Every K step in both dtypes with H from {1, 2, 3, 13, M}; M % 4 and H % 4 of every residue;
# E = 12 / 24 / 48: no power of two
SENET_B = 67
SENET_STEP_SHAPES = {
    F32: {1: [(3, 3, 8), (64, 13, 4), (7, 2, 24), (5, 3, 12)], 2: [(5, 5, 64)], 4: [(64, 1, 16), (13, 13, 64)],
          5: [(39, 3, 32), (17, 2, 64)], 8: [(30, 13, 64)], 10: [(39, 39, 64)],
          16: [(45, 13, 64), (63, 2, 64), (64, 64, 64)]},
    BF16: {1: [(3, 2, 8), (64, 3, 8), (7, 7, 24)], 2: [(64, 13, 16)], 4: [(64, 1, 32), (39, 13, 48)], 5: [(39, 2, 64)],
           8: [(64, 64, 64)], 10: [(39, 39, 128)], 16: [(50, 3, 128), (64, 13, 128)]},
}
SENET_STEP_CASES = [(d, M, H, E, SENET_B) for d in DTYPES for k in SENET_STEPS for (M, H, E) in SENET_STEP_SHAPES[d][k]]
# the backward's wave counts: nw = 1 with more than 64 KiB of dynamic LDS, nw = 2, (nw = 4: every small case)
SENET_WAVE_CASES = [(d, 64, 64, 16, SENET_B) for d in DTYPES] + [(d, 64, 32, 16, SENET_B) for d in DTYPES]
# slabs 1, 1, 2, 7, 8, 9, 17 at nw = 4: the empty and the short segments of senet_finish_kernel
SENET_SLAB_B = [1, 3, 5, 28, 32, 33, 67]
SENET_SLAB_CASES = [(d, 13, 3, 32, B) for d in DTYPES for B in SENET_SLAB_B]
# a wave's second sample, forward (at most 8 workgroups of 4 waves on each of 256 CUs) and backward (1024 x 4)
SENET_TRIP_B = 8197
SENET_TRIP_CASES = [(d, M, H, E, SENET_TRIP_B) for d in DTYPES for (M, H, E) in ((2, 2, 4 if d == F32 else 8), (3, 2, 8))]
SENET_FUSED_CASES = SENET_STEP_CASES + SENET_WAVE_CASES + SENET_SLAB_CASES + SENET_TRIP_CASES
SENET_PARTIAL_CASES = [(F32, 13, 3, 32, 33), (BF16, 39, 2, 64, 33)]


def senet_id(c):
    return "%s_M%d_H%d_E%d_B%d" % (dt_tag(c[0]), c[1], c[2], c[3], c[4])


def _sparse(shape, g, lo=-2, hi=2, density=0.25):
    v = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    return v * (torch.rand(shape, generator=g) < density)


def _rows_multiple_of(x, E, g):
    """the last entry of every row moved so that the row sum is -E, 0 or E (a third each): the sum of a sparse row is
    far below E by itself, and its nearest multiple would be 0 nearly always"""
    s = x.sum(-1)
    x = x.clone()
    x[..., -1] += torch.randint(-1, 2, s.shape, generator=g).to(F64) * E - s
    return x


def pow2(v):
    return v & (v - 1) == 0


def senet_check(o):
    """the non-degeneracy conditions of a fused case -> list of the ones that fail.  With H = 1 no sample can hold a dead
    hidden unit beside a live one: there both states must occur over the batch instead, and 'between 20 % and 80 %'
    needs at least 5 units x samples to be decidable, so it is asked for H * B >= 5 only (the gates: M * B >= 5)."""
    z, u, v = pre_activations(o.x, o.W1, o.b1, o.W2, o.b2)
    bad = []
    live_h, live_a = float((u > 0).double().mean()), float((v > 0).double().mean())
    if u.numel() >= 5 and not 0.2 <= live_h <= 0.8:
        bad.append(f"{live_h:.2f} of the hidden units live")
    if v.numel() >= 5 and not 0.2 <= live_a <= 0.8:
        bad.append(f"{live_a:.2f} of the gates live")
    if not bool((u == 0).any()):
        bad.append("no hidden pre-activation of exactly 0")
    if not bool((v == 0).any()):
        bad.append("no gate pre-activation of exactly 0")
    dead, alive = (u <= 0).any(1), (u > 0).any(1)
    if o.H > 1 and not bool((dead & alive).any()):
        bad.append("no dead hidden unit beside a live one")
    if o.H == 1 and not (bool(dead.any()) and bool(alive.any())):
        bad.append("the one hidden unit does not take both states over the batch")
    r = senet_ref(o)
    for name in ("dW1", "db1", "dW2", "db2"):
        if not bool((getattr(r, name) != 0).any()):
            bad.append(f"{name} is zero")
    return bad


def _senet_draw(dtype, M, H, E, B, salt):
    g = gen(51, size_of(dtype), M, H, E, B, salt)
    x, gout = _sparse((B, M, E), g), _sparse((B, M, E), g)
    # few samples: denser operands, or a gradient has nothing to be built from
    if B < 8:
        x, gout = _sparse((B, M, E), g, density=0.6), _sparse((B, M, E), g, density=0.6)
    scale = 1 if pow2(E) else E
    if scale != 1:
        x = _rows_multiple_of(x, E, g)
    W1 = torch.randint(-1, 2, (H, M), generator=g).to(F64) * scale
    W2 = torch.randint(-1, 2, (M, H), generator=g).to(F64)
    b1 = torch.randint(-1, 2, (H,), generator=g).to(F64)
    b2 = torch.randint(-1, 2, (M,), generator=g).to(F64)
    # tiny layers: random weights tend to kill every gate; the biases decide.  The policies rotate with the salt
    policy = salt % 4
    if policy == 1:
        b2 = (torch.arange(M) % 2).to(F64)
    elif policy == 2:
        b1, b2 = (torch.arange(H) % 2).to(F64), (torch.arange(M) % 3 - 1).to(F64)
    elif policy == 3:
        b1, b2 = ((torch.arange(H) + 1) % 2).to(F64), ((torch.arange(M) + 1) % 2).to(F64)
    return NS(dtype=dtype, M=M, H=H, E=E, B=B, x=x, gout=gout, W1=W1, b1=b1, W2=W2, b2=b2, salt=salt)


@functools.lru_cache(maxsize=4)
def senet_case(dtype, M, H, E, B):
    """the first draw (salt 0, 1, ...) that meets ``senet_check``"""
    assert senet_fused_ok(M, H, E, dtype)
    for salt in range(200):
        o = _senet_draw(dtype, M, H, E, B, salt)
        if not senet_check(o):
            return o
    raise AssertionError(f"no draw of {senet_id((dtype, M, H, E, B))} meets the conditions: {senet_check(o)}")


def senet_ref(o, need_x=True, need_params=True):
    """float64 autograd through senet_ref.compose (torch.relu: derivative 0 at 0)"""
    x = o.x.clone().requires_grad_(need_x)
    P = [t.clone().requires_grad_(need_params) for t in (o.W1, o.b1, o.W2, o.b2)]
    out = compose(x, *P)
    if need_x or need_params:
        out.backward(o.gout)
    return NS(out=out.detach(), dx=x.grad, dW1=P[0].grad, db1=P[1].grad, dW2=P[2].grad, db2=P[3].grad)


def _three_orders(terms, dim, what):
    """the fp32 sum of ``terms`` along ``dim`` forwards, backwards and pairwise has the float64 sum's bits"""
    want = terms.sum(dim)
    t32 = terms.to(F32).movedim(dim, 0)
    assert torch.equal(t32.to(F64), terms.movedim(dim, 0)), f"{what}: a term is not an fp32 value"
    fwd = torch.zeros_like(t32[0])
    for i in range(t32.shape[0]):
        fwd = fwd + t32[i]
    bwd = torch.zeros_like(t32[0])
    for i in range(t32.shape[0] - 1, -1, -1):
        bwd = bwd + t32[i]
    pw = t32
    while pw.shape[0] > 1:
        if pw.shape[0] % 2:
            pw = torch.cat([pw, torch.zeros_like(pw[:1])])
        pw = pw[0::2] + pw[1::2]
    for name, got in (("forwards", fwd), ("backwards", bwd), ("pairwise", pw[0])):
        assert torch.equal(got.to(F64), want), f"{what}: the fp32 sum taken {name} differs from float64"


def senet_guard(o, orders=True):
    """every sum the fused kernels take, as (name, terms, dim): sum of |terms| in quanta of 1 / E below 2**24 (for E no
    power of two every value is an integer: quanta of 1), and -- ``orders`` -- three fp32 summation orders against
    float64.  For E no power of two also |S / E| and |gz / E| <= 4096, the range over which S * fl(1 / E) was verified
    to round to the integer.  -> the largest sum of |terms| in quanta"""
    E, q = o.E, (o.E if pow2(o.E) else 1)
    z, u, v = pre_activations(o.x, o.W1, o.b1, o.W2, o.b2)
    h, a = torch.relu(u), torch.relu(v)
    ga = (o.gout * o.x).sum(2)
    gv = ga * (v > 0)
    gu = (gv @ o.W2) * (u > 0)
    gz = gu @ o.W1
    one = lambda t: t.unsqueeze(-1)                                          # noqa: E731
    sums = [("row sums of x", o.x, 2, 1),
            ("W1 z + b1", torch.cat([o.W1.unsqueeze(0) * z.unsqueeze(1), one(o.b1.expand_as(u))], 2), 2, q),
            ("W2 h + b2", torch.cat([o.W2.unsqueeze(0) * h.unsqueeze(1), one(o.b2.expand_as(v))], 2), 2, q),
            ("ga = sum g x", o.gout * o.x, 2, 1),
            ("gu = W2^T gv", o.W2.t().unsqueeze(0) * gv.unsqueeze(1), 2, 1),
            ("gz = W1^T gu", o.W1.t().unsqueeze(0) * gu.unsqueeze(1), 2, 1),
            ("dW1 = sum_b gu z", gu.unsqueeze(2) * z.unsqueeze(1), 0, q),
            ("db1 = sum_b gu", gu, 0, 1),
            ("dW2 = sum_b gv h", gv.unsqueeze(2) * h.unsqueeze(1), 0, q),
            ("db2 = sum_b gv", gv, 0, 1)]
    worst = 0.0
    for name, terms, dim, quantum in sums:
        tq = terms * quantum
        assert torch.equal(tq, tq.round()), f"{name}: terms are not multiples of 1 / {quantum}"
        top = float(tq.abs().sum(dim).max())
        assert top < 2 ** 24, f"{name}: sum of |terms| {top} quanta"
        worst = max(worst, top)
        if orders:
            _three_orders(terms, dim, name)
    if not pow2(E):
        assert float(z.abs().max()) <= 4096 and float((gz / E).abs().max()) <= 4096
        for t in (z, gz / E):
            assert torch.equal(t, t.round())
        for S in (o.x.sum(2), gz):                                           # the device's own product, on this CPU
            got = S.to(F32) * torch.tensor(1.0, dtype=F32).div(torch.tensor(float(E), dtype=F32))
            assert torch.equal(got.to(F64), S / E), "S * fl(1 / E) does not round to S / E"
    # single products and the two-term results: exact when they are fp32 values
    r = senet_ref(o)
    for name in ("out", "dx", "dW1", "db1", "dW2", "db2"):
        t = getattr(r, name)
        assert torch.equal(t.to(F32).to(F64), t), f"{name} is not an fp32 value"
    for name, t in (("x", o.x), ("gout", o.gout), ("W1", o.W1), ("b1", o.b1), ("W2", o.W2), ("b2", o.b2)):
        assert torch.equal(t.to(o.dtype).to(F64), t), f"{name} changes in {o.dtype}"
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# SENET, general family: rows of E values, the gates given
# ---------------------------------------------------------------------------------------------------------------------
# (dtype, E, rows as (B, M), offset): vector rows at every group width, element rows, a pointer 4 bytes off, a second trip
SENET_ROW_VECTOR_E = [4, 8, 12, 16, 32, 64, 128, 256, 1024]
SENET_ROW_ELEMENT_E = [1, 3, 10, 70]
SENET_ROWS_TRIP = (F32, 256, 16389, 1, False)
SENET_ROW_CASES = ([(F32, E, 23, 3, False) for E in SENET_ROW_VECTOR_E + SENET_ROW_ELEMENT_E]
                   + [(BF16, E, 23, 3, False) for E in (8, 24, 128, 1024, 5)]
                   + [(F32, 16, 23, 3, True), SENET_ROWS_TRIP])


def senet_row_id(c):
    return "%s_E%d_B%d_M%d%s" % (dt_tag(c[0]), c[1], c[2], c[3], "_off" if c[4] else "")


def senet_row_path(E, dtype, aligned=True):
    """(vector?, units a group strides over, lg) of senet_rowsum_launch"""
    vec = (E * size_of(dtype)) % 16 == 0 and aligned
    units = E * size_of(dtype) // 16 if vec else E
    return vec, units, log2_group(units)


def senet_row_trips(rows, E, dtype, aligned=True):
    """(trips of senet_rowsum_kernel, trips of senet_rowscale_kernel)"""
    vec, units, lg = senet_row_path(E, dtype, aligned)
    groups = stream_grid(rows << lg) * 256 >> lg
    return -(-rows // groups), -(-(rows * units) // (stream_grid(rows * units) * 256))


@functools.lru_cache(maxsize=2)
def senet_row_case(dtype, E, B, M, off):
    """x, gout sparse integers with row sums of x multiples of E (E no power of two), gates a multiples of 1 / 4 in
    [0, 2] (a quarter of them 0), gz (the gradient arriving at the means) integers times E"""
    g = gen(61, size_of(dtype), E, B, M, int(off))
    dens = 0.25 if E >= 8 else 0.6
    x, gout = _sparse((B, M, E), g, density=dens), _sparse((B, M, E), g, density=dens)
    if not pow2(E):
        x = _rows_multiple_of(x, E, g)
    a = torch.randint(0, 9, (B, M), generator=g).to(F64) / 4 * (torch.rand(B, M, generator=g) < 0.75)
    gz = torch.randint(-3, 4, (B, M), generator=g).to(F64) * E
    z = x.sum(2) / E
    return NS(dtype=dtype, E=E, B=B, M=M, x=x, gout=gout, a=a, gz=gz, z=z, out=x * a.unsqueeze(-1),
              ga=(gout * x).sum(2), dx_scale=gout * a.unsqueeze(-1), dx_squeeze=(gz / E).unsqueeze(-1).expand(B, M, E),
              dx=gout * a.unsqueeze(-1) + (gz / E).unsqueeze(-1))


def senet_row_guard(o):
    assert float(o.x.abs().sum(2).max()) < 2 ** 24 and float((o.gout * o.x).abs().sum(2).max()) < 2 ** 24
    _three_orders(o.x, 2, "row sums")
    _three_orders(o.gout * o.x, 2, "ga")
    q = o.E if pow2(o.E) else 1
    for name in ("z", "out", "ga", "dx", "dx_scale", "dx_squeeze"):
        t = getattr(o, name) * (4 * q)
        assert torch.equal(t, t.round()) and float(t.abs().max()) < 2 ** 24, name
    assert float(o.z.abs().max()) <= 4096 and float((o.gz / o.E).abs().max()) <= 4096
    inv = torch.tensor(1.0, dtype=F32).div(torch.tensor(float(o.E), dtype=F32))
    for S in (o.x.sum(2), o.gz):
        assert torch.equal((S.to(F32) * inv).to(F64), S / o.E), "S * fl(1 / E) does not round to S / E"
    for name in ("x", "gout"):
        t = getattr(o, name)
        assert torch.equal(t.to(o.dtype).to(F64), t), name
    return float(max(o.x.abs().sum(2).max(), (o.gout * o.x).abs().sum(2).max()))


# a whole general-family layer: M = 65 fields (above SENET_MAX_M), H = 13, and H = 0 (reduction above M: gates relu(b2))
SENET_LAYER_CASES = [(d, 65, r, 16, 33) for d in DTYPES for r in (5, 66)]          # (dtype, M, reduction, E, B)


def senet_layer_id(c):
    return "%s_M%d_r%d_E%d_B%d" % (dt_tag(c[0]), c[1], c[2], c[3], c[4])


@functools.lru_cache(maxsize=2)
def senet_layer_case(dtype, M, reduction, E, B):
    H = M // reduction
    for salt in range(200):
        o = _senet_draw(dtype, M, H, E, B, 1000 + salt)
        if H == 0:
            o.b2 = (torch.arange(M) % 3 - 1).to(F64)
            return o
        if not senet_check(o):
            return o
    raise AssertionError("no draw meets the conditions")

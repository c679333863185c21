"""Operands, a float64 reference and dispatch mirrors that make EVERY attentional-FM kernel path of csrc/afm.hip comparable
BIT FOR BIT: the bf16 matrix-core kernels (afm_fwd_mfma_kernel<AT, KS>, afm_bwd_mfma_kernel<AT, KS, 4> under its three tile
schedules) and the generic kernels (afm_fwd_kernel<T>, afm_bwd_kernel<T, AMAX, ES>) in bf16 and fp32.

The obstacle is the softmax; it becomes exact when the logits of a sample take two kinds of value only: K "live" pairs with
bit-identical logits, K a power of two, and every other pair so far below them that its ``exp`` is 0 in fp32.  The scores are
then 1 / K or 0, and the output, d(logit) = s_p (ds_p - sum_q s_q ds_q), d(hidden), W1^T dh, dx, dW1, db1 and dw2 are dyadic
rationals of a handful of bits; db2 is 0.  A correct kernel of either family returns ``expect(ref, dtype)``.

The construction (``afm_operands``):
  * coordinate 0 of every field row is a TAG in {-1, 0, 1}: per sample p fields carry +1 and m fields -1, (p, m) = (2, 0),
    (2, 2), (3, 2), (5, 4) for K = C(p, 2) + C(m, 2) = 1, 2, 4, 16, every other field 0, the tagged fields drawn per sample;
  * unit 0 is the PENALTY unit: W1[0] = -e_0, b1[0] = 1, w2[0] = -PENALTY.  A pair whose tags multiply to +1 has
    pre-activation 0 (no penalty, and a dead ReLU in the backward), every other pair 1 or 2: PENALTY or 2 PENALTY below.
    PENALTY is 2048, not 1024: the other units move a logit by at most 5 (A - 1) <= 635 in all, so every dead logit stays
    more than 1024 below the live ones whatever the other units say (the host guard checks it case by case);
  * every other unit has k (2..4) entries of +-1 on a column set S that leaves the tag out (``support_cols``: the low half,
    the odd columns or the high half), b1 in {-1, 0, 1}, w2 in {-1, 1}; b2 = 1;
  * on S all "+" fields of a sample share one row u and all "-" fields one row v.  With |v| = |u| every live pair would have
    the SAME product row on S and the same hidden vector, and because sum_live d(logit) = 0 the gradients of b1, w2 and of
    W1 on S would vanish identically.  So S is split in two halves matched by an involution pi, |v| = pi(|u|), and the units
    come in twins W1[a'] = W1[a] o pi with equal b1 and w2 (an odd one out is pi-symmetric): the "-" pairs see the hidden
    vector of the "+" pairs with every twin swapped -- the logits agree bit for bit, the hidden vectors do not, and db1, dw2
    and dW1 on S are sums over the "+" pairs alone or the "-" pairs alone, which do not cancel;
  * |u| is a random 0 / 1 pattern per sample, but all ones in sample 0 and all zeros in sample 1, and every unit is drawn so
    that it is alive under exactly one of those two: no unit is dead (or alive) throughout a case.  In sample 2 |u| is the
    first half of S (so |v| the second): every column of S then meets a d(hidden) sum over one sign of pairs only;
  * off S and in the untagged fields x is random in {-1, 0, 1};
  * g_out has two entries of +-1 per row, g_attn is in {-1, 0, 1} and is then moved by +-1 on kept live pairs until
    sum_live ds is a multiple of K (values in {-2..2}), so d(logit) = (ds_p - mean) / K; with g_attn absent g_out is redrawn
    until that holds.  Only ``grad_samples(B)`` carry gradients (all of them up to B = 8; above, the first, the last and
    those either side of the grid caps), so the summed parameter gradients stay within bf16; the forward is compared in full;
  * score dropout with p = 0.5 / 0.75: keep_scale 2 / 4 and a fixed mask.

fp32 premises the comparison rests on: __expf(0) == 1; __expf(t) == 0 for t <= -1024; division by a power of two is exact
(no fast-math in the build).  ``afm_path`` and the functions above it restate the dispatch arithmetic of afm.hip; the case
lists are DERIVED from them and tests/test_exact_afm_host.py pins every restated line to the source text (one match per
site).  tests/test_gpu_exact_afm.py runs exactly these lists.  Nothing here imports torecsys_amd."""
import functools
import math
import os
import re
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from exact_ref import CSRC, F64, assert_exact_domain, expect, gen, mismatch, pair_index      # noqa: F401 (re-exported)

BF16, F32 = torch.bfloat16, torch.float32
PENALTY = 2048.0
LIVE_FIELDS = {1: (2, 0), 2: (2, 2), 4: (3, 2), 16: (5, 4)}          # K -> ("+" fields, "-" fields)


def dtype_tag(v):
    return {BF16: "bf16", F32: "fp32"}.get(v, str(v))


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch arithmetic of csrc/afm.hip (and the schedule of trs_common.hpp), one line per site
# ---------------------------------------------------------------------------------------------------------------------
AFM_MAX, AFM_TILE_MAX = 128, 112
BWD_MFMA_GRID, GENERIC_GRID, FWD_MFMA_GRID_MOST = 256, 256 * 4, 256 * 8    # the last: 256 CUs x at most 8 workgroups of 4 waves
LDS_PLAIN, LDS_MOST = 64 * 1024, 160 * 1024                                # above LDS_PLAIN a launch raises the attribute


def sched_rounds(N):
    return N if N & 1 else N - 1


def sched_width(N):
    return (N + 1) // 2


def sched_entry(r, k, N):
    M = N + 1 if N & 1 else N
    R = M - 1
    a, b = (r, M - 1) if k == 0 else ((r + k) % R, (r - k + R) % R)
    return None if a >= N or b >= N else (min(a, b), max(a, b))


def afm_fwd_mfma_lds(N, E):
    P = N * (N - 1) // 2; PT = (P + 15) // 16
    return ((N * (E * 2 + 16) + 15) & ~15) + PT * 16 * 12 + E * 4 + 64


def afm_bwd_mfma_lds(N, E, A, T=0, waves=4):
    P = N * (N - 1) // 2; PP = (P + 15) & ~15
    R = sched_rounds(N); H = sched_width(N); TPR = (H + 15) // 16
    NT = T if T > 0 else R * TPR
    grad = max(waves * N * (E + 4) * 4, (A * E + 2 * A + 1) * 4)
    return ((N * (E * 2 + 16) + 15) & ~15) + PP * 16 + E * 4 + 64 + NT * 64 + grad + waves * (A + E) * 80 + 64


def afm_lds_floats(N, E, A, bwd):
    P = N * (N - 1) // 2
    return N * E + E * A * (2 if bwd else 1) + 2 * A + P * (3 if bwd else 2) + E + (4 * A if bwd else 0) + 8


def generic_fwd_lds(N, E, A):
    return afm_lds_floats(N, E, A, False) * 4


def generic_bwd_lds(N, E, A):
    """trs_afm_bwd_dropout asks this of EVERY shape, before it looks at the matrix-core kernel"""
    return (afm_lds_floats(N, E, A, True) + N * E + A * E + sched_rounds(N) * sched_width(N)) * 4


def fwd_mfma_ok(N, E, A, dtype, aligned=True):
    return dtype == BF16 and E in (32, 64, 128) and A % 16 == 0 and A <= 128 and afm_fwd_mfma_lds(N, E) <= 64 * 1024 and aligned


def bwd_mfma_ok(N, E, A, dtype, aligned=True):
    return (dtype == BF16 and E in (32, 64, 128) and A % 32 == 0 and A <= 128 and (A // 16) * (E // 32) <= 12
            and afm_bwd_mfma_lds(N, E, A) <= 160 * 1024 and aligned)


@functools.lru_cache(maxsize=None)
def packed_tiles(N):
    """afm_packed_tiles restated: a greedy pass over the pairs in round order (circle method over M players), a pair taken
    when both of its fields are still free in the 16-pair tile being filled.  -> (tiles, 0 when they do not fit
    AFM_TILE_MAX else their number).  The source keeps the fields of a tile in a 64-bit mask: N <= 64 only."""
    assert 2 <= N <= 64
    M = N if N & 1 else N - 1
    rem = []
    for r in range(M):
        for d in range(1, M // 2 + 1):
            a, b = ((r - d) % M + M) % M, (r + d) % M
            rem.append((min(a, b), max(a, b)))
        if not N & 1:
            rem.append((r, N - 1))
    tiles = []
    while rem and len(tiles) < AFM_TILE_MAX:
        used, tile, keep = set(), [], []
        for pr in rem:
            if len(tile) < 16 and pr[0] not in used and pr[1] not in used:
                tile.append(pr)
                used.update(pr)
            else:
                keep.append(pr)
        rem = keep
        tiles.append(tile)
    return tiles, (0 if rem else len(tiles))


def bwd_schedule(N):
    """-> NS(kind in 'rounds' | 'packed' | 'tpr2' | 'tpr3', NT tiles of a sample, TPR, T the kernel argument)"""
    H = sched_width(N); TPR = (H + 15) // 16
    T = packed_tiles(N)[1] if N <= 64 else 0
    if N <= 32:
        T = 0
    NT = T if T > 0 else sched_rounds(N) * TPR
    return NS(kind="packed" if T > 0 else "rounds" if TPR == 1 else f"tpr{TPR}", NT=NT, TPR=TPR, T=T)


def schedule_tiles(N):
    """the tiles of a sample as the kernel builds them in LDS: lists of (i, j), None for an empty slot"""
    s = bwd_schedule(N)
    if s.T > 0:
        return [t + [None] * (16 - len(t)) for t in packed_tiles(N)[0]]
    H = sched_width(N)
    out = []
    for t in range(s.NT):
        r, k0 = divmod(t, s.TPR)
        out.append([sched_entry(r, 16 * k0 + n, N) if 16 * k0 + n < H else None for n in range(16)])
    return out


def wave_tiles(N):
    """tiles each of the four waves takes per sample (tile = wave, wave + 4, ...)"""
    NT = bwd_schedule(N).NT
    return [len(range(w, NT, 4)) for w in range(4)]


def generic_bwd_inst(E, A):
    return (32 if A <= 32 else 64 if A <= 64 else 128), (1 if E <= 64 else 2)


def afm_path(N, E, A, dtype, aligned=True):
    """what trs_afm_fwd_dropout / trs_afm_bwd_dropout launch.  fwd, bwd in 'mfma' | 'generic' | 'unsupported' (more than
    160 KiB of LDS: the entry refuses the shape); AT, KS of either matrix-core kernel; sched of the matrix-core backward;
    AMAX, ES of the generic backward"""
    assert N >= 2 and 1 <= E <= AFM_MAX and 1 <= A <= AFM_MAX and dtype in (BF16, F32)
    p = NS(fwd=None, bwd=None, fwd_AT=None, bwd_AT=None, KS=None, sched=None, AMAX=None, ES=None)
    if fwd_mfma_ok(N, E, A, dtype, aligned):
        p.fwd, p.fwd_AT, p.KS = "mfma", A // 16, E // 32
    else:
        p.fwd = "generic" if generic_fwd_lds(N, E, A) <= LDS_MOST else "unsupported"
    if generic_bwd_lds(N, E, A) > LDS_MOST:
        p.bwd = "unsupported"
    elif bwd_mfma_ok(N, E, A, dtype, aligned):
        p.bwd, p.bwd_AT, p.KS, p.sched = "mfma", A // 16, E // 32, bwd_schedule(N).kind
    else:
        p.bwd = "generic"
        p.AMAX, p.ES = generic_bwd_inst(E, A)
    return p


# source text each mirror restates: (function the line stands in, the line).  The body of a function is the text from its
# head to the first "\n}\n" behind it.
_HEADS = {
    "fwd_lds": "static size_t afm_fwd_mfma_lds(",
    "bwd_lds": "static size_t afm_bwd_mfma_lds(",
    "lds_floats": "__host__ __device__ inline size_t afm_lds_floats(",
    "tiles": "static const AfmTiles* afm_packed_tiles(",
    "grid": "static int afm_grid(",
    "trs_fwd": 'extern "C" int trs_afm_fwd_dropout(',
    "trs_bwd": 'extern "C" int trs_afm_bwd_dropout(',
    "trs_tiles": 'extern "C" int trs_afm_pair_tiles(',
    "fwd_mfma_kernel": "void afm_fwd_mfma_kernel(",
    "bwd_mfma_kernel": "void afm_bwd_mfma_kernel(",
    "fwd_kernel": "void afm_fwd_kernel(",
    "bwd_kernel": "void afm_bwd_kernel(",
}
_SITES = [
    ("fwd_lds", "const int P = N * (N - 1) / 2, PT = (P + 15) / 16;"),
    ("fwd_lds", "return (size_t)((N * (E * 2 + 16) + 15) & ~15) + (size_t)PT * 16 * 12 + (size_t)E * 4 + 64;"),
    ("bwd_lds", "const int P = N * (N - 1) / 2, PP = (P + 15) & ~15;"),
    ("bwd_lds", "const int R = afm_rounds(N), H = afm_width(N), TPR = (H + 15) / 16;"),
    ("bwd_lds", "const int NT = T > 0 ? T : R * TPR;"),
    ("bwd_lds", "const size_t grad = std::max<size_t>((size_t)waves * N * (E + 4) * 4, ((size_t)A * E + 2 * A + 1) * 4);"),
    ("bwd_lds", "return (size_t)((N * (E * 2 + 16) + 15) & ~15) + (size_t)PP * 16 + (size_t)E * 4 + 64 + (size_t)NT * 64 + grad +"),
    ("bwd_lds", "(size_t)waves * (A + E) * 80 + 64;"),
    ("lds_floats", "return (size_t)N * E + (size_t)E * A * (bwd ? 2 : 1) + 2 * A + (size_t)P * (bwd ? 3 : 2) + E + (bwd ? 4 * A : 0) + 8;"),
    ("tiles", "const int M = (N & 1) ? N : N - 1;"),
    ("tiles", "for (int d = 1; d <= M / 2; ++d) {"),
    ("tiles", "const int a = ((r - d) % M + M) % M, b = (r + d) % M;"),
    ("tiles", "if (!(N & 1)) rem.emplace_back(r, N - 1);"),
    ("tiles", "while (!rem.empty() && nt < AFM_TILE_MAX) {"),
    ("tiles", "if (cnt < 16 && !(used & m)) {"),
    ("tiles", "en->n = rem.empty() ? nt : 0;"),
    ("grid", "static int afm_grid(int64_t B) { return (int)std::min<int64_t>(B, 256 * 4); }"),
    ("trs_fwd", "if (dtype == TRS_BF16 && (E == 32 || E == 64 || E == 128) && A % 16 == 0 && A <= 128 &&"),
    ("trs_fwd", "afm_fwd_mfma_lds(N, E) <= 64 * 1024 && aligned16(x) && aligned16(W1)) {"),
    ("trs_fwd", "if (cap_lds != lds) { cap = resident_blocks((const void*)kern, 256, lds); cap_lds = lds; }"),
    ("trs_fwd", "const int grid = (int)std::min<int64_t>(B, cap);"),
    ("trs_fwd", "const size_t lds = afm_lds_floats(N, E, A, P, false) * 4;"),
    ("trs_fwd", "TRS_REQUIRE(lds <= 160 * 1024, TRS_ESHAPE,"),
    ("trs_fwd", "if (lds > 64 * 1024 &&"),
    ("trs_fwd", "hipLaunchKernelGGL(kern, dim3(afm_grid(B)), dim3(256), lds, s,"),
    ("trs_bwd", "const size_t lds = (afm_lds_floats(N, E, A, P, true) + (size_t)N * E + (size_t)A * E +"),
    ("trs_bwd", "(size_t)afm_rounds(N) * afm_width(N)) * 4;"),
    ("trs_bwd", "TRS_REQUIRE(lds <= 160 * 1024, TRS_ESHAPE,"),
    ("trs_bwd", "if (dtype == TRS_BF16 && (E == 32 || E == 64 || E == 128) && A % 32 == 0 && A <= 128 &&"),
    ("trs_bwd", "(A / 16) * (E / 32) <= 12 &&"),
    ("trs_bwd", "afm_bwd_mfma_lds(N, E, A) <= 160 * 1024 && aligned16(x) && aligned16(W1)) {"),
    ("trs_bwd", "const AfmTiles* packed = N <= 64 ? afm_packed_tiles(N, &T) : &no_tiles;"),
    ("trs_bwd", "if (N <= 32) T = 0;"),
    ("trs_bwd", "const int mgrid = (int)std::min<int64_t>(B, 256);"),
    ("trs_bwd", "if (mlds > 64 * 1024 &&"),
    ("trs_bwd", "const int grid = afm_grid(B);"),
    ("trs_bwd", "if (E <= 64) {"),
    ("trs_bwd", "if (A <= 32) TRS_AFM_B(T_, 32, 1);"),
    ("trs_bwd", "else if (A <= 64) TRS_AFM_B(T_, 64, 1);"),
    ("trs_bwd", "else TRS_AFM_B(T_, 128, 1);"),
    ("trs_bwd", "if (A <= 32) TRS_AFM_B(T_, 32, 2);"),
    ("trs_bwd", "else if (A <= 64) TRS_AFM_B(T_, 64, 2);"),
    ("trs_bwd", "else TRS_AFM_B(T_, 128, 2);"),
    ("trs_tiles", "TRS_REQUIRE(N >= 2 && N <= 64 && tiles && ntiles && capacity >= 0, TRS_EINVAL,"),
    ("fwd_mfma_kernel", "constexpr int E = 32 * KS, A = 16 * AT, RS = E * 2 + 16;"),
    ("fwd_mfma_kernel", "for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {"),
    ("fwd_mfma_kernel", "for (int pt = wave; pt < PT; pt += 4) {"),
    ("bwd_mfma_kernel", "const int R = afm_rounds(N), H = afm_width(N), TPR = (H + 15) / 16;"),
    ("bwd_mfma_kernel", "const int NT = T > 0 ? T : R * TPR;"),
    ("bwd_mfma_kernel", "const int r = t / (TPR * 16), k = t - r * (TPR * 16);"),
    ("bwd_mfma_kernel", "sched[t] = k < H ? sched_entry(r, k, N) : -1;"),
    ("bwd_mfma_kernel", "for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {"),
    ("bwd_mfma_kernel", "for (int tile = wave; tile < NT; tile += WAVES) {"),
    ("bwd_mfma_kernel", "const int col = 16 * (tiles_done & 1) + n;"),
    ("bwd_mfma_kernel", "const bool last = tile + WAVES >= NT;"),
    ("bwd_mfma_kernel", "if ((tiles_done & 1) == 0 || last) {"),
    ("bwd_mfma_kernel", "if (tiles_done & 1) ++tiles_done;"),
    ("fwd_kernel", "for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {"),
    ("bwd_kernel", "for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {"),
    ("bwd_kernel", "const int R = afm_rounds(N), H = afm_width(N);"),
]
_COMMON_SITES = [
    r"__host__ __device__ inline int sched_rounds\(int N\) \{ return \(N & 1\) \? N : N - 1; \}",
    r"__host__ __device__ inline int sched_width\(int N\) \{ return \(N \+ 1\) / 2; \}",
    r"const int M = \(N & 1\) \? N \+ 1 : N;",
    r"a = \(r \+ k\) % R; b = \(r - k \+ R\) % R;",
    r"if \(a >= N \|\| b >= N\) return -1;",
    r"return cus \* blocks;",
]
_CONST_SITES = [r"constexpr int AFM_MAX = 128;", r"constexpr int AFM_TILE_MAX = 112;",
                r"auto kern = afm_bwd_mfma_kernel<AT_, KS_, 4>;", r"if constexpr \(AT_ \* KS_ <= 12\) \{"]


def source_sites():
    """[(where, line, matches)]: the host test wants exactly one each"""
    with open(os.path.join(CSRC, "afm.hip")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "trs_common.hpp")) as f:
        common = f.read()
    out = []
    for fn, line in _SITES:
        assert src.count(_HEADS[fn]) == 1, (fn, src.count(_HEADS[fn]))
        s = src.index(_HEADS[fn])
        out.append((fn, line, src[s:src.index("\n}\n", s)].count(line)))
    out += [("trs_common.hpp", pat, len(re.findall(pat, common))) for pat in _COMMON_SITES]
    out += [("afm.hip", pat, len(re.findall(pat, src))) for pat in _CONST_SITES]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference: the formula of oracle.cpu_ref.afm_layer plus autograd, in chunks of samples
# ---------------------------------------------------------------------------------------------------------------------
def _bf16_ok(t):
    return bool(torch.equal(t.to(BF16).to(F64), t))


def afm_ref(x, W1, b1, w2, b2, g_out=None, g_attn=None, keep=None, keep_scale=1.0, chunk_elems=1 << 23):
    """x (B, N, E), W1 (A, E), b1 (A), w2 (A), b2 (1), g_out (B, E) | None, g_attn (B, P) | None, keep (B, P) 0 / 1 | None,
    all float64.  ``attn`` is what the layer returns (the dropped scores under a mask), ``attn0`` the softmax itself.
    d(logit) and d(hidden) are too large to keep at the largest cases: they are reduced chunk by chunk into ``facts``."""
    B, N, E = x.shape
    A = W1.shape[0]
    I, J = pair_index(N)
    P = I.numel()
    ps = [t.clone().requires_grad_() for t in (W1, b1, w2, b2)]
    for p in ps:
        p.grad = torch.zeros_like(p)
    out, attn, attn0, gx = (torch.empty(B, E, dtype=F64), torch.empty(B, P, dtype=F64), torch.empty(B, P, dtype=F64),
                            torch.zeros(B, N, E, dtype=F64))
    live = torch.zeros(B, P, dtype=torch.bool)
    facts = NS(dead_gap=math.inf, dl_bf16=True, dh_bf16=True, dl_max=0.0,
               alive=torch.zeros(A, dtype=torch.int64), dead=torch.zeros(A, dtype=torch.int64))
    # samples whose output gradients are all zero owe exactly zero to every gradient: they run without autograd
    has_g = torch.zeros(B, dtype=torch.bool)
    for gr in (g_out, g_attn):
        if gr is not None:
            has_g |= gr.abs().sum(1) > 0
    step = max(1, chunk_elems // (P * max(E, A)))
    for rows, with_grad in ((has_g.nonzero().flatten(), True), ((~has_g).nonzero().flatten(), False)):
        for s in range(0, rows.numel(), step * (1 if with_grad else 2)):
            r = rows[s:s + step * (1 if with_grad else 2)]
            with torch.set_grad_enabled(with_grad):
                xs = x[r].clone().requires_grad_(with_grad)
                prod = xs[:, I] * xs[:, J]
                pre = F.linear(prod, ps[0], ps[1])
                logit = F.linear(torch.relu(pre), ps[2].view(1, A), ps[3]).squeeze(-1)
                sm = torch.softmax(logit, dim=1)
                a = sm if keep is None else sm * (keep[r].to(F64) * keep_scale)
                o = (prod * a.unsqueeze(-1)).sum(dim=1)
            out[r], attn[r], attn0[r] = o.detach(), a.detach(), sm.detach()
            top = logit.detach().max(dim=1, keepdim=True).values
            lv = logit.detach() == top
            live[r] = lv
            gap = (top - logit.detach())[~lv]
            if gap.numel():
                facts.dead_gap = min(facts.dead_gap, float(gap.min()))
            al = (pre.detach() > 0)[lv]                                  # (live pairs of the chunk, A)
            facts.alive += al.sum(0)
            facts.dead += (~al).sum(0)
            if with_grad:
                loss = 0
                if g_out is not None:
                    loss = loss + (o * g_out[r]).sum()
                if g_attn is not None:
                    loss = loss + (a * g_attn[r]).sum()
                pre.retain_grad()
                logit.retain_grad()
                loss.backward()
                gx[r] = xs.grad
                facts.dl_bf16 &= _bf16_ok(logit.grad)
                facts.dh_bf16 &= _bf16_ok(pre.grad)
                facts.dl_max = max(facts.dl_max, float(logit.grad.abs().max()))
    return NS(out=out, attn=attn, attn0=attn0, gx=gx, gW1=ps[0].grad, gb1=ps[1].grad, gw2=ps[2].grad, gb2=ps[3].grad,
              live=live, facts=facts)


# ---------------------------------------------------------------------------------------------------------------------
# the operand makers
# ---------------------------------------------------------------------------------------------------------------------
def live_k(N):
    """the largest K the fields of a sample admit"""
    return 16 if N >= 9 else 4 if N >= 5 else 2 if N >= 4 else 1


def support_cols(E, kind):
    """the column set S (tag column 0 left out, an even number of columns) and its involution pi as a column permutation"""
    S = {"low": list(range(1, E // 2 + 1)), "odd": list(range(1, E, 2)), "high": list(range(E // 2, E))}[kind]
    S = S[:len(S) // 2 * 2]
    assert len(S) >= 2, (E, kind)
    h = len(S) // 2
    pi = torch.arange(E)
    pi[S[:h]], pi[S[h:]] = torch.tensor(S[h:]), torch.tensor(S[:h])
    return torch.tensor(S), pi


def grad_samples(B):
    """the samples that carry gradients: all up to 8; above that the first four, the last two and the samples either side
    of every multiple of a grid cap (block 0 takes sample ``cap`` as its second, the last block sample ``cap - 1``)"""
    if B <= 8:
        return list(range(B))
    want = {0, 1, 2, 3, B - 2, B - 1} | {c + d for c in (256, 512, 1024, 2048) for d in (-1, 0)}
    return sorted(b for b in want if 0 <= b < B)


def afm_weights(E, A, kind, g):
    S, pi = support_cols(E, kind)
    W1, b1, w2 = torch.zeros(A, E, dtype=F64), torch.zeros(A, dtype=F64), torch.zeros(A, dtype=F64)
    W1[0, 0], b1[0], w2[0] = -1.0, 1.0, -PENALTY
    units = (1 + torch.randperm(A - 1, generator=g)).tolist()         # twins are not neighbours
    rnd = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))      # noqa: E731
    while units:
        a = units.pop()
        bias, sign = float(rnd(-1, 1)), float(rnd(0, 1) * 2 - 1)
        twin = units.pop() if units else None                         # the odd one out is its own twin: pi-symmetric
        half = twin is None
        k = min(rnd(1, 2), len(S) // 2) if half else min(rnd(2, 4), len(S))
        pool = S[:len(S) // 2] if half else S
        cols = pool[torch.randperm(len(pool), generator=g)[:k]]
        while True:       # alive under exactly one of the patterns ONES (b1 + sum of the row) and ZERO (b1): see afm_operands
            sg = (torch.randint(0, 2, (k,), generator=g) * 2 - 1).to(F64)
            if (bias + float(sg.sum()) * (2 if half else 1) > 0) != (bias > 0):
                break
            bias = float(rnd(-1, 1))
        W1[a, cols], W1[a if half else twin, pi[cols]] = sg, sg
        if not half:
            b1[twin], w2[twin] = bias, sign
        b1[a], w2[a] = bias, sign
    return W1, b1, w2, torch.ones(1, dtype=F64), S, pi


def afm_operands(N, E, A, B, kind="low", drop=0, mode="both", slot=False, salt=0):
    """``drop``: score dropout in percent (0, 50, 75).  ``mode``: 'both' gradients, 'out' (g_attn absent), 'attn' (g_out
    absent).  ``slot``: B = P samples with K = 1, sample p live on pair p only."""
    g = gen(41, N, E, A, B, {"low": 0, "odd": 1, "high": 2}[kind], drop, {"both": 0, "out": 1, "attn": 2}[mode], slot, salt)
    I, J = pair_index(N)
    P = I.numel()
    K = 1 if slot else live_k(N)
    assert not slot or B == P
    npos, nneg = LIVE_FIELDS[K]
    W1, b1, w2, b2, S, pi = afm_weights(E, A, kind, g)
    x = torch.randint(-1, 2, (B, N, E), generator=g).to(F64)
    tag = torch.zeros(B, N, dtype=F64)
    for b in range(B):
        order = torch.tensor([int(I[b]), int(J[b])]) if slot else torch.randperm(N, generator=g)
        if not slot and b < 5 and N - b > 0:                           # the first field and the last four are live somewhere
            f = (N - 1, 0, N - 2, N - 3, N - 4)[b] % N
            at = int((order == f).nonzero())
            order[at], order[0] = order[0].clone(), f
        pos, neg = order[:npos], order[npos:npos + nneg]
        tag[b, pos], tag[b, neg] = 1.0, -1.0
        pat = torch.randint(0, 2, (E,), generator=g).to(F64)
        if not slot and b < 2:                                         # ONES, ZERO: every unit is alive under one, dead under the other
            pat = torch.full((E,), float(1 - b), dtype=F64)
        if not slot and b == 2:       # HALF: the "+" pairs have ones on the first half of S, the "-" pairs on the second, so
            pat = torch.zeros(E, dtype=F64)                            # every column of S meets d(hidden) that does not cancel
            pat[S[:len(S) // 2]] = 1.0
        su = (torch.randint(0, 2, (2, E), generator=g) * 2 - 1).to(F64)
        u, v = pat * su[0], pat[pi] * su[1]
        for f in pos.tolist():
            x[b, f, S] = u[S]
        for f in neg.tolist():
            x[b, f, S] = v[S]
    x[:, :, 0] = tag
    live = (tag[:, I] * tag[:, J]) == 1.0                              # (B, P)
    assert bool((live.sum(1) == K).all())
    keep, scale = None, 1.0
    if drop:
        scale = {50: 2.0, 75: 4.0}[drop]
        keep = (torch.rand(B, P, generator=g) >= drop / 100.0)
    Mod = K // math.gcd(K, int(scale))                                 # sum over the kept live pairs of ds: 0 modulo this
    if keep is not None:
        for b in range(B):                                             # enough kept live pairs to adjust on
            idx = live[b].nonzero().flatten()
            short = Mod // 2 - int(keep[b, idx].sum())
            if short > 0:
                keep[b, idx[~keep[b, idx]][:short]] = True
    # slot cases: every sample carries gradients (nothing is summed over samples: K = 1 gives no parameter gradient); from
    # 1000 pairs on every 8th sample and the usual ones, to keep the float64 reference within a few seconds
    gs = grad_samples(B) if not slot else list(range(B)) if B <= 1000 else sorted(set(range(0, B, 8)) | set(grad_samples(B)))
    g_out = g_attn = None
    prod_live = lambda b, idx: x[b, I[idx]] * x[b, J[idx]]             # noqa: E731   (pairs, E)
    if mode in ("both", "out"):
        g_out = torch.zeros(B, E, dtype=F64)
    if mode in ("both", "attn"):
        g_attn = torch.zeros(B, P, dtype=F64)
    for b in gs:
        idx = live[b].nonzero().flatten()
        kept = idx if keep is None else idx[keep[b, idx]]
        pl = prod_live(b, kept)
        if mode == "out":
            for _ in range(2000):                                      # redraw until the kept live ds sum to 0 mod Mod
                cols = torch.randperm(E, generator=g)[:2]
                sg = (torch.randint(0, 2, (2,), generator=g) * 2 - 1).to(F64)
                d = (pl[:, cols] * sg).sum(1)
                if int(d.sum()) % Mod == 0 and (kept.numel() < 2 or float(d.max()) != float(d.min())):
                    break
            else:
                raise AssertionError(("no g_out row found", N, E, A, B, b))
            g_out[b, cols] = sg
            continue
        d = torch.zeros(kept.numel(), dtype=F64)
        if g_out is not None:
            cols = torch.randperm(E, generator=g)[:2]
            g_out[b, cols] = (torch.randint(0, 2, (2,), generator=g) * 2 - 1).to(F64)
            d = (pl * g_out[b]).sum(1)
        g_attn[b] = torch.randint(-1, 2, (P,), generator=g).to(F64)
        r = int((d + g_attn[b, kept]).sum()) % Mod
        n_adj, step = (r, -1.0) if r <= Mod // 2 else (Mod - r, 1.0)
        assert n_adj <= kept.numel()
        g_attn[b, kept[torch.randperm(kept.numel(), generator=g)[:n_adj]]] += step
    keep_u8 = None if keep is None else keep.to(torch.uint8)
    ref = afm_ref(x, W1, b1, w2, b2, g_out, g_attn, None if keep is None else keep.to(F64), scale)
    return NS(N=N, E=E, A=A, B=B, K=K, S=S, pi=pi, x=x, W1=W1, b1=b1, w2=w2, b2=b2, g_out=g_out, g_attn=g_attn,
              keep=keep_u8, keep_scale=scale, live=live, tag=tag, grad_samples=gs, ref=ref)


# ---------------------------------------------------------------------------------------------------------------------
# case lists.  A case is (dtype, N, E, A, B, S kind, dropout percent, gradient mode)
# ---------------------------------------------------------------------------------------------------------------------
_KINDS = ("low", "odd", "high")


def _kind(*key):
    return _KINDS[sum(key) % 3]


# every forward <A / 16, E / 32>; the backward on the matrix cores where admitted, generic elsewhere, refused at
# (112, 128) and (128, 128): the generic backward's LDS figure is asked of every shape and passes 160 KiB there
AFM_INST = [(BF16, 9, E, A, 5, _kind(A // 16, E // 32), 0, "both") for A in range(16, 129, 16) for E in (32, 64, 128)]
# the three tile schedules of the matrix-core backward at A = 32: N below four tiles, rounds, packed, TPR = 2, TPR = 3
AFM_SCHED_N = (2, 3, 4, 5, 16, 17, 31, 32, 33, 39, 48, 60, 61, 64, 65)
AFM_SCHED = ([(BF16, N, 32, 32, 5, _kind(N), 0, "both") for N in AFM_SCHED_N]
             + [(BF16, N, 64, 32, 5, _kind(N, 1), 0, "both") for N in (17, 39, 61)])
# (dtype, N, E, A): slot_case
AFM_SLOT = ([(BF16, N, 32, 32) for N in (2, 17, 33, 61)] + [(BF16, 64, 128, 32)] + [(F32, N, 8, 8) for N in (5, 41)])
# grid caps.  Backward matrix-core (256): N = 17 (wave 0 ends every sample on an odd tile count) and N = 39 (wave 3);
# forward matrix-core: 2049 samples > 256 CUs x 8 workgroups; generic (1024) in both dtypes
AFM_CAP_BWD = [(BF16, N, 32, 32, B, _kind(N, B), 0, "both") for N in (17, 39) for B in (256, 257, 513)]
AFM_CAP_FWD = [(BF16, 9, 32, 32, FWD_MFMA_GRID_MOST + 1, "odd", 0, "both")]
AFM_CAP_GENERIC = [(dt, 5, 8, 8, B, "low", 0, "both") for dt in (F32, BF16) for B in (GENERIC_GRID, GENERIC_GRID + 1)]
# the generic kernels: ES = 1 / 2, every AMAX bucket and its edges, E and A that are no multiple of 4, LDS past 64 KiB
# (bf16 reaches them only outside E in {32, 64, 128} or with A % 16 != 0: one list that is generic in both dtypes)
# (E = 128, A = 100 at N = 5: the backward's 161 844 bytes of LDS are within the entry's 160 KiB, N = 7 is 236 bytes past)
_GEN_SHAPES = [(2, 8, 1), (7, 8, 8), (7, 24, 33), (39, 24, 8), (7, 24, 64), (7, 64, 65), (39, 64, 100), (7, 100, 33),
               (2, 100, 65), (7, 100, 64), (5, 128, 100), (2, 100, 128), (7, 100, 32), (7, 128, 33), (7, 30, 33)]
AFM_GENERIC = ([(dt, N, E, A, 5, _KINDS[i % 3], 0, "both") for dt in (F32, BF16) for i, (N, E, A) in enumerate(_GEN_SHAPES)]
               + [(F32, 128, 8, 8, 3, "high", 0, "both")])           # both directions past 64 KiB: the attribute branch
UNALIGNED_CASE = (BF16, 39, 64, 64, 5, "high", 0, "both")            # x one element into its buffer
# score dropout (keep_scale 2 and 4) and one absent gradient, on both families
AFM_DROP = [(BF16, 39, 64, 64, 5, "low", 50, "both"), (BF16, 17, 32, 32, 5, "odd", 75, "both"),
            (F32, 12, 24, 33, 5, "high", 50, "both"), (BF16, 12, 24, 33, 5, "low", 75, "both")]
AFM_MODES = [(dt, N, E, A, 5, "odd", drop, mode) for (dt, N, E, A) in ((BF16, 39, 64, 64), (F32, 12, 24, 33))
             for (drop, mode) in ((0, "out"), (0, "attn"), (50, "out"))]
AFM_CASES = (AFM_INST + AFM_SCHED + AFM_CAP_BWD + AFM_CAP_FWD + AFM_CAP_GENERIC + AFM_GENERIC + [UNALIGNED_CASE]
             + AFM_DROP + AFM_MODES)
# what tests/test_gpu_pairx.py::test_afm_vs_oracle ran, (B, N, E, A), in both dtypes
OLD_TOLERANCE_SHAPES = [(37, 39, 64, 64), (5, 2, 16, 8), (130, 7, 24, 40), (9, 5, 128, 100), (1, 3, 8, 1), (64, 10, 32, 16),
                        (33, 12, 128, 32), (20, 39, 64, 128), (3, 2, 64, 48), (40, 9, 32, 64), (17, 6, 64, 96),
                        (9, 4, 32, 128), (300, 2, 64, 32), (70, 34, 64, 32)]


def case_id(c):
    return "-".join(dtype_tag(v) if isinstance(v, torch.dtype) else str(v) for v in c)


def covers(c):
    """the coverage conditions a case with parameter gradients (K >= 2) owes: every column of S has a nonzero dW1 entry, at
    least 15 % of dW1 is nonzero, db1 and dw2 are not zero throughout"""
    r = c.ref
    return c.K < 2 or (bool((r.gW1[:, c.S] != 0).any(0).all()) and float((r.gW1 != 0).double().mean()) >= 0.15
                       and (c.A == 1 or (bool((r.gb1 != 0).any()) and bool((r.gw2 != 0).any()))))


@functools.lru_cache(maxsize=2)
def afm_case(dtype, N, E, A, B, kind, drop, mode):
    """the operands do not depend on ``dtype``: both dtypes of a shape are held to the same float64 result.  A draw that
    misses a coverage condition is replaced by the next one (``salt``); the host test holds the result to all of them."""
    for salt in range(8):
        c = afm_operands(N, E, A, B, kind, drop, mode, salt=salt)
        if covers(c):
            break
    return c


@functools.lru_cache(maxsize=2)
def slot_case(N, E, A):
    """B = P samples, K = 1, sample p live on pair p only: attn is the identity, out[p] the product row of pair p, gx
    touches fields i_p and j_p alone -- a misplaced slot of any pair changes the result"""
    return afm_operands(N, E, A, N * (N - 1) // 2, _kind(N), 0, "both", slot=True)

"""Integer operands, float64 references and dispatch mirrors that make EVERY inner-product (IPN) kernel path of
csrc/pair.hip comparable BIT FOR BIT: the bf16 matrix-core kernels (pair_dot_fwd_mfma_kernel, its gather-fused form behind
trs_embed_pair_dot, pair_dot_bwd_mfma_kernel), the fp32-staging LDS-tile kernels (pair_dot_fwd_kernel / pair_dot_bwd_kernel)
and the generic kernels.

The operation is purely bilinear.  With x and gout in {-1, 0, 1} every forward value x_i . x_j is an integer of magnitude at
most E <= 128 and every backward value (Gs x)[i, e] an integer of at most N - 1 <= 64: exact in bf16 and in fp32 in any
order of summation, so a correct kernel of any family returns ``expect(ref, dtype)`` and a missing, doubled or misplaced
term changes it.  The table gradient of the gather-fused entry sums dx + ge (|v| <= 64) over the lookups of a row; the ids
of ``embed_case`` hit every row at most four times, so that sum stays within 256.

``ipn_path`` / ``tile_fwd_lds`` / ``tile_bwd_lds`` / ``bwd_mfma_lds`` restate the dispatch arithmetic of pair.hip; the case
lists are DERIVED from them, and tests/test_exact_ipn_host.py pins each restated line to the source text (one match per
site).  tests/test_gpu_exact_ipn.py runs exactly these lists.  Nothing here imports torecsys_amd."""
import functools
import os
import re
from types import SimpleNamespace as NS

import torch

from exact_ref import CSRC, F64, assert_exact_domain, expect, gen, ints, mismatch, pair_index      # noqa: F401 (re-exported)

BF16, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def sym(gout, N):
    """Gs (B, N, N): the symmetric zero-diagonal matrix of the pair gradients gout (B, P)"""
    I, J = pair_index(N)
    Gs = torch.zeros(gout.shape[0], N, N, dtype=gout.dtype)
    Gs[:, I, J] = gout
    Gs[:, J, I] = gout
    return Gs


def ipn_ref(x, gout):
    """x (B, N, E), gout (B, P) -> (out (B, P), dx (B, N, E)): out[b, p] = x[b, i_p] . x[b, j_p] with the pairs in the
    row-major order of torch.triu_indices(N, N, 1); dx = Gs x"""
    B, N, E = x.shape
    I, J = pair_index(N)
    out = torch.bmm(x, x.transpose(1, 2))[:, I, J]
    return out, torch.bmm(sym(gout, N), x)


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch arithmetic of csrc/pair.hip, one line per site
# ---------------------------------------------------------------------------------------------------------------------
LDS_BUDGET = 80 * 1024                  # the tile kernels' budget per block
WAVES_MAX = 4 * 256 * 8                 # four waves per block, grid capped at 256 * 8 blocks: one sample per wave up to here
GENERIC_ITEMS_MAX = 256 * 8192          # generic kernels: stream_grid(items, 256, 8192) threads, one item each up to here


def grid(B):
    return min((B + 3) // 4, 256 * 8)


def mfma_ok(N, E):
    return 2 <= N <= 64 and E in (32, 64, 128)


def tile_fwd_lds(N, E):
    TN = (N + 3) // 4; NP = TN * 4; ES = E + 4; P = N * (N - 1) // 2
    return ((TN * (TN + 1) // 2 * 4 + 15) & ~15) + 4 * (NP * ES + ((P + 3) & ~3)) * 4


def tile_bwd_lds(N, E):
    TN = (N + 3) // 4; NP = TN * 4; ES = E + 4; GS = NP + 4
    return 4 * (NP * ES + NP * GS) * 4


def bwd_mfma_lds(N, E):
    NT = (N + 15) // 16; NP = 16 * NT; NPK = 32 * ((NP + 31) // 32); P = N * (N - 1) // 2
    return ((P + 7) & ~7) * 2 + 4 * (NP * (NPK + 8) + E * (NPK + 8)) * 2


def ipn_path(dtype, N, E, aligned=True):
    """which kernel family trs_pair_dot_fwd / trs_pair_dot_bwd launch: ``fwd`` / ``bwd`` in {'mfma', 'tile', 'generic'};
    NT, KS (forward), KE (backward) are the template arguments of the matrix-core instantiation, None elsewhere"""
    assert N >= 2
    if dtype == BF16 and mfma_ok(N, E) and aligned:
        return NS(fwd="mfma", bwd="mfma", NT=(N + 15) // 16, KS=E // 32, KE=E // 16)
    return NS(fwd="tile" if E % 4 == 0 and tile_fwd_lds(N, E) <= LDS_BUDGET else "generic",
              bwd="tile" if E % 4 == 0 and tile_bwd_lds(N, E) <= LDS_BUDGET else "generic", NT=None, KS=None, KE=None)


def tile_max_n(lds_of, E):
    """the largest N the tile kernel of one direction takes at this E"""
    N = 2
    while lds_of(N + 1, E) <= LDS_BUDGET:
        N += 1
    assert lds_of(N, E) <= LDS_BUDGET
    return N


# source text each mirror above restates: (function the line stands in, the line).  The head of a function is the text
# from its name to the first "\n}\n" behind it.
_HEADS = {
    "mfma_ok": "static bool pair_mfma_ok(",
    "fwd_mfma": "static int pair_dot_fwd_mfma(",
    "embed_mfma": "static int embed_pair_dot_mfma(",
    "bwd_mfma": "static int pair_dot_bwd_mfma(",
    "fwd_launch": "static int pair_dot_fwd_launch(",
    "bwd_launch": "static int pair_dot_bwd_launch(",
    "trs_fwd": 'extern "C" int trs_pair_dot_fwd(',
    "trs_bwd": 'extern "C" int trs_pair_dot_bwd(',
    "trs_embed": 'extern "C" int trs_embed_pair_dot(',
    "fwd_mfma_kernel": "void pair_dot_fwd_mfma_kernel(",
    "bwd_mfma_kernel": "void pair_dot_bwd_mfma_kernel(",
    "fwd_kernel": "void pair_dot_fwd_kernel(",
    "bwd_kernel": "void pair_dot_bwd_kernel(",
}
_GRID = "const int grid = (int)std::min<int64_t>((B + 3) / 4, 256 * 8);"
_SITES = [
    ("mfma_ok", "return N >= 2 && N <= 64 && (E == 32 || E == 64 || E == 128);"),
    ("fwd_mfma", "const int NT = (N + 15) / 16, KS = E / 32;"), ("fwd_mfma", _GRID),
    ("fwd_mfma", "const size_t lds_f = (size_t)4 * (((N * (N - 1) / 2) + 7) & ~7) * 2;"),
    ("embed_mfma", "const int NT = (N + 15) / 16, KS = E / 32;"), ("embed_mfma", _GRID),
    ("embed_mfma", "const size_t lds_f = (size_t)4 * (((N * (N - 1) / 2) + 7) & ~7) * 2;"),
    ("bwd_mfma", "const int NT = (N + 15) / 16, KE = E / 16;"), ("bwd_mfma", _GRID),
    ("bwd_mfma", "const int NP = 16 * NT, NPK = 32 * ((NP + 31) / 32);"),
    ("bwd_mfma", "const size_t lds = (size_t)((P + 7) & ~7) * 2 + (size_t)4 * (NP * (NPK + 8) + E * (NPK + 8)) * 2;"),
    ("fwd_launch", "const int TN = (N + 3) / 4, NP = TN * 4, ES = E + 4, P = N * (N - 1) / 2;"),
    ("fwd_launch", "const size_t lds = (size_t)((TN * (TN + 1) / 2 * 4 + 15) & ~15) + 4 * (size_t)(NP * ES + ((P + 3) & ~3)) * 4;"),
    ("fwd_launch", "if (E % 4 == 0 && lds <= LDS_BUDGET && N >= 2) {"), ("fwd_launch", _GRID),
    ("fwd_launch", "dim3(stream_grid(B * P, 256, 8192))"),
    ("bwd_launch", "const int TN = (N + 3) / 4, NP = TN * 4, ES = E + 4, GS = NP + 4;"),
    ("bwd_launch", "const size_t lds = 4 * (size_t)(NP * ES + NP * GS) * 4;"),
    ("bwd_launch", "if (E % 4 == 0 && lds <= LDS_BUDGET && N >= 2) {"), ("bwd_launch", _GRID),
    ("bwd_launch", "dim3(stream_grid(B * N * E, 256, 8192))"),
    ("trs_fwd", "if (dtype == TRS_F32) return pair_dot_fwd_launch<float>(x, out, B, N, E, (hipStream_t)stream);"),
    ("trs_fwd", "if (pair_mfma_ok(N, E) && aligned16(x)) return pair_dot_fwd_mfma(x, out, B, N, E, (hipStream_t)stream);"),
    ("trs_bwd", "if (dtype == TRS_F32) return pair_dot_bwd_launch<float>(x, g, dx, B, N, E, (hipStream_t)stream);"),
    ("trs_bwd", "if (pair_mfma_ok(N, E) && aligned16(x)) return pair_dot_bwd_mfma(x, g, dx, B, N, E, (hipStream_t)stream);"),
    ("trs_embed", "if (dtype != TRS_BF16 || !pair_mfma_ok(N, E) || N < 2 || !aligned16(table) || !aligned16(emb))"),
    ("fwd_mfma_kernel", "for (int64_t b = wid; b < B; b += nwaves) {"),
    ("bwd_mfma_kernel", "for (int64_t b = wid; b < B; b += nwaves) {"),
    ("bwd_mfma_kernel", "const int64_t bn = b + nwaves < B ? b + nwaves : b;"),
    ("bwd_mfma_kernel", "for (int j = i + 1; j < N; ++j) lut[base + (j - i - 1)] = (unsigned short)((i << 8) | j);"),
    ("fwd_kernel", "const int TN = (N + 3) >> 2, NP = TN * 4, ES = E + 4;"),
    ("fwd_kernel", "for (int q = lane; q < ntiles; q += 64) {"),
    ("bwd_kernel", "const int TN = (N + 3) >> 2, NP = TN * 4, ES = E + 4, GS = NP + 4;"),
]


def source_sites():
    """[(function, line, matches of the line inside the function)]: the host test wants exactly one each"""
    with open(os.path.join(CSRC, "pair.hip")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "trs_common.hpp")) as f:
        common = f.read()
    out = []
    for fn, line in _SITES:
        heads = re.findall(re.escape(_HEADS[fn]), src)
        assert len(heads) == 1, (fn, heads)
        s = src.index(_HEADS[fn])
        out.append((fn, line, len(re.findall(re.escape(line), src[s:src.index("\n}\n", s)]))))
    out.append(("LDS_BUDGET", "", len(re.findall(r"constexpr size_t LDS_BUDGET = 80 \* 1024;", src))))
    out.append(("pair_index", "", len(re.findall(
        r"int pair_index\(int i, int j, int N\) \{\s*//[^\n]*\n\s*return i \* N - \(i \* \(i \+ 1\)\) / 2 \+ \(j - i - 1\);", src))))
    out.append(("stream_grid", "", len(re.findall(
        r"if \(g > max_blocks\) g = max_blocks;", common))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------------------------------
# (N, E, B), bf16: every NT x KS / KE instantiation with N one below, on and one above each 16-field tile edge; five
# samples: one block and one wave of a second
IPN_MFMA_N = [(N, E, 5) for N in (2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64) for E in (32, 64, 128)]
# (N, E, B), bf16: the grid cap; WAVES_MAX + 1: wave 0 takes a second sample (the backward's prefetch chain hands over a
# DIFFERENT sample, then clamps on the last one); 2 * WAVES_MAX + 1: a third (two hand-overs, then the clamp)
IPN_MFMA_B = [(N, E, B) for (N, E) in ((17, 32), (33, 64))
              for B in (1, 3, 4, WAVES_MAX - 1, WAVES_MAX, WAVES_MAX + 1, 2 * WAVES_MAX + 1)]
# (dtype, N, E): slot_case, one sample per pair
IPN_SLOT = ([(BF16, N, 32) for N in (2, 17, 33, 49, 64)] + [(F32, N, 8) for N in (5, 41)] + [(BF16, 64, 128)])
# (dtype, N, E, B): the LDS-tile kernels; N around the 4-field register tile, and N >= 41: TN (TN + 1) / 2 > 64 tiles, a
# lane of the forward takes a second one
IPN_TILE = ([(F32, N, E, 6) for E in (4, 16, 64) for N in (2, 3, 4, 5, 7, 8, 9, 40, 41, 44, 45)]
            + [(BF16, N, E, 6) for E in (16, 96) for N in (2, 3, 4, 5, 7, 8, 9, 40, 41, 44, 45)])
# (dtype, N, E, B): the largest N each direction's tile kernel takes and that N + 1 (generic), from the mirrors
IPN_BUDGET = [(dt, N, E, 6) for (dt, E) in ((F32, 64), (F32, 128), (BF16, 96))
              for N in sorted({tile_max_n(f, E) + d for f in (tile_fwd_lds, tile_bwd_lds) for d in (0, 1)})]
# (dtype, N, E, B): the generic kernels proper.  300 samples: more than one block of 256 threads in either direction at
# every N; (65, 64) with 1009 samples: more items than GENERIC_ITEMS_MAX threads in BOTH directions (1009 * 2080 pairs),
# so a thread walks on to a second item
IPN_GENERIC = ([(dt, N, E, 300) for dt in (F32, BF16) for E in (1, 3, 10) for N in (2, 5, 39)] + [(BF16, 65, 64, 1009)])
# (N, E, B, index dtype): the gather-fused entry
IPN_EMBED = ([(N, E, 5, it) for N in (2, 16, 17, 39, 48, 49, 64) for E in (32, 64, 128) for it in (torch.int32, torch.int64)]
             + [(17, 32, WAVES_MAX + 1, it) for it in (torch.int32, torch.int64)])
# the backward's dynamic LDS grows with N inside an (NT, KE) instantiation: (E, ascending Ns of one instantiation)
IPN_LDS_BUCKETS = [(64, (33, 39, 48)), (64, (49, 64)), (128, (33, 48)), (128, (49, 64))]
UNALIGNED_CASE = (39, 64, 5)             # bf16, x one element into its buffer: the matrix-core path hands over to the tiles


def dtype_tag(v):
    return {BF16: "bf16", F32: "fp32", torch.int32: "i32", torch.int64: "i64"}.get(v, str(v))


@functools.lru_cache(maxsize=2)
def ipn_case(N, E, B):
    g = gen(21, N, E, B)
    x, gout = ints((B, N, E), g), ints((B, N * (N - 1) // 2), g)
    out, dx = ipn_ref(x, gout)
    return NS(x=x, gout=gout, out=out, dx=dx)


@functools.lru_cache(maxsize=2)
def slot_case(N, E):
    """B = P samples; sample p has exactly two live fields, i_p and j_p, both holding v_p in {-1, 1}^E, and gout[p] is
    one-hot at slot p with a random sign s_p: out = E * I_P, dx[p, i_p] = dx[p, j_p] = s_p v_p and zero elsewhere -- a
    misplaced slot of any pair, in the forward's pair_index or the backward's lut, changes the result"""
    g = gen(22, N, E)
    P = N * (N - 1) // 2
    I, J = pair_index(N)
    p = torch.arange(P)
    v = (torch.randint(0, 2, (P, E), generator=g) * 2 - 1).to(F64)
    s = (torch.randint(0, 2, (P,), generator=g) * 2 - 1).to(F64)
    x = torch.zeros(P, N, E, dtype=F64)
    x[p, I] = v
    x[p, J] = v
    gout = torch.zeros(P, P, dtype=F64)
    gout[p, p] = s
    out, dx = ipn_ref(x, gout)
    return NS(x=x, gout=gout, out=out, dx=dx, v=v, s=s, I=I, J=J)


def embed_ref(table, rid, valid, ge, gp):
    """the lookup (an invalid id reads as a zero row and receives no gradient), ipn_ref on the block, and the table
    gradient: index_add_ of dx + ge over the valid lookups"""
    B, N = rid.shape
    V, E = table.shape
    safe = torch.where(valid, rid, torch.zeros_like(rid))
    emb = table[safe] * valid.unsqueeze(-1).to(F64)
    out, dx = ipn_ref(emb, gp)
    rows = (dx + ge) * valid.unsqueeze(-1).to(F64)
    gtab = torch.zeros(V, E, dtype=F64).index_add_(0, safe.reshape(-1), rows.reshape(B * N, E))
    terms = torch.zeros(V, E, dtype=F64).index_add_(0, safe.reshape(-1), (rows.abs()).reshape(B * N, E))
    return NS(emb=emb, out=out, dx=dx, rows=rows, gtab=gtab, terms=terms)


@functools.lru_cache(maxsize=2)
def embed_case(N, E, B, idx_dtype):
    """one table of ``ints`` rows for N fields of sizes ceil(B / 2) + 1 + (n % 3); the ids of a field are drawn without
    replacement from four copies of its id range, so every table row is looked up at most FOUR times over the whole batch
    (and some never); ge (B, N, E) and gp (B, P) in {-1, 0, 1}.  ``oob``: the same with the id at (0, N // 2) replaced by
    one that lands behind the table."""
    g = gen(23, N, E, B)
    sizes = [(B + 1) // 2 + 1 + (n % 3) for n in range(N)]
    offsets = torch.tensor([0] + sizes[:-1]).cumsum(0)
    V = sum(sizes)
    table = ints((V, E), g)
    idx = torch.stack([torch.arange(s).repeat(4)[torch.randperm(4 * s, generator=g)[:B]] for s in sizes], 1)
    ge, gp = ints((B, N, E), g), ints((B, N * (N - 1) // 2), g)
    rid = idx + offsets
    lookups = torch.zeros(V, dtype=torch.int64).index_add_(0, rid.reshape(-1), torch.ones(B * N, dtype=torch.int64))
    assert int(lookups.max()) <= 4
    bad = idx.clone()
    bad[0, N // 2] = V                                       # + offsets[N // 2] >= V whatever the field
    ok = torch.ones(B, N, dtype=torch.bool)
    ok[0, N // 2] = False
    return NS(table=table, sizes=sizes, offsets=offsets, V=V, idx=idx.to(idx_dtype), bad=bad.to(idx_dtype), ge=ge, gp=gp,
              lookups=lookups, ref=embed_ref(table, rid, torch.ones(B, N, dtype=torch.bool), ge, gp),
              oob=embed_ref(table, rid, ok, ge, gp))

"""Test helpers for the row-bucket (CSR) build and the bucket walk of csrc/scatter.hip -- not product code.

* ``bucket_ladder``: an index matrix in which chosen rows of every field receive EXACTLY a prescribed number of lookups
  (the lengths at which the walk changes kernel) and no other row receives more than one.
* ``integer_case``: table values and gradients drawn from {-2, ..., 2}.  Every term and every partial sum of the walk is
  then an integer far below 2**24, so the kernels' fp32 accumulators hold the TRUE sum whatever the order and the only
  rounding is the final store: the expected result is the float64 reference rounded once, compared with torch.equal.
* float64 references that take the flat lookups: plain / FM-folded / E = 1 companion gradient, SGD, Adagrad, lazy Adam,
  and the per-element rounding bounds of the last two (derivation: tests/test_gpu_scatter_boundaries.py).
* ``check_csr``: the exact (integer) restatement of a row-bucket index.
"""
import math
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCATTER_HIP = os.path.join(ROOT, "torecsys_amd", "csrc", "scatter.hip")

# One ladder for both paths.  Vector path: > 64 lookups -> queue of whole waves, > 256 -> chunks of 256 (2304 / 2305 =
# 9 / 10 chunks, 4096 / 4097 = 16 / 17: the finish kernel adds partials eight at a time).  Element path: > 32 -> queue,
# > 2048 -> chunks of 2048 over several waves (4097 = 3 chunks).  tests/test_scatter_ref_host.py holds these numbers
# against the constants in the source.
LADDER = (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 2304,
          2305, 4096, 4097)
LADDER_FIELDS = 3
VALUE_RANGE = 2                # tables and gradients are drawn from {-VALUE_RANGE, ..., VALUE_RANGE}
U32 = 2.0 ** -24               # one fp32 rounding, relative to the result (round to nearest)


def bucket_ladder(lengths, N, seed, singles=999, spare=500):
    """(field_sizes, idx): idx is (B, N) int64 with B = sum(lengths) + singles.  In every field one row per entry of
    ``lengths`` receives exactly that many lookups, ``singles`` further rows receive one each and ``spare + n`` rows none;
    which row plays which part is drawn per field (so every field assigns the lengths to different rows, and the field
    sizes differ), and the sample order is permuted per field, so chunk edges do not coincide with the batch order.  The
    field sizes do not depend on the seed: ladders of different seeds index the same table."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(list(lengths), dtype=torch.int64)
    R = lens.numel()
    B = int(lens.sum()) + singles
    field_sizes, cols = [], []
    for n in range(N):
        size = R + singles + spare + n
        rows = torch.randperm(size, generator=g)
        planned = rows[:R][torch.randperm(R, generator=g)]
        col = torch.cat([torch.repeat_interleave(planned, lens), rows[R:R + singles]])
        cols.append(col[torch.randperm(B, generator=g)])
        field_sizes.append(size)
    return field_sizes, torch.stack(cols, 1).contiguous()


def field_offsets(field_sizes):
    sizes = torch.tensor(list(field_sizes), dtype=torch.int64)
    return torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)[:-1]])


def flat_rows(field_sizes, idx):
    """table row of every lookup, (B*N,) int64 in (sample, field) order -- the 'flat lookups' the references take"""
    return (idx.long() + field_offsets(field_sizes).view(1, -1)).reshape(-1)


def row_of_length(field_sizes, idx, field, length):
    """table row of ``field`` that receives exactly ``length`` lookups (must be unique)"""
    counts = torch.bincount(idx[:, field], minlength=field_sizes[field])
    hit = (counts == length).nonzero().flatten()
    assert hit.numel() == 1, (field, length, hit.numel())
    return int(field_offsets(field_sizes)[field]) + int(hit[0])


def integer_case(field_sizes, idx, E, seed):
    """Integer-valued operands for the ladder, as int8 (exact in fp32, bf16 and float64): table ``w`` (V,E), companion
    table ``w1`` (V,1), embedding gradient ``ge`` (B,N,E), per-sample gradient row ``gs`` (B,1,E), FM gradients ``gf``
    (B,E) and ``gf1`` (B,1), companion gradient ``g1`` (B,N,1)."""
    g = torch.Generator().manual_seed(seed)
    B, N = idx.shape
    V = sum(field_sizes)

    def draw(*shape):
        return torch.randint(-VALUE_RANGE, VALUE_RANGE + 1, shape, generator=g, dtype=torch.int8)
    return {"w": draw(V, E), "w1": draw(V, 1), "ge": draw(B, N, E), "gs": draw(B, 1, E), "gf": draw(B, E),
            "gf1": draw(B, 1), "g1": draw(B, N, 1)}


# ---- float64 references over the flat lookups -----------------------------------------------------------------------
def scatter_sum(rows, V, terms):
    """out[r] = sum of terms[p] over the lookups p with rows[p] == r; terms (B*N, E) float64.  Lookups whose row is
    outside [0, V) contribute nothing."""
    terms = terms.double()
    ok = (rows >= 0) & (rows < V)
    out = torch.zeros(V, terms.shape[1], dtype=torch.float64)
    return out.index_add_(0, rows[ok], terms[ok])


def plain_terms(g, B, N):
    """per-lookup terms of the plain gradient: g is (B,N,E), or (B,1,E) = one row per sample shared by its fields"""
    g = g.double()
    return g.expand(B, N, g.shape[-1]).reshape(B * N, -1)


def fm_sum(rows, N, w):
    """S[b] = sum over the fields of the looked-up rows, (B,E) float64"""
    w = w.double()
    return w[rows].reshape(-1, N, w.shape[1]).sum(1)


def fm_terms(rows, N, w, g_fm):
    """per-lookup terms of the FM-folded gradient  g_fm[b] * (S[b] - w[r]);  g_fm is (B,E) or (B,1)"""
    w = w.double()
    S = fm_sum(rows, N, w)
    B, E = S.shape
    g = g_fm.double().expand(B, E)
    return (g.unsqueeze(1) * (S.unsqueeze(1) - w[rows].reshape(B, N, E))).reshape(B * N, E)


def fm_terms_abs(rows, N, w, g_fm):
    """what the walk actually adds per lookup, in magnitude: |g*S| (the staged [g*S | g] rows) and |w[r]| * |g| (the
    folded  - w[r] * sum g)"""
    w = w.double()
    S = fm_sum(rows, N, w)
    B, E = S.shape
    g = g_fm.double().expand(B, E).abs()
    return (g.unsqueeze(1) * (S.abs().unsqueeze(1) + w[rows].reshape(B, N, E).abs())).reshape(B * N, E)


def grad_plain(rows, V, g, B, N):
    return scatter_sum(rows, V, plain_terms(g, B, N))


def grad_fm(rows, V, N, w, g_fm):
    return scatter_sum(rows, V, fm_terms(rows, N, w, g_fm))


def grad_first(rows, V, g1):
    """gradient of the E = 1 companion table: g1 holds one value per lookup, (B,N,1) -> (V,1)"""
    return scatter_sum(rows, V, g1.double().reshape(-1, 1))


def touched_rows(rows, V, padding_row=-1):
    """(V,) bool: rows with at least one lookup -- the rows a fused optimizer step changes (whatever their gradient)"""
    ok = (rows >= 0) & (rows < V)
    t = torch.bincount(rows[ok], minlength=V) > 0
    if padding_row >= 0:
        t[padding_row] = False
    return t


def assert_exact_regime(terms_abs_sum, staged, dtype):
    """The conditions under which the kernels' sums are exact, asserted on the CPU reference: every element's
    sum_i |term_i| stays below 2**24 (so every partial sum, in any order, is an integer fp32 holds exactly), and every
    value staged in the table dtype (g*S, and the operands themselves) is representable in it."""
    assert float(terms_abs_sum.max()) < 2 ** 24, float(terms_abs_sum.max())
    assert torch.equal(terms_abs_sum, terms_abs_sum.round())
    for t in staged:
        t = t.double()
        assert torch.equal(t, t.round())
        assert torch.equal(t.to(dtype).double(), t), "a staged value is not representable in the table dtype"


def rounded(ref64, dtype):
    """the float64 reference as a kernel with an exact fp32 accumulator stores it: to fp32 (exact here), then one
    round-to-nearest-even to the table dtype"""
    return ref64.to(torch.float32).to(dtype)


def as_f32(x):
    """a host scalar as the kernel receives it (passed as a C float)"""
    return float(torch.tensor(x, dtype=torch.float32))


def sgd_step(w, G, touched, lr):
    w = w.double()
    return torch.where(touched.view(-1, 1), w - lr * G, w)


def adagrad_step(w, s, G, touched, lr, eps):
    """torch.optim.Adagrad without decay on the touched rows: s += G^2;  w -= lr * G / (sqrt(s) + eps).
    Returns (w', s', tol_w, tol_s): the tolerances are the rounding bounds of ONE fp32 step from (w, s)."""
    w, s, t = w.double(), s.double(), touched.view(-1, 1)
    s2 = s + G * G
    den = s2.sqrt() + eps
    d = lr * G / den
    w2 = w - d
    tol_s = 2 * U32 * torch.maximum(s2, G * G)
    tol_w = 5 * U32 * torch.maximum(torch.maximum(w.abs(), d.abs()), w2.abs())
    z = torch.zeros_like(w)
    return torch.where(t, w2, w), torch.where(t, s2, s), torch.where(t, tol_w, z), torch.where(t, tol_s, z)


def adam_step_size(lr, betas, t):
    """optim.FusedSparseAdam.next_step_size: lr * sqrt(1 - beta2^t) / (1 - beta1^t), handed to the kernel as fp32"""
    return as_f32(lr * (1.0 - betas[1] ** t) ** 0.5 / (1.0 - betas[0] ** t))


def lazy_adam_step(w, m, v, G, touched, step_size, betas, eps):
    """torch.optim.SparseAdam on the touched rows: m += (G - m)(1 - b1);  v += (G^2 - v)(1 - b2);
    w -= step_size * m / (sqrt(v) + eps).  Rows nobody looked up keep weight AND moments.
    Returns (w', m', v', tol_w, tol_m, tol_v), tolerances as in adagrad_step."""
    w, m, v, t = w.double(), m.double(), v.double(), touched.view(-1, 1)
    b1, b2 = betas
    m2 = m + (G - m) * (1.0 - b1)
    v2 = v + (G * G - v) * (1.0 - b2)
    den = v2.sqrt() + eps
    d = step_size * m2 / den
    w2 = w - d
    tol_m = 2 * U32 * torch.maximum(torch.maximum(m.abs(), G.abs()), m2.abs())
    tol_v = 2 * U32 * torch.maximum(torch.maximum(v, G * G), v2)
    tol_w = 5 * U32 * torch.maximum(torch.maximum(w.abs(), d.abs()), w2.abs())
    z = torch.zeros_like(w)
    return (torch.where(t, w2, w), torch.where(t, m2, m), torch.where(t, v2, v), torch.where(t, tol_w, z),
            torch.where(t, tol_m, z), torch.where(t, tol_v, z))


def bf16_half_ulp(value):
    """half a bf16 unit in the last place (8 significand bits) of ``value``, per element"""
    mag = value.double().abs()
    _, e = torch.frexp(mag.clamp_min(2.0 ** -126))           # mag = f * 2^e, f in [0.5, 1): ulp = 2^(e - 8)
    return torch.ldexp(torch.ones_like(mag), e - 9)


# ---- the row-bucket index ---------------------------------------------------------------------------------------------
def _check_csr(rb, rows_flat, V):
    """row_start = exclusive prefix sum of the per-row lookup counts; perm lists, row by row, exactly the flat
    lookup positions that hit the row (any order inside a row)."""
    valid = (rows_flat >= 0) & (rows_flat < V)
    counts = torch.bincount(rows_flat[valid], minlength=V)
    expect_start = torch.zeros(V + 1, dtype=torch.int64, device=rows_flat.device)
    expect_start[1:] = counts.cumsum(0)
    assert torch.equal(rb.row_start.long(), expect_start)
    total = int(expect_start[-1])
    perm = rb.perm[:total].long()
    assert torch.equal(perm.sort().values, valid.nonzero().flatten())       # a permutation of the valid lookups
    got_rows = rows_flat[perm]
    assert torch.equal(got_rows, got_rows.sort().values)                    # grouped by destination row
    assert torch.equal(torch.bincount(got_rows, minlength=V), counts)


# ---- the constants the ladder and the CSR seams were built around -----------------------------------------------------
def source_constants(path=SCATTER_HIP):
    """the thresholds of csrc/scatter.hip, read from the source text: {name: int}"""
    with open(path) as f:
        src = f.read()
    out = {}
    for name in ("SCAN_THREADS", "SCAN_ITEMS", "LONG_ROW", "LONG_ROW_ELEM", "LONG_CHUNK", "ELEM_SPLIT", "CSR2_CHUNK",
                 "CSR2_TINY", "CSR2_STAGE", "CSR2_MAX_FIELDS"):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m, f"constexpr int {name} not found in scatter.hip"
        out[name] = int(m.group(1))
    assert re.search(r"constexpr\s+int\s+SCAN_TILE\s*=\s*SCAN_THREADS\s*\*\s*SCAN_ITEMS\s*;", src)
    out["SCAN_TILE"] = out["SCAN_THREADS"] * out["SCAN_ITEMS"]
    m = re.search(r"const bool onepass = \(n \+ SCAN_TILE - 1\) / SCAN_TILE <= (\d+)", src)
    assert m, "the one-pass scan's tile cap not found in scatter.hip"
    out["ONEPASS_TILES"] = int(m.group(1))
    m = re.search(r"const bool part = offsets != nullptr && N <= CSR2_MAX_FIELDS && B >= (\d+) && "
                  r"max_items <= (\d+) \* \(int64_t\)N \+ (\d+) &&\s*max_items <= (\d+) && skip_row < 0;", src)
    assert m, "the partitioned build's gate not found in scatter.hip"
    out["PART_MIN_B"], out["PART_PER_FIELD"], out["PART_BASE"], out["PART_MAX_ITEMS"] = (int(x) for x in m.groups())
    # the chunk size and the item estimate, which csr_chunk() below restates
    m = re.search(r"const int64_t target = std::max<int64_t>\((\d+), (\d+) \* \(int64_t\)N\);", src)
    assert m, "the partitioned build's workgroup target not found in scatter.hip"
    out["CHUNK_TARGET"], out["CHUNK_TARGET_PER_FIELD"] = int(m.group(1)), int(m.group(2))
    assert "int64_t chunk = (V + (target - N) - 1) / std::max<int64_t>(1, target - N);" in src
    m = re.search(r"chunk = std::min<int64_t>\(CSR2_CHUNK, std::max<int64_t>\((\d+), \(chunk \+ (\d+)\) / (\d+) \* (\d+)\)\);",
                  src)
    assert m, "the partitioned build's chunk rounding not found in scatter.hip"
    out["CHUNK_MIN"], out["CHUNK_ROUND"] = int(m.group(1)), int(m.group(3))
    assert int(m.group(2)) == out["CHUNK_ROUND"] - 1 and int(m.group(4)) == out["CHUNK_ROUND"]
    assert "const int64_t max_items = (int64_t)N + (V + chunk - 1) / chunk;" in src
    return out


def csr_chunk(V, N, chunk_max=15360):
    """csr_build_impl's chunk size and its upper estimate of the (field, chunk) work items, restated"""
    target = max(256, 4 * N)
    chunk = (V + (target - N) - 1) // max(1, target - N)
    chunk = min(chunk_max, max(1024, (chunk + 255) // 256 * 256))
    return chunk, N + (V + chunk - 1) // chunk


def partitioned(V, N, B, skip_row=None):
    """does csr_build_impl take the partitioned (LDS-counter) build for this shape?"""
    _, items = csr_chunk(V, N)
    return N <= 120 and B >= 2048 and items <= 16 * N + 256 and items <= 16384 and skip_row is None


def scan_tiles(V, tile=4096):
    return math.ceil((V + 1) / tile)

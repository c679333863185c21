"""The width axis of the lane-group kernels, without a device: the list of row widths the tests sweep, fp64 references of
every row-walking op in plain torch on the CPU (no call into torecsys_amd), and the makers of integer-valued operands.

A row of 16 * 2^k bytes, k = 0 .. 6, is handled by 2^k adjacent lanes of a wave, one 16-byte vector per lane
(csrc/trs_common.hpp: log2_lanes / dispatch_lanes); every other row size takes a one-thread-per-element kernel.  WIDTHS
holds all seven lane-group widths in both dtypes and the element-path neighbours: three whole vectors, 128 whole vectors
(the first power of two past the range) and a row that is no whole number of vectors.

Exactness.  Table entries and output gradients are integers in [-2, 2], per-sample weights are in {0.5, 1, 2}, a mean is
only taken over a power-of-two count.  Every term of every sum is then a multiple of 1/4 (1/8 under a mean over 8) and
every sum of magnitudes stays far below 2^22, so each partial sum, in any order, is exact in fp32 and the kernel's result
is the fp64 result rounded once to the dtype: torch.equal.  tests/test_lane_width_host.py checks that condition for every
op at every width instead of assuming it: all references below are built from the two reductions ``rsum`` and
``rscatter``, which show their terms to a watcher."""
import contextlib

import torch

F32, BF16 = torch.float32, torch.bfloat16


def elem_size(dtype):
    return 4 if dtype == F32 else 2


def log2_lanes(E, dtype):
    """k for a row of 16 * 2^k bytes, k = 0 .. 6 (the lane-group kernels), -1 for any other row (the element kernels)"""
    row_bytes = E * elem_size(dtype)
    if row_bytes % 16:
        return -1
    v = row_bytes // 16
    if v < 1 or v > 64 or v & (v - 1):
        return -1
    return v.bit_length() - 1


WIDTHS = ([(F32, 4 << k, k) for k in range(7)] + [(BF16, 8 << k, k) for k in range(7)]
          + [(F32, 12, -1), (BF16, 24, -1), (F32, 512, -1), (BF16, 1024, -1), (F32, 10, -1)])


def width_id(w):
    dtype, E, k = w
    return f"{'f32' if dtype == F32 else 'bf16'}-E{E}-k{k}"


def vec_elems(dtype):
    """elements in one 16-byte vector"""
    return 16 // elem_size(dtype)


def num_vectors(dtype, E):
    """16-byte vectors a row spans (the last one partly, where E is no whole number of them)"""
    return -(-E // vec_elems(dtype))


# ------------------------------------------------------------------------------------------------ the two reductions
_watch = None


@contextlib.contextmanager
def watching(fn):
    """inside, every rsum / rscatter calls fn(terms, dest): ``terms`` (n, ...) summed along dim 0, into one result
    (dest None) or into row dest[i] of the result (dest (n,))"""
    global _watch
    prev, _watch = _watch, fn
    try:
        yield
    finally:
        _watch = prev


def rsum(terms, dim):
    if _watch is not None:
        _watch(terms.movedim(dim, 0), None)
    return terms.sum(dim)


def rscatter(ids, terms, V):
    """zeros(V, ...).index_add_(0, ids, terms); ids outside [0, V) contribute nothing"""
    keep = (ids >= 0) & (ids < V)
    ids, terms = ids[keep], terms[keep]
    if _watch is not None:
        _watch(terms, ids)
    return terms.new_zeros(V, *terms.shape[1:]).index_add_(0, ids, terms)


# ------------------------------------------------------------------------------------------------ operand makers
def int_table(g, V, E, no_zero_rows=False):
    """(V, E) fp64 integers in [-2, 2]"""
    w = torch.randint(-2, 3, (V, E), generator=g).double()
    if no_zero_rows:
        w[:, 0] = torch.where(w.abs().sum(1) == 0, torch.ones(V, dtype=torch.float64), w[:, 0])
    return w


def int_grad(g, *shape):
    """output gradient: fp64 integers in [-2, 2]"""
    return torch.randint(-2, 3, shape, generator=g).double()


def weights(g, *shape):
    """per-sample weights in {0.5, 1, 2}"""
    return torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, shape, generator=g)]


def lane_probe(dtype, E):
    """(L + 1, E) fp64, L = the row's vector count: row v < L is zero except vector v, which holds ones; row L is all
    ones.  Any sum over rows 0 .. L-1 is the all-ones row and the dot of row L with row v is the vector's element count,
    so a lane dropped, duplicated or read at the wrong offset changes an integer that bf16 holds exactly."""
    L, VE = num_vectors(dtype, E), vec_elems(dtype)
    t = torch.zeros(L + 1, E, dtype=torch.float64)
    for v in range(L):
        t[v, v * VE: (v + 1) * VE] = 1.0
    t[L] = 1.0
    return t


# ------------------------------------------------------------------------------------------------ bag pooling
def bag_ref(w, idx, mode, pad=None, gout=None):
    """every position counts (mean = sum / L), the first position wins a tie of the max; ``pad``: the row without a
    gradient.  -> (out (B, E), grad_w (V, E) or None)"""
    idx = idx.long()
    B, L = idx.shape
    rows = w[idx]                                                                # (B, L, E)
    if mode == "max":
        out = rows.max(dim=1)[0]
        first = (rows == out.unsqueeze(1)).int().argmax(dim=1)                   # argmax: the first of equal values
        d = (torch.arange(L).view(1, L, 1) == first.unsqueeze(1)).to(w.dtype)
    else:
        scale = 1.0 / L if mode == "mean" else 1.0                               # L a power of two: exact
        out = rsum(rows, 1) * scale
        d = torch.full_like(rows, scale)
    if gout is None:
        return out, None
    grad = rscatter(idx.reshape(-1), (d * gout.unsqueeze(1)).reshape(B * L, -1), w.shape[0])
    if pad is not None:
        grad[pad] = 0
    return out, grad


# ------------------------------------------------------------------------------------------------ FM over looked-up rows
def fm_of_block(x, g_fm=None):
    """x (B, N, E) -> fm = 0.5 * (s^2 - q) (B, E), s (B, E), and d fm / d x times g_fm (B, N, E) or None"""
    s = rsum(x, 1)
    q = rsum(x * x, 1)
    fm = 0.5 * (s * s - q)
    dx = None if g_fm is None else g_fm.unsqueeze(1) * (s.unsqueeze(1) - x)
    return fm, s, dx


def embed_fm_ref(w, fw, idx, offsets, g_emb=None, g_fm=None, g_first=None, g_fields=None):
    """index selection + FM term + first-order values.  fw (V, 1).  -> dict: emb (B, N, E), fm, fm_sum (B, E), first
    (B, 1), fields (B, N, 1); with gradients given: grad_w from (g_emb, g_fm), grad_fw_first from g_first (B, 1),
    grad_fw_fields from g_fields (B, N, 1)"""
    gid = idx.long() if offsets is None else idx.long() + offsets.long().view(1, -1)
    B, N = gid.shape
    V, E = w.shape
    emb = w[gid]
    fm, s, dx = fm_of_block(emb, g_fm)
    fields = fw[gid]                                                             # (B, N, 1)
    r = dict(emb=emb, fm=fm, fm_sum=s, fields=fields, first=rsum(fields, 1))
    flat = gid.reshape(-1)
    if g_emb is not None or g_fm is not None:
        rows = torch.zeros(B, N, E, dtype=w.dtype)
        if g_emb is not None:
            rows = rows + g_emb
        if dx is not None:
            rows = rows + dx
        r["grad_w"] = rscatter(flat, rows.reshape(B * N, E), V)
    if g_first is not None:
        r["grad_fw_first"] = rscatter(flat, g_first.view(B, 1, 1).expand(B, N, 1).reshape(B * N, 1), V)
    if g_fields is not None:
        r["grad_fw_fields"] = rscatter(flat, g_fields.reshape(B * N, 1), V)
    return r


# ------------------------------------------------------------------------------------------------ pair scores
COS_EPS = 1e-8


def pair_ref(Wa, Wt, a_idx, t_idx, a_off, t_off, sim, gout=None):
    """scores (B, 1 + K) of anchor row against target rows, 'dot' or 'cosine' (each norm clamped at 1e-8, as ATen's
    cosine_similarity); Wt None: one shared table.  With gout (B, 1 + K): the gradient rows (B, 2 + K, E) ordered
    [anchor, positive, negatives] and the table gradients (one for a shared table).  Ids are inside their tables."""
    Wt_ = Wa if Wt is None else Wt
    E = Wa.shape[1]
    ai, ti = a_idx.long() + a_off, t_idx.long() + t_off
    a, t = Wa[ai].unsqueeze(1), Wt_[ti]                                          # (B, 1, E), (B, 1 + K, E)
    d = rsum(a * t, 2)
    if sim == "dot":
        s = d
    else:
        na = rsum(a * a, 2).sqrt().clamp_min(COS_EPS)                            # (B, 1)
        nt = rsum(t * t, 2).sqrt().clamp_min(COS_EPS)                            # (B, 1 + K)
        s = d / (na * nt)
    if gout is None:
        return s, None, None
    g = gout.unsqueeze(-1)
    if sim == "dot":
        ga_terms, gt_rows = g * t, g * a
        ga_rows = rsum(ga_terms, 1)
    else:                            # d/da of d / (na nt) = t / (na nt) - s a / na^2 (norms above the clamp)
        ga_rows = (g * (t / (na * nt).unsqueeze(-1) - s.unsqueeze(-1) * a / (na * na).unsqueeze(-1))).sum(1)
        gt_rows = g * (a / (na * nt).unsqueeze(-1) - s.unsqueeze(-1) * t / (nt * nt).unsqueeze(-1))
    block = torch.cat([ga_rows.unsqueeze(1), gt_rows], dim=1)
    if Wt is None:                   # one walk over the (B, 2 + K) id matrix: the two parts are one sum
        both = rscatter(torch.cat([ai.unsqueeze(1), ti], 1).reshape(-1), block.reshape(-1, E), Wa.shape[0])
        return s, block, (both,)
    ga = rscatter(ai, ga_rows, Wa.shape[0])
    gt = rscatter(ti.reshape(-1), gt_rows.reshape(-1, E), Wt_.shape[0])
    return s, block, (ga, gt)


# ------------------------------------------------------------------------------------------------ field-aware FM
def ffm_pairs(N):
    return [(i, j) for i in range(N - 1) for j in range(i + 1, N)]


def ffm_ref(ws, idx, offsets, gout=None):
    """N tables (V, E): out[:, p(i, j)] = ws[i][gid[:, j]] * ws[j][gid[:, i]], i < j in lexicographic order
    (B, N(N-1)/2, E); with gout the N table gradients"""
    gid = idx.long() + offsets.long().view(1, -1)
    N = len(ws)
    pairs = ffm_pairs(N)
    out = torch.stack([ws[i][gid[:, j]] * ws[j][gid[:, i]] for i, j in pairs], dim=1)
    if gout is None:
        return out, None
    ids = [[] for _ in range(N)]
    terms = [[] for _ in range(N)]
    for p, (i, j) in enumerate(pairs):
        ids[i].append(gid[:, j])
        terms[i].append(gout[:, p] * ws[j][gid[:, i]])
        ids[j].append(gid[:, i])
        terms[j].append(gout[:, p] * ws[i][gid[:, j]])
    return out, [rscatter(torch.cat(ids[i]), torch.cat(terms[i]), ws[i].shape[0]) for i in range(N)]


# ------------------------------------------------------------------------------------------------ sharded lookup
def unpermute_ref(back, shard, inv_pos, send_ids, self_lo, self_n):
    """(K, E): lookup k sits in slot s = inv_pos[k] of the exchange order; slots [self_lo, self_lo + self_n) read
    shard[send_ids[s]], every other slot the received rows ``back``, which are stored without that segment"""
    s = inv_pos.long()
    is_self = (s >= self_lo) & (s < self_lo + self_n)
    from_shard = shard[send_ids.long()[torch.where(is_self, s, torch.full_like(s, self_lo))]]
    slot = s - (s >= self_lo + self_n).long() * self_n
    from_back = back[torch.where(is_self, torch.zeros_like(s), slot)]
    return torch.where(is_self.unsqueeze(1), from_shard, from_back)


# ------------------------------------------------------------------------------------------------ sharded bag pooling
def _segment_of(seg_start, n):
    """segment of every position q < n (positions behind the last segment: S)"""
    return torch.bucketize(torch.arange(n), seg_start.long()[1:], right=True)


def segments_ref(shard, n_valid, ids, seg_start):
    """(S, E): the rows ids[seg_start[s] : seg_start[s + 1]] of the shard summed; ids outside [0, n_valid): zero rows"""
    S = seg_start.numel() - 1
    ids = ids.long()
    ok = (ids >= 0) & (ids < n_valid)
    rows = shard[torch.where(ok, ids, torch.zeros_like(ids))] * ok.unsqueeze(1).to(shard.dtype)
    return rscatter(_segment_of(seg_start, ids.numel()), rows, S)


def combine_ref(parts, scale):
    """(P, B, E) -> (B, E): the sum over P times ``scale``"""
    return rsum(parts, 0) * scale


def expand_ref(g_all, ids, seg_start, n_valid, pad_local_row):
    """-> rows (n, E): g_all[segment of q], and ids_bwd (n) int32: the id; a zero row and -1 for the padding row, ids
    outside the shard and positions behind the last segment"""
    S = seg_start.numel() - 1
    ids = ids.long()
    seg = _segment_of(seg_start, ids.numel())
    ok = (ids >= 0) & (ids < n_valid) & (ids != pad_local_row) & (seg < S)
    rows = g_all[seg.clamp_max(S - 1)] * ok.unsqueeze(1).to(g_all.dtype)
    return rows, torch.where(ok, ids, torch.full_like(ids, -1)).to(torch.int32)


# ------------------------------------------------------------------------------------------------ the cases
# One construction per op, used by the host test (which checks the exactness condition on it) and by the GPU test (which
# runs the kernels on it).  Everything is seeded; a case is a dict of fp64 / integer CPU tensors.
GRID_CAP_GROUPS_K6 = 4096 * 256 >> 6          # groups of 64 lanes in a forward grid capped at 4096 blocks of 256 threads
B_SECOND_TRIP = GRID_CAP_GROUPS_K6 + 5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def index_dtype(i):
    """index dtypes alternate by case"""
    return torch.int32 if i % 2 else torch.int64


def bag_cases(E, B=67, V=53, lengths=(1, 8, 9)):
    """plain bag_pool: (w, idx, mode, pad, gout); the mean only over power-of-two lengths; bag 0 lists row 0 alone"""
    for L in lengths:
        g = _gen(300 + 11 * L + E)
        w, gout = int_table(g, V, E), int_grad(g, B, E)
        idx = torch.randint(0, V, (B, L), generator=g)
        idx[0] = 0
        for pad in (0, None):
            for mode in ("sum", "mean", "max"):
                if mode == "mean" and L & (L - 1):
                    continue
                yield dict(w=w, idx=idx, mode=mode, pad=pad, gout=gout)


def probe_bag_case(dtype, E):
    """three bags that each list rows 0 .. L-1 of the lane probe once: ascending, descending, rotated by one"""
    L = num_vectors(dtype, E)
    r = torch.arange(L)
    return dict(w=lane_probe(dtype, E), idx=torch.stack([r, r.flip(0), r.roll(1)]), gout=int_grad(_gen(7 + E), 3, E))


def masked_case(E, L, B=67, V=53, pad=0):
    """the operands of test_gpu_bag_masked._all_exact_cases for the same generator: (w, idx, idx_mean, psw, gout)"""
    from test_gpu_bag_masked import _exact_bags, _exact_operands, _pow2_counts
    g = _gen(100 + 7 * L + E)
    idx = _exact_bags(g, B, L, V, pad)
    w, psw, gout = _exact_operands(g, B, L, V, E)
    return dict(seed=100 + 7 * L + E, w=w, idx=idx, idx_mean=_pow2_counts(idx, pad), psw=psw, gout=gout, pad=pad)


MASKED_COMBOS = (("sum", True, False), ("max", True, False), ("sum", True, True), ("sum", False, True),
                 ("mean", True, False))             # (mode, exclude, weighted) of _all_exact_cases, in its order
MASKED_LENGTHS = (1, 9)
HOT_LANE = ((5, 64), (6, 65), (7, 257), (8, 600))   # (table row, lookups)
HOT_ELEMENT = ((5, 32), (6, 33), (7, 257))
HOT_WIDTHS = ([(dt, E, k) for dt, E, k in WIDTHS if k in (0, 3, 5, 6)] + [(F32, 12, -1), (F32, 512, -1)])


def masked_widths():
    """every width tests/test_gpu_bag_masked.py does not reach"""
    return [(dt, E, k) for dt, E, k in WIDTHS if E not in (8, 16, 64, 128) and not (dt == F32 and E in (4, 10))]


def hot_case(E, k, B=96, L=12, V=40, pad=0):
    from test_gpu_bag_masked import _exact_operands, _planted
    g = _gen(29 + E)
    w, psw, gout = _exact_operands(g, B, L, V, E)
    idx = _planted(g, B, L, V, pad, HOT_LANE if k >= 0 else HOT_ELEMENT)
    return dict(w=w, idx=idx, psw=psw, gout=gout, pad=pad)


def fm_field_counts(k):
    return (1, 5, 65) if k in (5, 6) else (1, 5)


def fm_cases(E, k, B=67, V=40):
    """(w, fw, idx, offsets | None, g_emb, g_fm, g_first, g_fields); with offsets: field n owns rows [8 (n % 5), + 8)"""
    for N in fm_field_counts(k):
        for with_off in (False, True):
            g = _gen(500 + 3 * N + E + int(with_off))
            w, fw = int_table(g, V, E), int_table(g, V, 1)
            if with_off:
                idx, off = torch.randint(0, 8, (B, N), generator=g), (torch.arange(N) % 5) * 8
            else:
                idx, off = torch.randint(0, V, (B, N), generator=g), None
            yield dict(w=w, fw=fw, idx=idx, offsets=off, g_emb=int_grad(g, B, N, E), g_fm=int_grad(g, B, E),
                       g_first=int_grad(g, B, 1), g_fields=int_grad(g, B, N, 1))


def pair_cases(E, V=50):
    """(Wa, Wt | None, a_idx, t_idx, a_off, t_off, gout): B in {1, 67} x K in {0, 5} x shared / two tables x offsets (anchors
    in rows [3, 23), targets in rows [25, 50), as tests/test_gpu_rank.py)"""
    for B in (1, 67):
        for K in (0, 5):
            for shared in (True, False):
                for with_off in (False, True):
                    g = _gen(1000 * B + 10 * K + E + 2 * int(shared) + int(with_off))
                    Wa = int_table(g, V, E, no_zero_rows=True)
                    Wt = None if shared else int_table(g, V, E, no_zero_rows=True)
                    if with_off:
                        a_idx, t_idx = torch.randint(0, 20, (B,), generator=g), torch.randint(0, 25, (B, 1 + K), generator=g)
                        a_off, t_off = 3, 25
                    else:
                        a_idx, t_idx = torch.randint(0, V, (B,), generator=g), torch.randint(0, V, (B, 1 + K), generator=g)
                        a_off, t_off = 0, 0
                    yield dict(Wa=Wa, Wt=Wt, a_idx=a_idx, t_idx=t_idx, a_off=a_off, t_off=t_off,
                               gout=int_grad(g, B, 1 + K))


def probe_pair_case(dtype, E):
    """anchor = the all-ones row L of the lane probe, targets = rows 0 .. min(L, 33) - 1: score j = elements of vector j"""
    L = num_vectors(dtype, E)
    n = min(L, 33)
    return dict(Wa=lane_probe(dtype, E), Wt=None, a_idx=torch.tensor([L]), t_idx=torch.arange(n).view(1, n), a_off=0,
                t_off=0, gout=int_grad(_gen(9 + E), 1, n))


def ffm_cases(E, B=9, rows_per_field=11):
    """(ws, idx, offsets, gout) for N in {2, 3, 7}: 1, 3, 21 pairs"""
    for N in (2, 3, 7):
        g = _gen(700 + N + E)
        ws = [int_table(g, N * rows_per_field, E) for _ in range(N)]
        yield dict(ws=ws, idx=torch.randint(0, rows_per_field, (B, N), generator=g),
                   offsets=torch.arange(N) * rows_per_field, gout=int_grad(g, B, N * (N - 1) // 2, E))


def unpermute_case(E, B=67, N=5, V=500):
    """the construction of test_embed_fm_sharded_two_sources with integer operands: a self segment in the middle"""
    g = _gen(B + N + E)
    K = B * N
    self_lo, self_n = K // 3, K // 4
    return dict(B=B, N=N, V=V, self_lo=self_lo, self_n=self_n, inv_pos=torch.randperm(K, generator=g).to(torch.int32),
                send_ids=torch.randint(0, V, (K,), generator=g).to(torch.int32), shard=int_table(g, V, E),
                back=int_table(g, K - self_n, E))


def segment_cases(E, V=37, B=5):
    """per (world, L, owner): (shard, n_valid, ids, seg_start) as the owner receives them from bag_shard_ref.route, the
    output gradient g_all (B, E), and for the expansion ``ids_x`` with one padding id (``pad_local``) and one id past
    the shard planted"""
    import bag_shard_ref as R
    for world in (1, 3):
        per = -(-V // world)
        for L in (3, 65):
            g = _gen(900 + world + L + E)
            table = int_table(g, V, E)
            idx = torch.randint(0, V, (B, L), generator=g)
            idx[0, :world] = torch.arange(world) * per                      # every owner is looked up at least twice
            idx[1, :world] = torch.arange(world) * per + 1
            counts, seg_start, send_ids, bad = R.route(idx, V, per, world)
            assert not bad
            for me in range(world):
                lo, hi = me * per, min(V, (me + 1) * per)
                a, b = int(seg_start[me * B]), int(seg_start[(me + 1) * B])
                ids = send_ids[a:b].clone()
                assert ids.numel() >= 2
                ids_x = ids.clone()
                pad_local = int(ids[0])
                ids_x[-1] = hi - lo + 2
                if pad_local == int(ids[-1]) and ids.numel() > 2:
                    ids_x[-2] = hi - lo + 2
                yield dict(world=world, L=L, me=me, shard=table[lo:hi], n_valid=hi - lo, ids=ids, ids_x=ids_x,
                           seg_start=(seg_start[me * B: (me + 1) * B + 1] - a).to(torch.int32), pad_local=pad_local,
                           g_all=int_grad(g, B, E), table=table, idx=idx)


def second_trip_case(E, B=B_SECOND_TRIP, V=53):
    """k = 6 only: one more sample than the capped forward grid has lane groups, so the grid-stride loops run twice"""
    g = _gen(40 + E)
    return dict(w=int_table(g, V, E), fw=int_table(g, V, 1), idx=torch.randint(0, V, (B, 2), generator=g),
                psw=weights(g, B, 2), gout=int_grad(g, B, E), g2=int_grad(g, B, 2))

"""Host checks of tests/scatter_ref.py: the bucket-ladder builder, the float64 references (against autograd over the
oracle and against torch.optim), the conditions under which the GPU tests' sums are exact, and the thresholds of
csrc/scatter.hip the ladder and the CSR seams were built around."""
import pytest
import torch

import scatter_ref as R
from oracle import cpu_ref as O


@pytest.fixture(scope="module")
def ladder():
    return R.bucket_ladder(R.LADDER, R.LADDER_FIELDS, 1)


def test_ladder_gives_every_planned_row_exactly_its_length(ladder):
    fs, idx = ladder
    B, N = idx.shape
    assert N == R.LADDER_FIELDS and B == sum(R.LADDER) + 999 and 20000 < B < 26000
    maps = []
    for n in range(N):
        counts = torch.bincount(idx[:, n], minlength=fs[n])
        assert counts.numel() == fs[n]                                       # no lookup outside the field
        planned = sorted(x for x in R.LADDER if x > 1)
        assert sorted(int(c) for c in counts if c > 1) == planned            # exactly the requested bincount ...
        assert int((counts == 1).sum()) == 999 + R.LADDER.count(1)           # ... every other sample on its own row
        assert int((counts == 0).sum()) == 500 + n + R.LADDER.count(0)       # rows nobody looks up
        maps.append({int(c): int(r) for r, c in enumerate(counts) if c > 1})
    assert len(set(fs)) == N
    assert maps[0] != maps[1] and maps[1] != maps[2] and maps[0] != maps[2]  # a different assignment per field
    # sample order is permuted: the lookups of the longest row are not a run of consecutive samples
    hot = (idx[:, 0] == maps[0][4097]).nonzero().flatten()
    assert hot.numel() == 4097 and int(hot[-1] - hot[0]) > 2 * 4097
    # another seed: same table, other rows
    fs2, idx2 = R.bucket_ladder(R.LADDER, R.LADDER_FIELDS, 2)
    assert fs2 == fs and not torch.equal(idx2, idx)
    t1 = R.touched_rows(R.flat_rows(fs, idx), sum(fs))
    t2 = R.touched_rows(R.flat_rows(fs2, idx2), sum(fs))
    assert int((t1 & ~t2).sum()) > 500                                       # touched by seed 1, untouched by seed 2
    assert R.row_of_length(fs, idx, 0, 257) == maps[0][257]


def test_ladder_lengths_sit_on_the_thresholds_in_the_source():
    """Whoever retunes one of these constants must move the ladder (scatter_ref.LADDER) and the seams of
    tests/test_gpu_csr_boundaries.py with it."""
    c = R.source_constants()
    assert c["LONG_ROW"] == 64 and c["LONG_CHUNK"] == 256 and c["LONG_ROW_ELEM"] == 32 and c["ELEM_SPLIT"] == 2048
    assert c["SCAN_TILE"] == 4096 and c["ONEPASS_TILES"] == 2048
    assert c["CSR2_TINY"] == 32 and c["CSR2_STAGE"] == 24576 and c["CSR2_MAX_FIELDS"] == 120
    assert c["CSR2_CHUNK"] == 15360
    assert (c["PART_MIN_B"], c["PART_PER_FIELD"], c["PART_BASE"], c["PART_MAX_ITEMS"]) == (2048, 16, 256, 16384)
    # the chunk formula scatter_ref.csr_chunk restates: target max(256, 4 N) workgroups, chunks of 1024 ... 15360 rows
    # rounded up to 256
    assert (c["CHUNK_TARGET"], c["CHUNK_TARGET_PER_FIELD"], c["CHUNK_MIN"], c["CHUNK_ROUND"]) == (256, 4, 1024, 256)
    assert R.csr_chunk(1_000_000, 39) == (4864, 39 + 206) and R.csr_chunk(4095, 39) == (1024, 43)
    lad = set(R.LADDER)
    for edge in (c["LONG_ROW"], c["LONG_CHUNK"], c["LONG_ROW_ELEM"], c["ELEM_SPLIT"]):
        assert {edge - 1, edge, edge + 1} <= lad
    finish_unroll = 8                                                        # scatter_long_rows_finish_kernel's U
    for chunks in (finish_unroll + 1, 2 * finish_unroll, 2 * finish_unroll + 1):
        assert any((x + c["LONG_CHUNK"] - 1) // c["LONG_CHUNK"] == chunks for x in lad)
    assert (max(lad) + c["ELEM_SPLIT"] - 1) // c["ELEM_SPLIT"] == 3
    # the restated gate of the partitioned build, at the shapes tests/test_gpu_csr_boundaries.py relies on
    assert R.scan_tiles(2048 * 4096 - 1) == 2048 and R.scan_tiles(2048 * 4096) == 2049
    assert R.scan_tiles(20_000_003) == 4883
    assert R.partitioned(2048 * 4096 + 1, 39, 2048) and not R.partitioned(2048 * 4096 + 1, 39, 2047)
    assert not R.partitioned(20_000_003, 39, 2048) and R.partitioned(20_000_003, 72, 2048)
    assert R.csr_chunk(301 * 15360, 3) == (15360, 16 * 3 + 256)
    assert R.partitioned(301 * 15360, 3, 2048) and not R.partitioned(301 * 15360 + 1, 3, 2048)
    assert R.partitioned(4000, 120, 2048) and not R.partitioned(4000, 121, 2048)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ladder_and_value_range_keep_every_sum_exact(ladder, dtype):
    """The premise of tests/test_gpu_scatter_boundaries.py, on the CPU: with operands in {-2..2} and three fields, every
    element's sum of |terms| is an integer below 2**24, g*S is representable in the table dtype, and w - G/4 (the SGD
    step) is exact in fp32."""
    fs, idx = ladder
    B, N = idx.shape
    V = sum(fs)
    rows = R.flat_rows(fs, idx)
    c = R.integer_case(fs, idx, 8, 3)
    for k, t in c.items():
        assert int(t.abs().max()) == R.VALUE_RANGE, k
    w = c["w"].double()
    S = R.fm_sum(rows, N, w)
    assert float(S.abs().max()) <= N * R.VALUE_RANGE
    worst = (R.scatter_sum(rows, V, R.plain_terms(c["ge"], B, N).abs())
             + R.scatter_sum(rows, V, R.fm_terms_abs(rows, N, w, c["gf"])))
    R.assert_exact_regime(worst, [c["gf"].double() * S, c["gf1"].double() * S, w, c["ge"]], dtype)
    assert float(worst.max()) <= max(R.LADDER) * R.VALUE_RANGE * (1 + 2 * N * R.VALUE_RANGE) < 2 ** 24
    G = R.grad_plain(rows, V, c["ge"], B, N) + R.grad_fm(rows, V, N, w, c["gf"])
    step = w - 0.25 * G
    assert torch.equal(step.float().double(), step)                         # one fp32 rounding away from nothing
    # a sum that is NOT exact must be caught, not waved through
    with pytest.raises(AssertionError):
        R.assert_exact_regime(worst * 2 ** 12, [w], dtype)
    with pytest.raises(AssertionError):
        R.assert_exact_regime(worst, [w * 257.0], torch.bfloat16)


def test_references_agree_with_autograd_over_the_oracle():
    g = torch.Generator().manual_seed(4)
    fs = [5, 9, 3]
    B, N, E, V = 64, 3, 5, 17
    idx = torch.stack([torch.randint(0, f, (B,), generator=g) for f in fs], 1)
    off = O.field_offsets(fs)
    assert torch.equal(off, R.field_offsets(fs))
    rows = R.flat_rows(fs, idx)
    w = torch.randn(V, E, generator=g, dtype=torch.float64)
    w1 = torch.randn(V, 1, generator=g, dtype=torch.float64)
    ge = torch.randn(B, N, E, generator=g, dtype=torch.float64)
    gs = torch.randn(B, 1, E, generator=g, dtype=torch.float64)
    gf = torch.randn(B, E, generator=g, dtype=torch.float64)
    gf1 = torch.randn(B, 1, generator=g, dtype=torch.float64)
    g1 = torch.randn(B, N, 1, generator=g, dtype=torch.float64)
    wr, w1r = w.clone().requires_grad_(), w1.clone().requires_grad_()
    emb = O.multi_indices_embedding(wr, idx, off)
    fm = O.fm_layer(emb)
    first = O.multi_indices_embedding(w1r, idx, off)

    def grads(loss):
        wr.grad = w1r.grad = None
        loss.backward(retain_graph=True)
        return wr.grad
    close = dict(rtol=0, atol=1e-12)
    torch.testing.assert_close(R.grad_plain(rows, V, ge, B, N), grads((emb * ge).sum()), **close)
    torch.testing.assert_close(R.grad_plain(rows, V, gs, B, N), grads((emb * gs).sum()), **close)
    torch.testing.assert_close(R.grad_fm(rows, V, N, w, gf), grads((fm * gf).sum()), **close)
    torch.testing.assert_close(R.grad_fm(rows, V, N, w, gf1), grads((fm.sum(1, keepdim=True) * gf1).sum()), **close)
    grads((first * g1).sum())
    torch.testing.assert_close(R.grad_first(rows, V, g1), w1r.grad, **close)
    assert bool((R.fm_terms_abs(rows, N, w, gf) >= R.fm_terms(rows, N, w, gf).abs() - 1e-12).all())
    # a padding row and out-of-table lookups drop out
    bad = rows.clone()
    bad[3], bad[10] = -1, V
    ref = R.grad_plain(rows, V, ge, B, N) - torch.zeros(V, E, dtype=torch.float64).index_add_(
        0, rows[[3, 10]], ge.reshape(-1, E)[[3, 10]])
    torch.testing.assert_close(R.scatter_sum(bad, V, ge.reshape(-1, E)), ref, **close)
    assert torch.equal(R.touched_rows(rows, V, padding_row=int(rows[0])).nonzero().flatten(),
                       torch.tensor(sorted(set(rows.tolist()) - {int(rows[0])})))


def test_optimizer_references_agree_with_torch_optim():
    """three steps in float64: SGD and Adagrad against the dense torch.optim step (rows nobody looked up have a zero
    gradient, which leaves them alone), lazy Adam against torch.optim.SparseAdam on the coalesced touched rows"""
    g = torch.Generator().manual_seed(9)
    V, E, lr, eps, betas = 23, 4, 0.015625, 1e-8, (0.875, 0.984375)
    w0 = torch.randn(V, E, generator=g, dtype=torch.float64)
    steps = []
    for _ in range(3):
        rows = torch.randint(0, V, (30,), generator=g)
        G = R.scatter_sum(rows, V, torch.randint(-2, 3, (30, E), generator=g).double())
        steps.append((G, R.touched_rows(rows, V)))
    close = dict(rtol=1e-13, atol=1e-13)
    # SGD
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.SGD([p], lr=lr)
    w = w0.clone()
    for G, t in steps:
        p.grad = G.clone()
        opt.step()
        w = R.sgd_step(w, G, t, lr)
    torch.testing.assert_close(w, p.detach(), **close)
    # Adagrad
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.Adagrad([p], lr=lr, eps=1e-10)
    w, s = w0.clone(), torch.zeros_like(w0)
    for G, t in steps:
        p.grad = G.clone()
        opt.step()
        w_prev, s_prev = w, s
        w, s, tol_w, tol_s = R.adagrad_step(w, s, G, t, lr, 1e-10)
        assert torch.equal(w[~t], w_prev[~t]) and torch.equal(s[~t], s_prev[~t])
        assert float(tol_w[~t].max()) == 0.0 and bool((tol_w[t] > 0).any()) and bool((tol_s >= 0).all())
    torch.testing.assert_close(w, p.detach(), **close)
    torch.testing.assert_close(s, opt.state[p]["sum"], **close)
    # lazy Adam
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.SparseAdam([p], lr=lr, betas=betas, eps=eps)
    w, m, v = w0.clone(), torch.zeros_like(w0), torch.zeros_like(w0)
    for k, (G, t) in enumerate(steps):
        r = t.nonzero().flatten()
        p.grad = torch.sparse_coo_tensor(r.unsqueeze(0), G[r], size=G.shape)
        opt.step()
        ss = lr * (1.0 - betas[1] ** (k + 1)) ** 0.5 / (1.0 - betas[0] ** (k + 1))
        assert abs(R.adam_step_size(lr, betas, k + 1) - ss) <= 2.0 ** -24 * ss
        w_prev, m_prev = w, m
        w, m, v, tol_w, tol_m, tol_v = R.lazy_adam_step(w, m, v, G, t, ss, betas, eps)
        assert torch.equal(w[~t], w_prev[~t]) and torch.equal(m[~t], m_prev[~t])
        assert float(tol_w[~t].max()) == 0.0 and bool((tol_m >= 0).all()) and bool((tol_v >= 0).all())
    torch.testing.assert_close(w, p.detach(), **close)
    torch.testing.assert_close(m, opt.state[p]["exp_avg"], **close)
    torch.testing.assert_close(v, opt.state[p]["exp_avg_sq"], **close)


def test_bf16_half_ulp_and_rounding_helpers():
    x = torch.tensor([1.0, 1.5, 2.0, 3.0, 0.015625, 300.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -14, 1.0], dtype=torch.float64)
    assert torch.equal(R.bf16_half_ulp(x), want)
    # ties go to even, as at::BFloat16 rounds: 257 -> 256, 259 -> 260, 57 358 (a 4097-lookup sum) -> 57 344
    ref = torch.tensor([257.0, 259.0, 57358.0], dtype=torch.float64)
    assert R.rounded(ref, torch.bfloat16).tolist() == [256.0, 260.0, 57344.0]
    assert torch.equal(R.rounded(ref, torch.float32).double(), ref)
    assert R.as_f32(0.015625) == 0.015625 and R.as_f32(0.1) != 0.1


def test_widths_take_the_path_they_are_listed_under():
    """the row widths of tests/test_gpu_scatter_boundaries.py: one per instantiation of the vector path (1, 2, 4, 16, 64
    vectors of 16 bytes), the others not a power-of-two count of whole vectors"""
    from test_gpu_scatter_boundaries import BF16, F32, WIDTHS
    assert len(WIDTHS) == 18
    for dtype, E, path in WIDTHS:
        row_bytes = E * (4 if dtype == F32 else 2)
        vecs = row_bytes // 16
        is_vec = row_bytes % 16 == 0 and vecs & (vecs - 1) == 0 and 0 < vecs <= 64
        assert is_vec == (path == "vec"), (dtype, E)
    for dtype in (F32, BF16):
        assert sorted((E * (4 if dtype == F32 else 2)) // 16 for d, E, p in WIDTHS if p == "vec" and d == dtype) == [1, 2, 4, 16, 64]

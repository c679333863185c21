"""GPU: every kernel that walks embedding rows, at every lane-group width (rows of 16 * 2^k bytes, k = 0 .. 6, in fp32 and
bf16) and at the element-path neighbours of that range (3 and 128 whole vectors, a row that is no whole number of
vectors) -- tests/lane_width_ref.WIDTHS -- against fp64 references in plain torch on the CPU.  The operands are integer
valued (tests/lane_width_ref.py; tests/test_lane_width_host.py checks for these very cases that every partial sum is
exact in fp32), so a kernel's result is the fp64 result rounded once to the dtype, in whatever order it adds:
torch.equal, unless stated otherwise (the cosine: the bounds of tests/test_gpu_rank.py).  Index dtypes alternate by case.

Measured worst cosine rel_err (printed by test_pair_scores): see profiles/lane_width_cases.md."""
import pytest
import torch

import bag_shard_ref as S
import lane_width_ref as R
from conftest import rel_err
from lane_width_ref import BF16, F32, WIDTHS, width_id
from test_gpu_bag_masked import _all_exact_cases, _check_exact
from test_gpu_rank import TOL

pytestmark = pytest.mark.gpu

K6 = [w for w in WIDTHS if w[2] == 6]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def no_index_errors():
    from torecsys_amd import functional as F_
    F_.index_errors_seen()
    yield
    assert not F_.index_errors_seen()


def _path_is(dtype, E, k):
    """the device-free path query agrees with the case's k"""
    from torecsys_amd import functional as F_
    assert R.log2_lanes(E, dtype) == k
    assert F_.pair_score_path(E, dtype) == (1 if k >= 0 else 0)


def _eq(got, want, dtype, tag):
    """bit equality with the fp64 reference rounded once"""
    got = got.detach().cpu()
    assert got.dtype == dtype, tag
    assert torch.equal(got, want.to(dtype).reshape(got.shape)), tag


# ------------------------------------------------------------------------------------------------ 1. bag_pool, plain
def _bag(dev, dtype, idt, c, mode, pad):
    from torecsys_amd import functional as F_
    wd = c["w"].to(dtype).to(dev).requires_grad_()
    y = F_.bag_pool(wd, c["idx"].to(dev).to(idt), mode, padding_idx=pad)
    assert tuple(y.shape) == (c["idx"].shape[0], 1, c["w"].shape[1])
    y.backward(c["gout"].to(dtype).to(dev).unsqueeze(1))
    return y.detach().squeeze(1), wd.grad


@pytest.mark.parametrize("width", WIDTHS, ids=width_id)
def test_bag_pool_plain(dev, width):
    """B = 67, V = 53, L in {1, 8, 9} (the mean at 1 and 8): output and dense table gradient of sum / mean / max with
    padding_idx 0 and None; the padding row's gradient is exactly zero.  Then the lane probe: bags that list rows
    0 .. L-1 once give all ones under sum; under max they give all ones with vector v won by row v, which the gradient
    shows -- row v receives g in vector v alone."""
    dtype, E, k = width
    _path_is(dtype, E, k)
    n = 0
    for i, c in enumerate(R.bag_cases(E)):
        want_y, want_g = R.bag_ref(c["w"], c["idx"], c["mode"], c["pad"], c["gout"])
        y, grad = _bag(dev, dtype, R.index_dtype(i + E), c, c["mode"], c["pad"])
        tag = (c["mode"], c["pad"], c["idx"].shape[1])
        _eq(y, want_y, dtype, tag)
        _eq(grad, want_g, dtype, tag)
        if c["pad"] is not None:
            assert float(grad[c["pad"]].abs().max()) == 0.0, tag
        n += 1
    assert n == 2 * (3 + 3 + 2)
    c = R.probe_bag_case(dtype, E)
    L, VE = R.num_vectors(dtype, E), R.vec_elems(dtype)
    for i, mode in enumerate(("sum", "max")):
        want_y, want_g = R.bag_ref(c["w"], c["idx"], mode, None, c["gout"])
        assert bool((want_y == 1.0).all())
        y, grad = _bag(dev, dtype, R.index_dtype(i), c, mode, None)
        _eq(y, want_y, dtype, ("probe", mode))
        _eq(grad, want_g, dtype, ("probe", mode))
        if mode == "max":
            own = torch.zeros(L + 1, E, dtype=torch.bool)
            for v in range(L):
                own[v, v * VE: (v + 1) * VE] = True
            assert float(grad.cpu()[~own].abs().max()) == 0.0
            assert torch.equal(grad.cpu()[:L].sum(0).double(), c["gout"].sum(0))


# ------------------------------------------------------------------------------------------------ 2. masked, weighted
@pytest.mark.parametrize("L", R.MASKED_LENGTHS)
@pytest.mark.parametrize("width", R.masked_widths(), ids=width_id)
def test_bag_pool_masked_and_weighted(dev, width, L):
    """the five combinations of test_gpu_bag_masked._all_exact_cases (sum / max / weighted sum with and without
    exclusion / mean over power-of-two counts; outputs, table gradient, dw) at the widths that file does not reach"""
    dtype, E, k = width
    _path_is(dtype, E, k)
    seed = R.masked_case(E, L)["seed"]
    _all_exact_cases(dev, dtype, R.index_dtype(L // 8 + (E >> 3)), torch.Generator().manual_seed(seed), 67, L, 53, E,
                     0)


# ------------------------------------------------------------------------------------------------ 3. hot rows
@pytest.mark.parametrize("width", R.HOT_WIDTHS, ids=width_id)
def test_hot_rows(dev, width):
    """table rows with exactly 64, 65, 257 and 600 lookups (element path: 32, 33, 257) in B * L = 96 * 12 positions: the
    weighted sum with and without exclusion and the max, whose walks fold 64 / 2^k lane groups per wave"""
    dtype, E, k = width
    _path_is(dtype, E, k)
    c = R.hot_case(E, k)
    for r, n in (R.HOT_LANE if k >= 0 else R.HOT_ELEMENT):
        assert int((c["idx"] == r).sum()) == n
    for i, (mode, exclude, weighted) in enumerate((("sum", True, True), ("sum", False, True), ("max", True, False))):
        _check_exact(dev, dtype, R.index_dtype(i + (E >> 2)), c["w"], c["idx"], mode, c["pad"], exclude,
                     c["psw"] if weighted else None, c["gout"])


# ------------------------------------------------------------------------------------------------ 4. lookup + FM
@pytest.mark.parametrize("width", WIDTHS, ids=width_id)
def test_embed_fm(dev, width):
    """B = 67, V = 40, N in {1, 5} (and 65 at k = 5, 6: the first-order values' placement in the group wraps), with and
    without offsets, a first-order table of the same dtype: embed_fm and embed_fm_fields -- the block bitwise, the FM
    term, the first-order sum / per-field values, both tables' gradients -- and fm_layer on the same block."""
    from torecsys_amd import functional as F_
    dtype, E, k = width
    _path_is(dtype, E, k)

    def d(t):
        return t.to(dtype).to(dev)

    n = 0
    for i, c in enumerate(R.fm_cases(E, k)):
        idt = R.index_dtype(i + (E >> 2))
        idx = c["idx"].to(dev).to(idt)
        off = None if c["offsets"] is None else c["offsets"].to(dev)
        want = R.embed_fm_ref(c["w"], c["fw"], c["idx"], c["offsets"], c["g_emb"], c["g_fm"], c["g_first"], c["g_fields"])
        tag = (c["idx"].shape[1], off is not None, idt)
        for fields in (False, True):
            w, fw = d(c["w"]).requires_grad_(), d(c["fw"]).requires_grad_()
            if fields:
                emb, fm, first = F_.embed_fm_fields(w, fw, idx, off)
                g1, want_first, want_gfw = c["g_fields"], want["fields"], want["grad_fw_fields"]
            else:
                emb, fm, first = F_.embed_fm(w, idx, off, fw)
                g1, want_first, want_gfw = c["g_first"], want["first"], want["grad_fw_first"]
            _eq(emb, want["emb"], dtype, tag)
            _eq(fm, want["fm"], dtype, tag)
            _eq(first, want_first, dtype, (tag, fields))
            torch.autograd.backward([emb, fm, first], [d(c["g_emb"]), d(c["g_fm"]), d(g1)])
            _eq(w.grad, want["grad_w"], dtype, (tag, fields))
            _eq(fw.grad, want_gfw, dtype, (tag, fields))
        # the FM term alone (no block gradient): the walk with the broadcast operand only
        w = d(c["w"]).requires_grad_()
        _, fm, _ = F_.embed_fm(w, idx, off, None, want_emb=False)
        fm.backward(d(c["g_fm"]))
        _eq(w.grad, R.embed_fm_ref(c["w"], c["fw"], c["idx"], c["offsets"], None, c["g_fm"])["grad_w"], dtype, tag)
        # fm_layer on the block
        x = d(want["emb"]).requires_grad_()
        y = F_.fm_layer(x)
        y.backward(d(c["g_fm"]))
        want_fm, _, want_dx = R.fm_of_block(want["emb"], c["g_fm"])
        _eq(y, want_fm, dtype, tag)
        _eq(x.grad, want_dx, dtype, tag)
        n += 1
    assert n == 2 * len(R.fm_field_counts(k))


# ------------------------------------------------------------------------------------------------ 5. pair scores
def _pair_device(dev, dtype, idt, c):
    wa = c["Wa"].to(dtype).to(dev).requires_grad_()
    wt = None if c["Wt"] is None else c["Wt"].to(dtype).to(dev).requires_grad_()
    return wa, wt, c["a_idx"].to(dev).to(idt), c["t_idx"].to(dev).to(idt)


@pytest.mark.parametrize("width", WIDTHS, ids=width_id)
def test_pair_scores(dev, width):
    """B in {1, 67} x K in {0, 5} x shared / two tables x offsets.  dot: fp32 scores exact, scores in the table dtype the
    fp64 result rounded once, gradient rows (pair_scores_backward_raw) and table gradients exact.  cosine: the same cases
    against the fp64 reference within the bounds of tests/test_gpu_rank.py.  Lane probe: the all-ones row against rows
    0 .. min(L, 33) - 1 scores the element count of each vector."""
    from torecsys_amd import functional as F_
    dtype, E, k = width
    _path_is(dtype, E, k)
    cases = list(R.pair_cases(E))
    assert len(cases) == 16
    worst = [0.0, 0.0, 0.0]
    for i, c in enumerate(cases + [R.probe_pair_case(dtype, E)]):
        idt = R.index_dtype(i + (E >> 2))
        probe = i == len(cases)
        tag = ("probe" if probe else i, idt)
        for sim in ("dot", "cosine"):
            want_s, want_block, want_grads = R.pair_ref(c["Wa"], c["Wt"], c["a_idx"], c["t_idx"], c["a_off"], c["t_off"],
                                                        sim, c["gout"])
            wa, wt, a_idx, t_idx = _pair_device(dev, dtype, idt, c)
            gout = c["gout"].to(dtype).to(dev)
            s32 = F_.pair_scores(wa.detach(), a_idx, None if wt is None else wt.detach(), t_idx, c["a_off"], c["t_off"], sim,
                                 out_dtype=torch.float32)
            s = F_.pair_scores(wa, a_idx, wt, t_idx, c["a_off"], c["t_off"], sim)
            assert s.dtype == dtype and s32.dtype == torch.float32
            (s * gout).sum().backward()
            block = F_.pair_scores_backward_raw(wa.detach(), a_idx, (wa if wt is None else wt).detach(), t_idx, gout,
                                                c["a_off"], c["t_off"], sim)
            grads = [w.grad for w in (wa, wt) if w is not None]
            if sim == "dot":
                _eq(s32, want_s, torch.float32, tag)
                _eq(s, want_s, dtype, tag)
                _eq(block, want_block, dtype, tag)
                for got, want in zip(grads, want_grads):
                    _eq(got, want, dtype, tag)
                if probe:
                    VE = R.vec_elems(dtype)
                    counts = [min(VE, E - v * VE) for v in range(t_idx.shape[1])]
                    assert s32.cpu().tolist() == [[float(x) for x in counts]], tag
                    assert k < 0 or counts == [VE] * len(counts)
            elif probe and t_idx.shape[1] == 1:
                # a row of one vector: the probe's anchor row equals its only target row, the cosine is 1 and its gradient
                # vanishes.  rel_err against a zero reference says nothing, so the rows are held to the same bound relative
                # to the terms g t / (|a| |t|) and g s a / |a|^2 that cancel in them, each at most |g| in magnitude.
                bound = TOL[dtype] * max(1.0, float(c["gout"].abs().max()))
                assert float(want_block.abs().max()) <= 1e-15
                assert rel_err(s32.cpu(), want_s) <= TOL[torch.float32] and rel_err(s.float().cpu(), want_s) <= TOL[dtype]
                assert float(block.float().abs().max()) <= bound and float(grads[0].float().abs().max()) <= bound, tag
            else:
                errs = [max(rel_err(s32.cpu(), want_s), rel_err(s.float().cpu(), want_s)),
                        rel_err(block.float().cpu(), want_block),
                        max(rel_err(got.float().cpu(), want) for got, want in zip(grads, want_grads))]
                worst = [max(a, b) for a, b in zip(worst, errs)]
                assert rel_err(s32.cpu(), want_s) <= TOL[torch.float32], (tag, errs)
                assert max(errs) <= TOL[dtype], (tag, errs)
    print(f"pair_scores cosine {width_id(width)}: worst rel_err scores {worst[0]:.2e} rows {worst[1]:.2e} "
          f"table {worst[2]:.2e}")


# ------------------------------------------------------------------------------------------------ 6. fused FFM
@pytest.mark.parametrize("width", WIDTHS, ids=width_id)
def test_ffm_fused(dev, width):
    """N in {2, 3, 7} (1, 3, 21 pairs: 21 exceeds the pairs one pass keeps in flight at the widest group), B = 9, 11 rows
    per field: output and the N table gradients exact, a row nobody looked up exactly zero"""
    from torecsys_amd import functional as F_
    dtype, E, k = width
    _path_is(dtype, E, k)
    for i, c in enumerate(R.ffm_cases(E)):
        idt = R.index_dtype(i + (E >> 2))
        N = len(c["ws"])
        want_y, want_g = R.ffm_ref(c["ws"], c["idx"], c["offsets"], c["gout"])
        ws = [w.to(dtype).to(dev).requires_grad_() for w in c["ws"]]
        y = F_.ffm_fused(ws, c["idx"].to(dev).to(idt), c["offsets"].to(dev))
        _eq(y, want_y, dtype, (N, idt))
        y.backward(c["gout"].to(dtype).to(dev))
        gid = c["idx"] + c["offsets"].view(1, -1)
        unseen = torch.ones(ws[0].shape[0], dtype=torch.bool)
        unseen[gid.reshape(-1)] = False
        assert bool(unseen.any())
        for w, want in zip(ws, want_g):
            _eq(w.grad, want, dtype, (N, idt))
            assert float(w.grad.cpu()[unseen].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 7. sharded lookup
@pytest.mark.parametrize("width", WIDTHS, ids=width_id)
def test_unpermute_local(dev, width):
    """trs_embed_fm_sharded with both sources in play (the construction of test_embed_fm_sharded_two_sources, integer
    operands, B = 67, N = 5): the block bit-exact, fm and fm_sum exact.  Its ids are int32 by contract."""
    from torecsys_amd.dist import HipOps
    dtype, E, k = width
    _path_is(dtype, E, k)
    c = R.unpermute_case(E)
    B, N = c["B"], c["N"]
    want = R.unpermute_ref(c["back"], c["shard"], c["inv_pos"], c["send_ids"], c["self_lo"], c["self_n"])
    want_fm, want_sum, _ = R.fm_of_block(want.reshape(B, N, E))
    block, fm, fm_sum = HipOps().unpermute_local(c["back"].to(dtype).to(dev), c["shard"].to(dtype).to(dev), c["V"],
                                                 c["inv_pos"].to(dev), c["send_ids"].to(dev), c["self_lo"], c["self_n"],
                                                 B, N, True)
    torch.cuda.synchronize()
    _eq(block, want, dtype, "block")
    assert fm is not None and fm_sum is not None
    _eq(fm, want_fm, dtype, "fm")
    _eq(fm_sum, want_sum, torch.float32, "fm_sum")


# ------------------------------------------------------------------------------------------------ 8. sharded bag pooling
@pytest.mark.parametrize("width", WIDTHS, ids=width_id)
def test_bag_segments_combine_expand(dev, width):
    """world in {1, 3}, B = 5, L in {3, 65}, every owner: bag_pool_segments against the fp64 segment sums (not against
    bag_pool), bag_combine of the owners' parts against the whole-table sum, bag_expand_grad with one padding id and one id
    past the shard (zero rows, id -1).  The owner-side ids are int32 by contract."""
    from torecsys_amd.dist import HipOps
    dtype, E, k = width
    _path_is(dtype, E, k)
    ops = HipOps()
    parts, n = {}, 0
    for c in R.segment_cases(E):
        tag = (c["world"], c["L"], c["me"])
        shard, seg = c["shard"].to(dtype).to(dev), c["seg_start"].to(dev)
        want = R.segments_ref(c["shard"], c["n_valid"], c["ids"], c["seg_start"])
        got = ops.bag_pool_segments(shard, c["n_valid"], c["ids"].to(dev), seg)
        _eq(got, want, torch.float32, tag)
        parts.setdefault((c["world"], c["L"]), []).append((got, want, c))
        g_all = c["g_all"].to(dtype).to(dev)
        rows, ids_bwd = ops.bag_expand_grad(g_all, c["ids_x"].to(dev), seg, c["n_valid"], c["pad_local"])
        want_rows, want_ids = R.expand_ref(c["g_all"], c["ids_x"], c["seg_start"], c["n_valid"], c["pad_local"])
        _eq(rows, want_rows, dtype, tag)
        assert torch.equal(ids_bwd.cpu(), want_ids), tag
        gone = (c["ids_x"] == c["pad_local"]) | (c["ids_x"] >= c["n_valid"])
        assert int(gone.sum()) >= 2 and torch.equal(ids_bwd.cpu() == -1, gone), tag
        assert float(rows.cpu()[gone].abs().max()) == 0.0, tag
        n += 1
    assert n == 8
    for (world, L), owners in parts.items():
        c = owners[0][2]
        whole = c["table"][c["idx"]].sum(1)
        for scale in (1.0, 0.25):
            got = ops.bag_combine(torch.stack([o[0] for o in owners]), scale, dtype)
            want = R.combine_ref(torch.stack([o[1] for o in owners]), scale)
            assert torch.equal(want, whole * scale)
            _eq(got, want, dtype, (world, L, scale))


# ------------------------------------------------------------------------------------------------ 9. the second trip
@pytest.mark.parametrize("width", K6, ids=width_id)
def test_second_trip_of_the_forward_loops(dev, width):
    """k = 6, B = 16 384 + 5: one sample more than a forward grid capped at 4096 blocks has lane groups, so the
    grid-stride loops over samples run a second time: bag_pool sum (L = 2), the weighted sum with dw (B * L = 32 778
    positions against the 32 768 groups of that grid), embed_fm (N = 2), pair_scores dot (K = 1), bag_pool_segments with
    that many segments of length 1.  All exact."""
    from torecsys_amd import functional as F_
    from torecsys_amd.dist import HipOps
    dtype, E, k = width
    _path_is(dtype, E, 6)
    B = R.B_SECOND_TRIP
    assert B << 6 > 4096 * 256 and B * 2 > 2 * (4096 * 256 >> 6)
    c = R.second_trip_case(E)
    idt = R.index_dtype(E >> 8)
    idx = c["idx"].to(dev).to(idt)

    def d(t):
        return t.to(dtype).to(dev)

    want_y, want_g = R.bag_ref(c["w"], c["idx"], "sum", None, c["gout"])
    y, grad = _bag(dev, dtype, idt, c, "sum", None)
    _eq(y, want_y, dtype, "bag sum")
    _eq(grad, want_g, dtype, "bag sum")
    _check_exact(dev, dtype, idt, c["w"], c["idx"], "sum", 0, False, c["psw"], c["gout"])

    want = R.embed_fm_ref(c["w"], c["fw"], c["idx"], None, None, c["gout"], c["g2"][:, :1])
    w, fw = d(c["w"]).requires_grad_(), d(c["fw"]).requires_grad_()
    emb, fm, first = F_.embed_fm(w, idx, None, fw)
    _eq(emb, want["emb"], dtype, "emb")
    _eq(fm, want["fm"], dtype, "fm")
    _eq(first, want["first"], dtype, "first")
    torch.autograd.backward([fm, first], [d(c["gout"]), d(c["g2"][:, :1])])
    _eq(w.grad, want["grad_w"], dtype, "fm grad")
    _eq(fw.grad, want["grad_fw_first"], dtype, "first grad")

    want_s, want_block, want_grads = R.pair_ref(c["w"], None, c["idx"][:, 0], c["idx"], 0, 0, "dot", c["g2"])
    w = d(c["w"]).requires_grad_()
    s = F_.pair_scores(w, idx[:, 0].contiguous(), None, idx, sim="dot", out_dtype=torch.float32)
    _eq(s, want_s, torch.float32, "scores")
    (s * c["g2"].float().to(dev)).sum().backward()
    _eq(w.grad, want_grads[0], dtype, "pair grad")
    block = F_.pair_scores_backward_raw(w.detach(), idx[:, 0].contiguous(), w.detach(), idx, d(c["g2"]), 0, 0, "dot")
    _eq(block, want_block, dtype, "pair rows")

    ids = c["idx"][:, 0].to(torch.int32)
    seg = torch.arange(B + 1, dtype=torch.int32)
    got = HipOps().bag_pool_segments(d(c["w"]), c["w"].shape[0], ids.to(dev), seg.to(dev))
    _eq(got, R.segments_ref(c["w"], c["w"].shape[0], ids, seg), torch.float32, "segments")

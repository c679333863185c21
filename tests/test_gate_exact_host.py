"""Host checks of tests/gate_exact_ref.py: the operands of every case tests/test_gpu_moe_exact.py,
tests/test_gpu_senet_exact.py and tests/test_gpu_rank_loss_exact.py run are exact in fp32 (and survive their dtype), the
dispatch arithmetic restated there agrees with the text of csrc/moe.hip, csrc/senet.hip and csrc/rank.hip, and the case
lists reach what they exist for: every instantiation, both fill states, every wave count, every second trip."""
import pytest
import torch

import gate_exact_ref as R

F32, BF16, F64 = R.F32, R.BF16, R.F64


# ---------------------------------------------------------------------------------------------------------------------
# the sources
# ---------------------------------------------------------------------------------------------------------------------
def test_constants_match_the_sources():
    c = R.source_constants()
    assert c["MOE_LANE_COLS"] == R.MOE_LANE_COLS and c["MOE_TILE_COLS"] == R.MOE_TILE_COLS
    assert 256 * c["MOE_GRID_VEC"] == 256 * c["MOE_GRID_FWD_ELEM"] == 256 * c["MOE_GRID_BWD_ELEM"] == R.STREAM_GRID_CAP
    assert c["MOE_DISPATCH_LG"] == [0, 1, 2, 3, 4, 5]
    assert (c["SENET_MAX_M"], c["SENET_MAX_VEC"], c["SENET_MAX_BLOCKS"], c["SENET_FIN_SEG"]) == \
        (R.SENET_MAX_M, R.SENET_MAX_VEC, R.SENET_MAX_BLOCKS, R.SENET_FIN_SEG)
    assert c["SENET_LDS_KIB"] * 1024 == R.SENET_LDS_CAP
    assert c["SENET_STEPS"] == c["SENET_DISPATCH"] == R.SENET_STEPS
    assert 256 * c["SENET_ROW_GRID"] == 256 * c["SENET_SCALE_GRID"] == R.STREAM_GRID_CAP
    assert (c["RANK_BLOCK"], c["RANK_MAX_BLOCKS"], c["RANK_FINISH_LANES"]) == \
        (R.RANK_BLOCK, R.RANK_MAX_BLOCKS, R.RANK_FINISH_LANES)


def test_the_lds_formulas_match_the_source():
    """senet_bwd_lds / senet_quad_floats, term by term as senet.hip spells them"""
    import os
    with open(os.path.join(R.CSRC, "senet.hip")) as f:
        src = f.read()
    assert "return (size_t)4 * (((M + 3) / 4) * H + ((H + 3) / 4) * M);" in src
    assert "const size_t P = (size_t)2 * M * H + M + H;\n  return sizeof(float) * (senet_quad_floats(M, H) + nw * P + " \
           "(size_t)nw * (2 * nvec + 128));" in src
    assert "int nw = 4;\n  while (nw > 1 && senet_bwd_lds(M, H, nvec, nw) > 64 * 1024) nw >>= 1;" in src
    assert "const int per = (nslab + SENET_FIN_SEG - 1) / SENET_FIN_SEG;" in src
    # 64 fields, 64 hidden units, E = 16 fp32: a strip of 8320 accumulators a wave
    assert R.senet_bwd_lds(64, 64, 256, 1) == 4 * (8192 + 8320 + 640)


# ---------------------------------------------------------------------------------------------------------------------
# MoE gate
# ---------------------------------------------------------------------------------------------------------------------
def test_moe_dispatch_rule():
    assert R.moe_group(4, F32) == (0, 1, 1) and R.moe_group(8, BF16) == (0, 1, 1)
    assert R.moe_group(12, F32) == (2, 1, 3) and R.moe_group(256, F32) == (6, 1, 64)
    assert R.moe_group(260, F32) == (6, 2, 65) and R.moe_group(516, F32) == (6, 4, 129)
    assert R.moe_group(1024, BF16) == (6, 2, 128) and R.moe_group(1024, F32) == (6, 4, 256)
    assert R.moe_path(1028, F32) == R.ELEMENT and R.moe_path(12, BF16) == R.ELEMENT and R.moe_path(12, F32) == R.VECTOR
    assert R.moe_path(64, F32, aligned=False) == R.ELEMENT
    assert R.moe_bwd_tiles(512) == 1 and R.moe_bwd_tiles(513) == 2 and R.moe_bwd_tiles(2051) == 5


def test_moe_cases_reach_every_instantiation():
    for dtype, reached in ((F32, {(lg, 1) for lg in range(7)} | {(6, 2), (6, 4)}),
                           (BF16, {(lg, 1) for lg in range(7)} | {(6, 2)})):
        ks = R.MOE_VECTOR_K[dtype]
        assert all(R.moe_path(K, dtype) == R.VECTOR for K in ks)
        assert {R.moe_group(K, dtype)[:2] for K in ks} == reached
        fills = {(R.moe_group(K, dtype)[0], R.moe_fill(K, dtype)) for K in ks}
        for lg in range(2, 6):                      # one or two vectors fill a group of one or two lanes: lg 0, 1 are full
            assert (lg, "full") in fills and (lg, "part") in fills, (dtype, lg)
        for lg, R_ in reached:
            if lg == 6:
                assert {R.moe_fill(K, dtype) for K in ks if R.moe_group(K, dtype)[:2] == (6, R_)} == {"full", "part"}
        assert all(R.moe_path(K, dtype) == R.ELEMENT for K in R.MOE_ELEMENT_K[dtype])
        assert {min(R.moe_bwd_tiles(K), 2) for K in R.MOE_ELEMENT_K[dtype]} == {1, 2}
        assert any(K > 64 and K % 64 for K in R.MOE_ELEMENT_K[dtype])
    # three and four vectors per lane under lg 6 / R 4
    per = {K: -(-R.moe_group(K, F32)[2] // 64) for K in (516, 768, 772, 1024)}
    assert per == {516: 3, 768: 3, 772: 4, 1024: 4}
    assert R.moe_path(R.MOE_UNALIGNED_K, F32) == R.moe_path(R.MOE_UNALIGNED_K, BF16) == R.VECTOR
    # rows that are multiples of 4 columns but no whole vectors in bf16
    assert all(K % 4 == 0 and R.moe_path(K, BF16) == R.ELEMENT for K in (4, 12, 20))


def test_moe_second_trips():
    for dtype, K, G, B in R.MOE_TRIP_VECTOR:
        lg = R.moe_group(K, dtype)[0]
        assert B << lg > R.STREAM_GRID_CAP * 256
        assert R.moe_trips(R.VECTOR, B, G, K, dtype, False) == R.moe_trips(R.VECTOR, B, G, K, dtype, True) == 2
    assert {R.moe_group(K, d)[0] for d, K, _, _ in R.MOE_TRIP_VECTOR} == {0, 6}
    for dtype, K, G, B in R.MOE_TRIP_ELEMENT:
        assert B * 64 > R.STREAM_GRID_CAP * 256 and R.moe_path(K, dtype) == R.ELEMENT
        assert R.moe_trips(R.ELEMENT, B, G, K, dtype, False) == R.moe_trips(R.ELEMENT, B, G, K, dtype, True) == 2
    # the cases of 67 samples stay within one trip
    assert R.moe_trips(R.VECTOR, R.MOE_B, 4, 1024, F32, True) == 1


@pytest.mark.parametrize("case", R.MOE_VECTOR_CASES + R.MOE_ELEMENT_CASES, ids=R.moe_case_id)
def test_moe_operands_are_exact(case):
    dtype, K = case
    some_full = False
    for G in R.MOE_GS:
        for bias in (False, True):
            o = R.moe_operands(R.MOE_B, G, K, bias)
            r = R.moe_ref(o)
            R.assert_moe_exact(o, r)
            for t in (o.experts, o.gout) + ((o.bias,) if bias else ()):
                assert torch.equal(t.to(dtype).to(F64), t)
            assert bool(o.live[..., 0].any()) and bool(o.live[..., K - 1].any())
            assert len(set(o.logits.view(-1, K).max(1).values.tolist())) > 1 or bias      # c differs between the rows
            some_full |= bool((o.n == K).any())
            assert bool((r.gexperts != 0).any()) and bool((r.out != 0).any())
            assert bool((r.glogits != 0).any()) or K == 1                         # one column: P = 1 whatever the logit
    if R.pow2(K):
        assert some_full


def test_moe_large_operands_are_exact():
    for dtype, K, G, B in R.MOE_TRIP_VECTOR[:1] + R.MOE_TRIP_ELEMENT[:1]:
        o = R.moe_operands(B, G, K, True)
        R.assert_moe_exact(o, R.moe_ref(o))


def test_exp_of_a_dead_column_is_zero_in_float64():
    assert float(torch.exp(torch.tensor(R.MOE_DEAD - 3, dtype=F64))) == 0.0
    assert float(torch.exp(torch.tensor(R.MOE_DEAD + 3, dtype=F32))) == 0.0
    assert float(torch.exp(torch.tensor(0.0, dtype=F32))) == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# SENET
# ---------------------------------------------------------------------------------------------------------------------
def test_senet_cases_reach_every_step_and_wave_count():
    for dtype in R.DTYPES:
        for k, shapes in R.SENET_STEP_SHAPES[dtype].items():
            for M, H, E in shapes:
                assert R.senet_fused_ok(M, H, E, dtype) and R.senet_vec_per_lane(M, E, dtype) == k, (dtype, M, H, E)
        assert sorted(R.SENET_STEP_SHAPES[dtype]) == R.SENET_STEPS
        mine = [c for c in R.SENET_FUSED_CASES if c[0] is dtype]
        assert {c[1] % 4 for c in mine} == {0, 1, 2, 3} and {c[2] % 4 for c in mine} == {0, 1, 2, 3}
        assert {c[2] for c in mine} >= {1, 2, 3, 13} and any(c[1] == c[2] for c in mine)
        assert {R.senet_bwd_waves(*c[1:4], dtype) for c in mine} == {1, 2, 4}
        assert any(not R.pow2(c[3]) for c in mine)
        assert R.senet_bwd_waves(64, 64, 16, dtype) == 1 and R.senet_bwd_waves(64, 32, 16, dtype) == 2
        nvec = 64 * (16 * R.size_of(dtype) // 16)
        assert R.senet_bwd_lds(64, 64, nvec, 1) > 64 * 1024
    assert {c[3] for c in R.SENET_FUSED_CASES if c[0] is F32 and not R.pow2(c[3])} == {12, 24}
    assert {c[3] for c in R.SENET_FUSED_CASES if c[0] is BF16 and not R.pow2(c[3])} == {24, 48}


def test_senet_slab_counts_and_second_samples():
    for dtype in R.DTYPES:
        cases = [c for c in R.SENET_SLAB_CASES if c[0] is dtype]
        assert all(R.senet_bwd_waves(*c[1:4], dtype) == 4 for c in cases)
        slabs = [R.senet_slabs(c[4], *c[1:4], dtype) for c in cases]
        assert slabs == [1, 1, 2, 7, 8, 9, 17]
        # per = ceil(nslab / 8): segments past the slabs are empty, the last used one is short
        assert any(s % R.SENET_FIN_SEG and s > R.SENET_FIN_SEG for s in slabs) and any(s < R.SENET_FIN_SEG for s in slabs)
    for c in R.SENET_TRIP_CASES:
        B = c[4]
        assert B > R.CUS * R.FWD_BLOCKS_PER_CU * 4            # forward: at most 8 x 256 resident workgroups of 4 waves
        assert B > R.SENET_MAX_BLOCKS * 4                     # backward: at most 1024 workgroups of at most 4 waves


@pytest.mark.parametrize("case", R.SENET_FUSED_CASES + R.SENET_PARTIAL_CASES, ids=R.senet_id)
def test_senet_fused_operands_are_exact_and_not_degenerate(case):
    o = R.senet_case(*case)
    assert R.senet_check(o) == []
    worst = R.senet_guard(o)
    print(f"senet guard {R.senet_id(case)}: draw {o.salt}, largest sum of |terms| {worst:.0f} quanta")
    for t in (o.W1 / (1 if R.pow2(o.E) else o.E), o.W2, o.b1, o.b2):
        assert float(t.abs().max()) <= 1 and torch.equal(t, t.round())


@pytest.mark.parametrize("case", R.SENET_ROW_CASES, ids=R.senet_row_id)
def test_senet_row_operands_are_exact(case):
    o = R.senet_row_case(*case)
    worst = R.senet_row_guard(o)
    print(f"senet rows {R.senet_row_id(case)}: largest sum of |terms| {worst:.0f}")
    assert bool((o.a == 0).any()) and bool((o.a > 0).any()) and bool((o.ga != 0).any())


def test_senet_row_cases_reach_every_group_width():
    assert {R.senet_row_path(E, F32)[2] for E in R.SENET_ROW_VECTOR_E} == set(range(7))
    assert all(R.senet_row_path(E, F32)[0] for E in R.SENET_ROW_VECTOR_E)
    assert not any(R.senet_row_path(E, F32)[0] for E in R.SENET_ROW_ELEMENT_E)
    assert R.senet_row_path(16, F32, aligned=False) == (False, 16, 4)
    dtype, E, B, M, _ = R.SENET_ROWS_TRIP
    lg = R.senet_row_path(E, dtype)[2]
    assert (B * M) << lg > R.STREAM_GRID_CAP * 256 and B * M * (E // 4) > R.STREAM_GRID_CAP * 256
    assert R.senet_row_trips(B * M, E, dtype) == (2, 2)


@pytest.mark.parametrize("case", R.SENET_LAYER_CASES, ids=R.senet_layer_id)
def test_senet_layer_operands_are_exact(case):
    o = R.senet_layer_case(*case)
    assert o.M > R.SENET_MAX_M and o.H == case[1] // case[2]
    if o.H:
        R.senet_guard(o)
    else:
        r = R.senet_ref(o)
        assert bool((r.out != 0).any()) and bool((r.db2 != 0).any())


def test_the_guard_refuses_what_is_not_exact():
    o = R.senet_case(F32, 13, 3, 32, 33)
    bad = R.NS(**vars(o))
    bad.x = o.x + 1.0 / 3
    with pytest.raises(AssertionError):
        R.senet_guard(bad)
    bad = R.NS(**vars(o))
    bad.x = o.x * 2.0 ** 22
    with pytest.raises(AssertionError):
        R.senet_guard(bad)


# ---------------------------------------------------------------------------------------------------------------------
# ranking losses
# ---------------------------------------------------------------------------------------------------------------------
def test_rank_sizes_reach_the_second_trips():
    assert R.rank_partials(16384) == 64 and R.rank_finish_trips(16384) == 1
    assert R.rank_partials(16385) == 65 and R.rank_finish_trips(16385) == 2
    assert R.rank_partial_trips(65536) == 1 and R.rank_partial_trips(65537) == 2
    Bs = {B for B, _ in R.RANK_SIZES}
    assert {16384, 16385, 65536, 65537} <= Bs and {R.rank_partials(B) for B in Bs} >= {1, 2, 64, 65, 256}
    assert {B for B, _ in R.RANK_POW2_SIZES} >= {16385, 65537}


@pytest.mark.parametrize("case", R.RANK_SIZES + R.RANK_POW2_SIZES, ids=R.rank_id)
def test_rank_operands_are_exact(case):
    B, K = case
    s = R.rank_scores(B, K)
    assert torch.equal(s.to(BF16).to(F64), s) and torch.equal(s * 4, (s * 4).round()) and float(s.abs().max()) <= 4
    for kind in R.RANK_EXACT_KINDS:
        zero = {m: int((R.rank_hinge_args(s, kind, m) == 0).sum()) for m in R.RANK_MARGINS}
        assert zero[0.625] == 0 and zero[1.0] >= 1, (kind, zero)
        if B >= 255:
            assert zero[1.0] >= B // 100, (kind, zero)
        for m in R.RANK_MARGINS:
            assert R.rank_term_quanta(s, kind, m) < 2 ** 24
    if K > 1:
        assert bool(R.rank_tied_first(s)[0])
    # the derivative of clamp at exactly 0 is 1: sample 0 at margin 1.0 takes its gradient
    r = R.rank_ref(s, "hinge", 1.0, None, "sum")
    assert r.grad[0].tolist() == [-float(K)] + [1.0] * K
    r = R.rank_ref(s, "adaptive_hinge", 1.0, None, "sum")
    assert r.grad[0].tolist() == [-1.0, 1.0] + [0.0] * (K - 1)


def test_rank_masks():
    for B, _ in R.RANK_SIZES:
        assert R.rank_mask(B, "none") is None and bool(R.rank_mask(B, "all").all())
        assert int(R.rank_mask(B, "last_only").sum()) == 1 and bool(R.rank_mask(B, "last_only")[-1])
        m = R.rank_mask(B, "drop_block")
        if B > 2 * R.RANK_BLOCK:
            assert not bool(m[256:512].any()) and int(m.sum()) == B - 256
    for B, _ in R.RANK_POW2_SIZES:
        for j in (1, 3, 8):
            m = R.rank_pow2_mask(B, j)
            assert int(m.sum()) == 1 << j and bool(m[0]) and bool(m[-1])

"""Host checks of tests/cin_glue_ref.py: the exactness guard over EVERY case tests/test_gpu_cin_glue_exact.py runs, the
restated dispatch arithmetic against the text of csrc/cin_glue.hip, the coverage conditions the case lists exist for, and
the float64 references against autograd through the plain formula."""
import pytest
import torch

import cin_glue_ref as R

F64 = R.F64


# ---------------------------------------------------------------------------------------------------------------------
# the guard
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_every_case_is_exact_in_fp32(case):
    """every pattern the GPU file runs on the case; about one pre-activation in twenty is exactly zero"""
    o = R.glue_case(*case)
    for pattern in R.case_patterns(case):
        f = R.assert_exact_domain(o, pattern)
        assert f.worst < 2 ** 24
    assert f.zeros > 0
    if f.values >= 4096:
        assert 0.02 <= f.zero_fraction <= 0.12, f.zero_fraction


@pytest.mark.parametrize("case", R.E2E_NOBN_CASES, ids=R.case_id)
def test_identity_statistics_cases_are_exact(case):
    R.assert_exact_domain(R.identity_operands(*case), "both", both_signs=False)


@pytest.mark.parametrize("case", R.E2E_BN_CASES, ids=R.case_id)
def test_batchnorm_cases_are_exact(case):
    o = R.bn_operands(*case)
    R.assert_bn_exact(o)
    R_ = o.B * o.E
    assert R_ & (R_ - 1) == 0
    # both sides of ReLU occur under a negative and under a positive weight, and some gradients are not zero
    r = R.bwd_ref(o, "both")
    assert bool((r.sums[0] != 0).any()) and bool((r.sums[1] != 0).any()) and bool((o.c1 != 0).any()) and bool((o.c2 != 0).any())


def test_the_guard_refuses_what_is_not_exact():
    o = R.operands(3, 5, 16, 8, 8)
    R.assert_exact_domain(o)
    bad = R.NS(**vars(o))
    bad.scale = o.scale.clone()
    bad.scale[3] = 1.0 / 3
    with pytest.raises(AssertionError):
        R.assert_exact_domain(bad)
    bad = R.NS(**vars(o))
    bad.y = o.y * 2.0 ** 22                                                   # sums of magnitudes past 2**24
    with pytest.raises(AssertionError):
        R.assert_exact_domain(bad)
    bad = R.NS(**vars(o))
    bad.y = o.y + 1.0 / 512                                                   # not a bf16 value
    with pytest.raises(AssertionError):
        R.assert_exact_domain(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the references are the plain formula
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 5, 16, 8, 8), (2, 4, 32, 24, 8), (2, 3, 24 + 8, 8, 24)], ids=R.case_id)
def test_backward_reference_is_autograd_of_batchnorm(case):
    """With c1 = dbeta / R and c2 = dgamma / R the closed form is the gradient of relu(batch_norm(y)) in training mode: on
    random real operands against float64 autograd.  Sums of R <= 15 terms, each off by 2**-53 relative."""
    B, E, C, D, Hs = case
    g = R.gen(74, *case)
    y = torch.randn(B, E, C, generator=g, dtype=F64)
    gamma, beta = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    gh, gp = torch.randn(B, E, C - Hs, generator=g, dtype=F64), torch.randn(B, D, generator=g, dtype=F64)
    ya, ga, ba = y.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    z = torch.relu(torch.nn.functional.batch_norm(ya.reshape(B * E, C), None, None, ga, ba, True, 0.0, 1e-5)).view(B, E, C)
    ((z[..., Hs:] * gh).sum() + (z[..., :D].sum(1) * gp).sum()).backward()
    rows = y.reshape(B * E, C)
    mean, var = rows.mean(0), rows.var(0, unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    o = R.NS(B=B, E=E, C=C, D=D, Hs=Hs, y=y, scale=gamma * invstd, shift=beta - mean * gamma * invstd, mean=mean,
             invstd=invstd, c1=torch.zeros(C, dtype=F64), c2=torch.zeros(C, dtype=F64), g_hidden=gh, g_pooled=gp)
    f = R.fwd_ref(o)
    assert torch.allclose(f.z, z.detach(), rtol=1e-12, atol=1e-12)
    sums = R.bwd_ref(o, "both").sums
    o.c1, o.c2 = sums[0] / (B * E), sums[1] / (B * E)
    r = R.bwd_ref(o, "both")
    dead = R.dead_channels(C, D, Hs, "both")
    assert torch.allclose(r.sums[0], ba.grad, rtol=1e-11, atol=1e-11) and torch.allclose(r.sums[1], ga.grad, rtol=1e-11, atol=1e-11)
    assert torch.allclose(r.gy, ya.grad, rtol=1e-10, atol=1e-10)
    assert float(ya.grad[..., dead].abs().max() if dead.any() else 0.0) == 0.0


def test_absent_gradients_are_zero_gradients():
    o = R.operands(3, 5, 32, 24, 8)
    for pattern, zh, zp in (("no_hidden", True, False), ("no_pooled", False, True), ("none", True, True)):
        z = R.NS(**vars(o))
        z.g_hidden = o.g_hidden * (0.0 if zh else 1.0)
        z.g_pooled = o.g_pooled * (0.0 if zp else 1.0)
        a, b = R.bwd_ref(o, pattern), R.bwd_ref(z, "both")
        live = ~R.dead_channels(o.C, o.D, o.Hs, pattern)
        assert torch.equal(a.sums, b.sums) and torch.equal(a.gy[..., live], b.gy[..., live])
        assert float(a.gy[..., ~live].abs().max() if (~live).any() else 0.0) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch arithmetic and what the case lists cover
# ---------------------------------------------------------------------------------------------------------------------
def test_restated_arithmetic_is_the_source_text():
    for line, n in R.source_sites():
        assert n == 1, (line, n)


def test_legal_shapes():
    assert R.LEGAL_C == [8, 16, 32, 64, 128, 256, 512, 1024, 2048]
    assert [C for C in range(0, 4100, 4) if R.glue_shape_ok(C, 0, 0)] == R.LEGAL_C
    assert not R.glue_shape_ok(64, 4, 0) and not R.glue_shape_ok(64, 72, 0) and not R.glue_shape_ok(64, 0, 72)
    # channels-first: one E per legal C, nothing else (C = 24 has E = 8 * (256 / 3) = 680: not a legal C)
    assert [(E, C) for C in range(0, 4100, 4) for E in range(0, 2100, 4) if C and R.glue_cf_ok(C, E)] == sorted(R.CF_SHAPES, key=lambda s: s[1])
    assert R.CF_SHAPES[5] == (64, 256) and R.CF_SHAPES[6] == (32, 512) and not R.glue_cf_ok(24, 680) and not R.glue_cf_ok(0, 8)
    for case in R.ALL_CASES + R.E2E_NOBN_CASES + R.E2E_BN_CASES:
        B, E, C, D, Hs = case
        assert R.glue_shape_ok(C, D, Hs) and B > 0 and E > 0, case


def test_lds_of_the_channels_first_launches():
    """the block reduction needs rpp * C * 4 = 8 KiB at every C; the largest request is the forward at C = 2048, E = 8,
    Hs = 0: 8 KiB + 64 KiB, inside the 160 KiB of a workgroup"""
    for C in R.LEGAL_C:
        assert R.rpp(C) * C * 4 == R.PLAIN_LDS == 8192
    most = 0
    for (B, E, C, D, Hs) in R.CF_CASES:
        most = max(most, R.fwd_cf_lds(C, E, Hs), R.bwd_cf_lds(C, E))
        assert R.bwd_cf_lds(C, E) == C * (E + 8) * 2 >= R.PLAIN_LDS
    assert most == R.fwd_cf_lds(2048, 8, 0) == 8 * 1024 + 64 * 1024 <= R.LDS_MOST
    assert (3, 8, 2048, 0, 0) in R.CF_CASES


def test_thread_layouts_are_covered():
    plain = R.PLAIN_CASES
    assert {c[2] for c in plain} == set(R.LEGAL_C)
    assert any(R.rpp(C) > E for (_, E, C, _, _) in plain)
    assert any(E > R.rpp(C) and E % R.rpp(C) for (_, E, C, _, _) in plain)
    assert any(E > R.rpp(C) and E % R.rpp(C) == 0 for (_, E, C, _, _) in plain)
    assert any(R.rpp(C) == 1 for (_, _, C, _, _) in plain)
    assert any(R.rpp(C) == 1 for (_, _, C, _, _) in R.CF_CASES) and any(R.rpp(C) == 256 for (_, _, C, _, _) in R.CF_CASES)


def test_grid_stride_is_covered():
    """B = 1025: workgroup 0 takes a second sample; B > 2048: a third.  For the plain kernels and for both channels-first
    kernels (every channels-first case runs the forward and the backward one)"""
    for cases in (R.PLAIN_CASES, R.CF_CASES):
        bs = {c[0] for c in cases}
        assert 1025 in bs and any(b > 2048 for b in bs)
        assert all(R.glue_grid(b) == min(b, 1024) for b in bs)
    assert R.glue_grid(1025) == 1024 and -(-2049 // R.glue_grid(2049)) == 3
    assert any(c[0] > 1024 for c in R.STATS_PAIR_CASES) and (5, 741, 8, 0, 0) in R.STATS_PAIR_CASES
    assert all(c[0] > 1024 for c in R.E2E_NOBN_CASES)
    assert [R.glue_cf_ok(c[2], c[1]) for c in R.E2E_NOBN_CASES] == [True, False]
    assert [R.glue_cf_ok(c[2], c[1]) for c in R.E2E_BN_CASES] == [True, False]


def test_split_kinds_are_covered():
    kinds = ("halves", "all_both", "direct_only", "hidden_only", "overlap", "gap")
    assert {R.split_kind(C, D, Hs) for (_, _, C, D, Hs) in R.PLAIN_CASES} == set(kinds)
    assert {R.split_kind(C, D, Hs) for (_, _, C, D, Hs) in R.CF_CASES} >= {"halves", "all_both", "overlap", "gap", "hidden_only"}
    assert R.split_kind(64, 32, 32) == "halves" and R.split_kind(64, 64, 0) == "all_both" and R.split_kind(64, 64, 64) == "direct_only"
    assert R.split_kind(64, 0, 0) == "hidden_only" and R.split_kind(64, 40, 24) == "overlap" and R.split_kind(64, 16, 40) == "gap"
    # every gradient-presence pattern leaves dead channels somewhere and live ones somewhere
    for pattern in R.PATTERNS:
        assert pattern in R.case_patterns(R.LAYOUT_CASES[0])
    assert any(bool(R.dead_channels(C, D, Hs, "both").any()) for (_, _, C, D, Hs) in R.PLAIN_CASES + R.CF_CASES)
    assert bool(R.dead_channels(64, 16, 40, "both")[16:40].all()) and int(R.dead_channels(64, 16, 40, "both").sum()) == 24
    assert bool(R.dead_channels(64, 32, 32, "none").all())


def test_channels_first_shapes_are_covered():
    """every (E, C) the channels-first entries take, with Hs in {0, 8, C / 2} wherever that is a multiple of 8 (C = 8 has
    0 and 8 = C, C = 16 has 0 and 8 = C / 2)"""
    have = {(E, C, Hs) for (_, E, C, _, Hs) in R.CF_CASES}
    for C in R.LEGAL_C:
        E = 8 * R.rpp(C)
        assert R.glue_cf_ok(C, E)
        for Hs in (0, 8, C // 2):
            if Hs % 8 == 0:
                assert (E, C, Hs) in have, (E, C, Hs)
    assert len(R.CF_SMALL_CASES) == 2 + 2 + 3 * 7

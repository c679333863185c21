"""The six kernels of csrc/cin_glue.hip behind the seven ``trs_cin_glue_*`` entries against float64 references BIT FOR BIT,
at every thread layout (all nine C, rpp above / below / beside E, rpp = 1), on second and third passes of the grid-stride
loop, at all six ways the pooled and the passed-on channels can lie, under every gradient-presence pattern and at every
channels-first shape (tests/cin_glue_ref.py: operands for which every fp32 product and sum is exact; the guard, the
restated dispatch arithmetic and the coverage conditions are checked on the CPU by tests/test_cin_glue_host.py over the
same lists).

The raw entries are called through ``call`` / ``size_query``.  Every output buffer is filled with NaN first, so an element
that is never written shows; in channels no gradient reaches, ``y`` itself is NaN for the two backward entries (the code
documents that it is not read there) and the outputs must be exact zeros.  Every comparison is ``torch.equal`` with the
float64 value rounded once; a failure names the entry, the tensor, the number of differing elements and the first differing
index.  The one tolerance of the file is 1e-6 on ``running_var``, whose unbiased factor R / (R - 1) is not dyadic.
profiles/cin_glue_exact_cases.md maps the case groups to the kernels and seams."""
import pytest
import torch

import cin_glue_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu

BF16, F32, F64 = R.BF16, R.F32, R.F64
OK, EINVAL, EDTYPE, ESHAPE, EALIGN = 0, -1, -2, -3, -4                  # include/trs_abi.h
ENTRIES = ("trs_cin_glue_stats", "trs_cin_glue_fwd", "trs_cin_glue_fwd_cf", "trs_cin_glue_bwd_reduce",
           "trs_cin_glue_bwd_apply", "trs_cin_glue_bwd_apply_cf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Diffs(list):
    def check(self, where, name, got, ref):
        want = ref if got.dtype == F64 else R.expect(ref, got.dtype)
        if got.shape == want.shape and torch.equal(got, want.to(got.device)):
            return
        self.append(R.mismatch(f"{where} {name}", got, want))

    def done(self):
        assert not self, "\n".join(self)


def _nan(dev, dtype, *shape):
    """an output buffer no kernel has written yet; None for an empty one (the entries take NULL there)"""
    return torch.full(shape, float("nan"), dtype=dtype, device=dev) if all(shape) else None


def _args(name, t, B, E, C, D, Hs, dtype=1):
    """the argument list of an entry from the buffers of ``t`` (dtype 1: TRS_BF16)"""
    from torecsys_amd._abi import ptr, stream_ptr
    p, s = (lambda k: ptr(getattr(t, k, None))), stream_ptr()
    stat = [p("scale"), p("shift"), p("mean"), p("invstd")]
    grads = [p("y"), p("g_hidden"), p("g_pooled")]
    return {
        "trs_cin_glue_stats": lambda: [p("y"), B, E, C, dtype, p("partial"), s],
        "trs_cin_glue_fwd": lambda: [p("y"), p("scale"), p("shift"), B, E, C, D, Hs, dtype, p("hidden"), p("pooled"), s],
        "trs_cin_glue_fwd_cf": lambda: [p("y"), p("scale"), p("shift"), B, E, C, D, Hs, dtype, p("hidden"), p("hidden_cf"),
                                        p("pooled"), s],
        "trs_cin_glue_bwd_reduce": lambda: grads + stat + [B, E, C, D, Hs, dtype, p("partial"), s],
        "trs_cin_glue_bwd_apply": lambda: grads + stat + [p("c1"), p("c2"), B, E, C, D, Hs, dtype, p("gy"), s],
        "trs_cin_glue_bwd_apply_cf": lambda: grads + stat + [p("c1"), p("c2"), B, E, C, D, Hs, dtype, p("gy"), p("gy_cf"),
                                                             p("colsum"), s],
    }[name]()


def _call(name, t, o, **kw):
    from torecsys_amd._abi import call
    call(name, *_args(name, t, o.B, o.E, o.C, o.D, o.Hs, **kw))


def _vectors(o):
    f32 = lambda v: v.to(F32).contiguous()                                  # noqa: E731
    return R.NS(scale=f32(o.scale), shift=f32(o.shift), mean=f32(o.mean), invstd=f32(o.invstd), c1=f32(o.c1), c2=f32(o.c2))


def _blocks(B):
    from torecsys_amd._abi import size_query
    n = size_query("trs_cin_glue_blocks", B)
    assert n == R.glue_grid(B)
    return n


def _cf(E, C):
    from torecsys_amd._abi import size_query
    cf = bool(size_query("trs_cin_glue_cf_supported", E, C))
    assert cf == R.glue_cf_ok(C, E)
    return cf


def _run_stats(d, dev, o, where):
    t = R.NS(y=o.y.to(BF16).contiguous(), partial=_nan(dev, F32, _blocks(o.B), 2, o.C))
    _call("trs_cin_glue_stats", t, o)
    d.check(where, "stats: summed partial", t.partial.double().sum(0), R.stats_ref(o.y))


def _run_forward(d, dev, o, where, cf):
    B, E, C, D, Hs = o.B, o.E, o.C, o.D, o.Hs
    f = R.fwd_ref(o)
    for name in ("trs_cin_glue_fwd",) + (("trs_cin_glue_fwd_cf",) if cf else ()):
        t = _vectors(o)
        t.y, t.hidden, t.pooled = o.y.to(BF16).contiguous(), _nan(dev, BF16, B, E, C - Hs), _nan(dev, BF16, B, D)
        t.hidden_cf = _nan(dev, BF16, B, C - Hs, E)
        _call(name, t, o)
        tag = f"{where} {name[13:]}:"
        if t.hidden is not None:
            d.check(tag, "hidden", t.hidden, f.hidden)
            if name.endswith("_cf"):
                d.check(tag, "hidden_cf", t.hidden_cf, f.hidden.transpose(1, 2))
        if t.pooled is not None:
            d.check(tag, "pooled", t.pooled, f.pooled)


def _run_backward(d, dev, o, where, cf, pattern):
    B, E, C, D, Hs = o.B, o.E, o.C, o.D, o.Hs
    r = R.bwd_ref(o, pattern)
    dead = R.dead_channels(C, D, Hs, pattern).to(dev)
    nblk = _blocks(B)
    t = _vectors(o)
    y = o.y.clone()
    y[..., dead] = float("nan")                                             # not read where no gradient arrives
    t.y = y.to(BF16).contiguous()
    some = lambda v, on: v.to(BF16).contiguous() if on and v.numel() else None      # noqa: E731
    t.g_hidden = some(o.g_hidden, pattern in ("both", "no_pooled"))
    t.g_pooled = some(o.g_pooled, pattern in ("both", "no_hidden"))
    tag = f"{where} [{pattern}]"
    t.partial = _nan(dev, F32, nblk, 2, C)
    _call("trs_cin_glue_bwd_reduce", t, o)
    d.check(f"{tag} bwd_reduce:", "summed partial (dbeta, dgamma)", t.partial.double().sum(0), r.sums)
    t.gy = _nan(dev, BF16, B, E, C)
    _call("trs_cin_glue_bwd_apply", t, o)
    d.check(f"{tag} bwd_apply:", "gy", t.gy, r.gy)
    if dead.any():
        d.check(f"{tag} bwd_apply:", "gy in the channels without a gradient", t.gy[..., dead], torch.zeros_like(r.gy[..., dead]))
    if not cf:
        return
    for with_colsum in (True, False):
        t.gy, t.gy_cf = _nan(dev, BF16, B, E, C), _nan(dev, BF16, B, C, E)
        t.colsum = _nan(dev, F32, nblk, C) if with_colsum else None
        _call("trs_cin_glue_bwd_apply_cf", t, o)
        e = f"{tag} bwd_apply_cf{'' if with_colsum else ' (colsum_partial NULL)'}:"
        d.check(e, "gy", t.gy, r.gy)
        d.check(e, "gy_cf", t.gy_cf, r.gy.transpose(1, 2))
        if with_colsum:
            d.check(e, "summed colsum_partial", t.colsum.double().sum(0), r.colsum)


def _run_case(dev, case, entries="all"):
    B, E, C, D, Hs = case
    o = R.to_device(R.glue_case(*case), dev)
    cf = _cf(E, C)
    where = f"cin_glue {R.case_id(case)} [rpp {R.rpp(C)}, {R.split_kind(C, D, Hs)}, {-(-B // R.glue_grid(B))} passes]"
    d = Diffs()
    _run_stats(d, dev, o, where)
    if entries == "all":
        _run_forward(d, dev, o, where, cf)
        for pattern in R.case_patterns(case):
            _run_backward(d, dev, o, where, cf, pattern)
    torch.cuda.synchronize()
    d.done()
    return cf


@pytest.mark.parametrize("case", R.LAYOUT_CASES, ids=R.case_id)
def test_thread_layouts_and_splits_exact(dev, case):
    """all nine C; rpp = 256 / (C / 8) above E (idle row groups feed zeros to the block reduction), E one or a few rows
    past a multiple of rpp, E a multiple, rpp = 1; the six split kinds, among them a gap whose channels are neither pooled
    nor passed on (C = 8: every channel) and direct-only / hidden-only, where one output tensor does not exist; all four
    gradient-presence patterns, y NaN wherever no gradient arrives"""
    assert not _run_case(dev, case)


@pytest.mark.parametrize("case", R.STRIDE_CASES, ids=R.case_id)
def test_grid_stride_passes_exact(dev, case):
    """min(B, 1024) workgroups: B = 1025 gives workgroup 0 a second sample, B > 2048 a third; the block reduction's LDS is
    re-used behind its barriers, the pooled accumulators start again, the backward sums carry on"""
    assert not _run_case(dev, case)


@pytest.mark.parametrize("case", R.STATS_PAIR_CASES, ids=R.case_id)
def test_stats_as_the_column_sum_of_a_pair_gradient_exact(dev, case):
    """functional._pair_bias_grad hands (B, P, E) to trs_cin_glue_stats as (B, E = P, C = E): 741 pairs are no multiple of
    anything, and a batch above the grid cap"""
    _run_case(dev, case, entries="stats")


@pytest.mark.parametrize("case", R.CF_SMALL_CASES, ids=R.case_id)
def test_channels_first_shapes_exact(dev, case):
    """every (E, C) trs_cin_glue_cf_supported accepts, Hs in {0, 8, C / 2}: the XOR swizzle of the LDS tile depends on rpp,
    on Hs and on E / 8.  Both plain entries run on the same operands; the backward also with colsum_partial NULL"""
    assert _run_case(dev, case)


@pytest.mark.parametrize("case", R.CF_STRIDE_CASES, ids=R.case_id)
def test_channels_first_grid_stride_passes_exact(dev, case):
    """the second and third pass of the two channels-first kernels re-use the LDS tile behind barriers; the column sums
    of gy run over all of a workgroup's samples"""
    assert _run_case(dev, case)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: an error code, never a launch
# ---------------------------------------------------------------------------------------------------------------------
def _refusal_buffers(dev, elems):
    """every buffer of every entry, ``elems`` values each, outputs NaN"""
    t = R.NS()
    for k in ("y", "g_hidden", "g_pooled"):
        setattr(t, k, torch.ones(elems, dtype=BF16, device=dev))
    for k in ("scale", "shift", "mean", "invstd", "c1", "c2"):
        setattr(t, k, torch.ones(elems, dtype=F32, device=dev))
    for k in ("hidden", "hidden_cf", "pooled", "gy", "gy_cf"):
        setattr(t, k, _nan(dev, BF16, elems))
    for k in ("partial", "colsum"):
        setattr(t, k, _nan(dev, F32, elems))
    return t


def _untouched(t):
    torch.cuda.synchronize()
    return all(bool(getattr(t, k).isnan().all()) for k in ("hidden", "hidden_cf", "pooled", "gy", "gy_cf", "partial", "colsum"))


def test_refusals(dev):
    """C = 24 and C = 4096 (not 8 x a divisor of 256), D = 4, D > C, fp32, a channels-first entry on another shape, a
    pointer two bytes off: the code the header names, nothing written.  B = 0: OK, nothing written"""
    from torecsys_amd._abi import load, size_query
    lib = load()
    rc = lambda name, t, *a, **kw: getattr(lib, name)(*_args(name, t, *a, **kw))         # noqa: E731
    t = _refusal_buffers(dev, 2 * 64 * 4096)
    cf_shape, plain = (64, 256), (16, 256)
    for name in ENTRIES:
        E, C = cf_shape if name.endswith("_cf") else plain
        assert rc(name, t, 2, E, 24, 8, 8) == ESHAPE, name
        assert rc(name, t, 2, E, 4096, 8, 8) == ESHAPE, name
        assert rc(name, t, 2, E, C, 128, 128, dtype=0) == EDTYPE, name
        assert rc(name, t, -1, E, C, 128, 128) == EINVAL, name
        assert rc(name, t, 0, E, C, 128, 128) == OK, name
        if name != "trs_cin_glue_stats":                                    # it has no split
            assert rc(name, t, 2, E, C, 4, 128) == ESHAPE, name
            assert rc(name, t, 2, E, C, C + 8, 128) == ESHAPE, name
            assert rc(name, t, 2, E, C, 128, C + 8) == ESHAPE, name
        if name.endswith("_cf"):
            assert rc(name, t, 2, plain[0], plain[1], 128, 128) == ESHAPE, name
            assert rc(name, t, 0, plain[0], plain[1], 128, 128) == ESHAPE, name
        off = R.NS(**vars(t))
        off.y = t.y[1:]
        assert off.y.data_ptr() % 16 == 2
        assert rc(name, off, 2, E, C, 128, 128) == EALIGN, name
    for name, out in (("trs_cin_glue_fwd", "hidden"), ("trs_cin_glue_fwd_cf", "hidden_cf"), ("trs_cin_glue_bwd_apply", "gy"),
                      ("trs_cin_glue_bwd_apply_cf", "gy_cf"), ("trs_cin_glue_bwd_reduce", "g_pooled")):
        E, C = cf_shape if name.endswith("_cf") else plain
        off = R.NS(**vars(t))
        setattr(off, out, getattr(t, out)[1:])
        assert rc(name, off, 2, E, C, 128, 128) == EALIGN, (name, out)
    null = R.NS(**vars(t))
    null.scale = None
    for name in ENTRIES[1:]:
        E, C = cf_shape if name.endswith("_cf") else plain
        assert rc(name, null, 2, E, C, 128, 128) == EINVAL, name
    assert _untouched(t)
    # what the entries take is what the query reports: one E per legal C; C = 24 would have E = 8 * (256 / 3) = 680
    for C in list(range(0, 72, 4)) + R.LEGAL_C + [4096]:
        for E in (0, 8, 64, 680, 8 * (256 // max(C // 8, 1))):
            assert bool(size_query("trs_cin_glue_cf_supported", E, C)) == R.glue_cf_ok(C, E), (E, C)
    assert size_query("trs_cin_glue_blocks", 0) == 0


# ---------------------------------------------------------------------------------------------------------------------
# F_.cin_glue end to end, where the Python finishing is exact as well
# ---------------------------------------------------------------------------------------------------------------------
def _glue_end_to_end(dev, o, bn, where):
    """forward and backward of F_.cin_glue on the case: hidden, pooled, the input gradient, and at a channels-first shape
    the copies that ride on the tensors and the column sums of the gradient.  -> (Diffs, reference of the backward)"""
    from torecsys_amd import functional as F_
    B, E, C, D, Hs = o.B, o.E, o.C, o.D, o.Hs
    d = Diffs()
    cf = _cf(E, C)
    ya = o.y.to(BF16).contiguous().requires_grad_()
    assert F_.cin_glue_supported(ya, D, Hs)
    hidden, pooled = F_.cin_glue(ya, bn, D, Hs)
    f = R.fwd_ref(o)
    d.check(where, "hidden", hidden, f.hidden)
    d.check(where, "pooled", pooled, f.pooled)
    if cf:
        d.check(where, "hidden._trs_cf", hidden._trs_cf, f.hidden.transpose(1, 2))
    else:
        assert getattr(hidden, "_trs_cf", None) is None
    seen = []
    ya.register_hook(lambda g_: seen.append((getattr(g_, "_trs_cf", None), getattr(g_, "_trs_colsum", None))))
    torch.autograd.backward([hidden, pooled], [o.g_hidden.to(BF16).contiguous(), o.g_pooled.to(BF16).contiguous()])
    torch.cuda.synchronize()
    r = R.bwd_ref(o, "both")
    d.check(where, "y.grad", ya.grad, r.gy)
    gy_cf, colsum = seen[0]
    if cf:
        assert gy_cf is not None and colsum is not None, "the channels-first copy / column sums did not ride on the gradient"
        d.check(where, "y.grad._trs_cf", gy_cf, r.gy.transpose(1, 2))
        d.check(where, "summed y.grad._trs_colsum", colsum[0].double().sum(0), r.colsum)
    else:
        assert gy_cf is None and colsum is None
    return d, r


@pytest.mark.parametrize("case", R.E2E_NOBN_CASES, ids=R.case_id)
def test_cin_glue_without_batchnorm_exact(dev, case):
    """bn=None: identity statistics, integer operands, B > 1024, at a channels-first shape and at another"""
    o = R.to_device(R.identity_operands(*case), dev)
    d, _ = _glue_end_to_end(dev, o, None, f"F_.cin_glue(bn=None) {R.case_id(case)}:")
    d.done()


@pytest.mark.parametrize("variant", ["momentum_0.5", "cumulative_average", "no_running_stats"])
@pytest.mark.parametrize("case", R.E2E_BN_CASES, ids=R.case_id)
def test_cin_glue_training_batchnorm_exact(dev, case, variant):
    """BatchNorm1d(C, eps=0) in training mode on channels that take mu_c +- 1 half and half over R = 2**k rows: mean,
    variance 1, invstd, c1 and c2 are exact, so outputs, the input gradient, the weight and bias gradients (some weights
    negative) and running_mean are held bit for bit; running_var = (1 - m) v0 + m R / (R - 1) to 1e-6"""
    o = R.to_device(R.bn_operands(*case), dev)
    Rows, C = o.B * o.E, o.C
    track = variant != "no_running_stats"
    momentum = 0.5 if variant != "cumulative_average" else None
    bn = torch.nn.BatchNorm1d(C, eps=0.0, momentum=momentum, track_running_stats=track).to(dev)
    with torch.no_grad():
        bn.weight.copy_(o.weight)
        bn.bias.copy_(o.bias)
        if track:
            bn.running_mean.copy_(o.running_mean0)
            bn.running_var.copy_(o.running_var0)
    bn.train()
    d, r = _glue_end_to_end(dev, o, bn, f"F_.cin_glue(BatchNorm1d {variant}) {R.case_id(case)}:")
    d.check("BatchNorm1d", "weight.grad", bn.weight.grad, r.sums[1])
    d.check("BatchNorm1d", "bias.grad", bn.bias.grad, r.sums[0])
    assert bool((o.weight < 0).any()) and bool((r.sums[1] != 0).any())
    if track:
        m = 0.5 if momentum is not None else 1.0                           # first step of a cumulative average: 1 / 1
        d.check("BatchNorm1d", "running_mean", bn.running_mean, (1.0 - m) * o.running_mean0 + m * o.mean)
        want_var = (1.0 - m) * o.running_var0 + m * (Rows / (Rows - 1.0))
        err = rel_err(bn.running_var.cpu(), want_var.cpu())
        assert err <= 1e-6, f"running_var: rel_err {err}"
        assert int(bn.num_batches_tracked) == 1
    else:
        assert bn.running_mean is None and bn.running_var is None
    d.done()

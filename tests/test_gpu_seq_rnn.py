"""GPU parity of SequenceIndicesEmbedding and functional.seq_rnn* (csrc/seq_rnn.hip): against the reference's own outputs
and gradients (tests/golden/seq_rnn.npz, seq_rnn_e64.npz) and, at sizes the fixture does not hold, against the plain torch
restatement run on the CPU in fp64 on the SAME dtype-rounded operands (tests/seq_rnn_ref.py, pinned to the fixture by
tests/test_seq_rnn_host.py) -- never against the ATen composition on the device.  Tolerances are the project's own: fp32
1e-5, bf16 1e-2, in conftest.rel_err_both (max norm and per-row norm) for the output and the table gradient, in the max
norm for the four RNN parameter gradients.  The bf16 bound rests on fp32 arithmetic between loads and stores with one
rounding of h per step (a CPU emulation of exactly that gave 1.1e-3 to 6.3e-3 over the three cells); figures seen on an
MI355X are in profiles/seq_rnn_kernels.md."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import rel_err, rel_err_both
from seq_rnn_ref import (CELLS, GOLDEN_CASES, GOLDEN_SHAPES, GPU_SHAPES, PARAM_KEYS, golden_file, make_ids, make_params,
                         seq_rnn_grads, seq_rnn_steps, shape_tag)

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
DTYPES = [torch.float32, torch.bfloat16]
FWD, BWD = "trs_seq_rnn_fwd", "trs_seq_rnn_bwd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("out", "g_table", "g_w_ih", "g_w_hh", "g_b_ih", "g_b_hh")


def _dt(d):
    return "fp32" if d == torch.float32 else "bf16"


def _id(v):
    return shape_tag(v) if isinstance(v, tuple) else (_dt(v) if isinstance(v, torch.dtype) else str(v))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def fused_path(monkeypatch):
    """the tests of this file are about the kernels: they take the fused path whatever the package default is (the
    composition is tested in a process of its own with TRS_SEQ_RNN=0)"""
    from torecsys_amd import inputs as I
    monkeypatch.setattr(I, "SEQ_RNN_FUSED", True)


@pytest.fixture
def calls(monkeypatch):
    """names of the library entries called, in order"""
    from torecsys_amd import _abi, functional as F_
    seen = []
    orig = _abi.call

    def spy(name, *args):
        seen.append(name)
        return orig(name, *args)

    monkeypatch.setattr(_abi, "call", spy)
    monkeypatch.setattr(F_, "call", spy)
    return seen


def _expected_path(E, dtype):
    """written out here, not taken from the library: the matrix-core path for bf16 at E = 16, 32 and 64, the vector path
    for fp32 and for every other covered E"""
    if dtype == torch.bfloat16 and E in (16, 32, 64):
        return 2
    return 1 if 1 <= E <= 128 and dtype in (torch.float32, torch.bfloat16) else 0


def _lengths(B, L, seed=0):
    """mixed lengths in [1, L]: the full L in sample 0, 1 in the last sample"""
    g = torch.Generator().manual_seed(6100 + 7 * B + L + seed)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    lens[B - 1] = 1 if B > 1 else L
    return lens


_REF = {}


def _case(shape, cell, dtype, method="avg_pooling"):
    """operands of a case (fp32 images of values representable in ``dtype``) and the fp64 restatement on them, computed
    once and shared; callers leave them unchanged.  ``method`` 'steps': every h_t over the full L."""
    key = (shape, cell, dtype, method)
    if key not in _REF:
        B, L, E = shape
        V = 3 * L + 5
        lengths = _lengths(B, L)
        idx = make_ids(B, L, V, lengths, 6300 + B + L + E)
        params = make_params(cell, E, V, dtype)
        shp = (B, 1, E) if method != "steps" else (B, L, E)
        gout = torch.randn(*shp, generator=torch.Generator().manual_seed(6500 + B + L + E)).to(dtype).float()
        ref = _restate(params, idx, lengths, cell, method, gout)
        _REF[key] = (params, idx, lengths, gout, ref)
    return _REF[key]


def _restate(params, idx, lengths, cell, method, gout):
    p64 = [p.double() for p in params]
    if method == "steps":
        ps = [p.clone().requires_grad_() for p in p64]
        out = seq_rnn_steps(ps[0], idx, lengths, *ps[1:], cell)
        return (out.detach(),) + tuple(torch.autograd.grad(out, ps, gout.double()))
    out, grads = seq_rnn_grads(p64, idx, lengths, cell, method, gout.double())
    return (out,) + tuple(grads)


def _run(dev, dtype, params, idx, lengths, cell, method, gout, padding_idx=0, idx_dtype=torch.int64,
         len_dtype=torch.int64, need=(True,) * 5):
    """functional.seq_rnn forward + backward on the device -> (out, the five gradients or None)"""
    from torecsys_amd import functional as F_
    ps = [p.to(dev).to(dtype).requires_grad_(n) for p, n in zip(params, need)]
    mode = {"avg_pooling": "avg", "sum": "sum", "steps": "none"}[method]
    out = F_.seq_rnn(ps[0], idx.to(dev).to(idx_dtype), lengths.to(dev).to(len_dtype), *ps[1:], cell=cell, mode=mode,
                     padding_idx=padding_idx)
    assert out.dtype == dtype
    wanted = [p for p in ps if p.requires_grad]
    got = iter(torch.autograd.grad(out, wanted, gout.to(dev).to(dtype)))
    grads = [next(got) if p.requires_grad else None for p in ps]
    assert all(g is None or g.dtype == dtype for g in grads)
    return (out.detach(),) + tuple(grads)


def _raw(dev, dtype, params, idx, lengths, cell, gout):
    """the two entries as they are: (out, h, dgates, dgates_h) of mode 0 with the average"""
    from torecsys_amd import functional as F_
    ps = [p.to(dev).to(dtype) for p in params]
    i, n = idx.to(dev), lengths.to(dev)
    out, scale, h, c = F_.seq_rnn_forward_raw(*ps[:1], i, n, *ps[1:], cell, 0, True, save=True)
    dg, dgh = F_.seq_rnn_backward_raw(*ps[:1], i, n, *ps[1:], cell, 0, scale, h, c,
                                      gout.to(dev).to(dtype).reshape(out.shape).contiguous())
    return out, h, dg, dgh


def _errs(got, ref):
    errs = []
    for name, a, b in zip(NAMES, got, ref):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        assert bool(torch.isfinite(a).all()), name
        norm = rel_err_both if name in ("out", "g_table") else rel_err
        errs.append(norm(a.float().cpu(), b))
    return errs


def _paired_case(shape, cell, dtype, seed=0):
    """operands for the bit comparisons: every id in [1, V) sits at no more than two live positions of the batch.  The
    table gradient leaves the sequence kernels as dX and reaches the table through the row-bucket walk all lookups share,
    where the order of a bucket's entries comes from the int32 atomics of the bucket build and may differ between two
    builds.  A sum of two terms has one value in either order, so with these ids all six results have defined bits (and
    rows with two entries still pass the walk's summing).  (params, idx, lengths, gout) as fp32 images of ``dtype``."""
    B, L, E = shape
    lengths = _lengths(B, L, seed)
    n = int(lengths.sum())
    V = n // 2 + 2
    g = torch.Generator().manual_seed(6700 + B + L + E + seed)
    pool = torch.arange(1, V).repeat(2)
    ids = pool[torch.randperm(pool.numel(), generator=g)[:n]]
    live = torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1)
    idx = torch.zeros(B, L, dtype=torch.int64)
    idx[live] = ids
    assert int(torch.bincount(idx[live]).max()) <= 2
    params = make_params(cell, E, V, dtype, seed=seed)
    gout = torch.randn(B, 1, E, generator=torch.Generator().manual_seed(6800 + B + L + E + seed)).to(dtype).float()
    return params, idx, lengths, gout


def _assert_same_bits(got, want):
    """equal bits in the output and all five gradients"""
    for name, a, b in zip(NAMES, got, want):
        assert torch.equal(a, b), name


def _fmt(errs):
    return " ".join(f"{n} {e:.2e}" for n, e in zip(NAMES, errs))


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("cell,method", GOLDEN_CASES, ids=lambda v: v)
@pytest.mark.parametrize("shape", GOLDEN_SHAPES, ids=shape_tag)
def test_sequence_embedding_golden(golden, dev, calls, shape, cell, method):
    """fp32 module with the fixture's state_dict: output, names and the five gradients; one forward and one backward entry"""
    from torecsys_amd import functional as F_, inputs as I
    B, L, E, V = shape
    G = golden(golden_file(shape))
    pre = shape_tag(shape)
    tag = f"{pre}/{cell}_{method}"
    m = I.SequenceIndicesEmbedding(embed_size=E, field_size=V, rnn_method=cell, output_method=method).to(dev)
    assert list(m.state_dict().keys()) == G(tag + "/keys") == PARAM_KEYS
    m.load_state_dict({k: G(f"{pre}/{cell}/param/{k}") for k in PARAM_KEYS}, strict=True)
    assert F_.seq_rnn_path(cell, L, E, torch.float32) == _expected_path(E, torch.float32) == 1
    out = m(G(pre + "/idx").to(dev), G(pre + "/lengths").to(dev))
    assert calls.count(FWD) == 1
    assert out.names == tuple(G(tag + "/names")) == ("B", "N", "E")
    y = out.rename(None)
    assert tuple(y.shape) == tuple(G(tag + "/out").shape)
    (y * G(tag + "/gout").to(dev)).sum().backward()
    assert calls.count(BWD) == 1 and calls.count(FWD) == 1
    sd = m.state_dict(keep_vars=True)
    got = (y.detach(),) + tuple(sd[k].grad for k in PARAM_KEYS)
    errs = _errs(got, (G(tag + "/out"),) + tuple(G(f"{tag}/grad/{k}") for k in PARAM_KEYS))
    print(f"seq golden {tag}: {_fmt(errs)}")
    assert max(errs) <= 1e-5, errs


def test_mean_and_sum_follow_avg_pooling(golden, dev):
    """'mean' is 'avg_pooling' bit for bit; 'sum' is 'avg_pooling' times max(lengths) (5 at this shape, where L is 7)"""
    from torecsys_amd import inputs as I
    shape = (5, 7, 64, 20)
    B, L, E, V = shape
    G = golden(golden_file(shape))
    pre = shape_tag(shape)
    idx, lengths = G(pre + "/idx").to(dev), G(pre + "/lengths").to(dev)
    assert int(lengths.max()) == 5
    outs = {}
    for method in ("avg_pooling", "mean", "sum"):
        m = I.SequenceIndicesEmbedding(embed_size=E, field_size=V, rnn_method="gru", output_method=method).to(dev)
        m.load_state_dict({k: G(f"{pre}/gru/param/{k}") for k in PARAM_KEYS})
        outs[method] = m(idx, lengths)
        assert outs[method].names == ("B", "N", "E") and tuple(outs[method].shape) == (B, 1, E)
    assert torch.equal(outs["mean"].rename(None), outs["avg_pooling"].rename(None))
    assert rel_err(outs["sum"].rename(None).cpu(), 5 * outs["avg_pooling"].rename(None).cpu()) <= 1e-6
    assert rel_err_both(outs["avg_pooling"].rename(None).cpu(), G(f"{pre}/gru_avg_pooling/out")) <= 1e-5


# ------------------------------------------------------------------------------------------------ the restatement, fp64
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=shape_tag)
def test_seq_rnn_against_the_fp64_restatement(dev, calls, shape, cell, dtype):
    from torecsys_amd import functional as F_
    B, L, E = shape
    assert F_.seq_rnn_path(cell, L, E, dtype) == _expected_path(E, dtype)
    assert _expected_path(E, dtype) == (2 if dtype == torch.bfloat16 and E % 16 == 0 and E <= 64 else 1)
    params, idx, lengths, gout, ref = _case(shape, cell, dtype)
    got = _run(dev, dtype, params, idx, lengths, cell, "avg_pooling", gout)
    assert calls.count(FWD) == 1 and calls.count(BWD) == 1
    errs = _errs(got, ref)
    print(f"seq {shape_tag(shape)} {cell} {_dt(dtype)}: {_fmt(errs)}")
    assert max(errs) <= TOL[dtype], errs


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("shape", [(17, 5, 32), (6, 4, 24)], ids=shape_tag)
def test_every_step_against_the_fp64_restatement(dev, shape, cell, dtype):
    """mode 1: (B, L, E) with zeros from each sample's length on, and a gradient of its own per step"""
    params, idx, lengths, gout, ref = _case(shape, cell, dtype, "steps")
    got = _run(dev, dtype, params, idx, lengths, cell, "steps", gout)
    live = (torch.arange(shape[1]).unsqueeze(0) < lengths.unsqueeze(1)).unsqueeze(-1)
    assert not bool((got[0].cpu() * ~live).any())
    errs = _errs(got, ref)
    print(f"seq steps {shape_tag(shape)} {cell} {_dt(dtype)}: {_fmt(errs)}")
    assert max(errs) <= TOL[dtype], errs


# ------------------------------------------------------------------------------------------------ lengths and ids
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("kind", ["all_one", "all_full", "one_short"])
def test_length_patterns(dev, cell, dtype, kind):
    B, L, E, V = 18, 6, 16, 23
    lengths = {"all_one": torch.ones(B, dtype=torch.int64), "all_full": torch.full((B,), L),
               "one_short": torch.tensor([L] * 7 + [1] + [L] * (B - 8))}[kind]
    idx = make_ids(B, L, V, lengths, 71)
    params = make_params(cell, E, V, dtype, seed=3)
    gout = torch.randn(B, 1, E, generator=torch.Generator().manual_seed(72)).to(dtype).float()
    errs = _errs(_run(dev, dtype, params, idx, lengths, cell, "avg_pooling", gout),
                 _restate(params, idx, lengths, cell, "avg_pooling", gout))
    assert max(errs) <= TOL[dtype], errs


@pytest.mark.parametrize("len_dtype", [torch.int32, torch.int64], ids=["len32", "len64"])
@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64], ids=["idx32", "idx64"])
def test_index_dtypes_give_the_same_bits(dev, idx_dtype, len_dtype):
    params, idx, lengths, gout = _paired_case((17, 5, 32), "lstm", torch.float32)
    got = _run(dev, torch.float32, params, idx, lengths, "lstm", "avg_pooling", gout, idx_dtype=idx_dtype, len_dtype=len_dtype)
    assert max(_errs(got, _restate(params, idx, lengths, "lstm", "avg_pooling", gout))) <= 1e-5
    base = _run(dev, torch.float32, params, idx, lengths, "lstm", "avg_pooling", gout)
    _assert_same_bits(got, base)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_padding_id_inside_a_live_stretch(dev, dtype):
    """the padding row is read like any other row (here it is not zero) and gets no gradient"""
    B, L, E, V = 9, 5, 16, 14
    lengths = _lengths(B, L, seed=5)
    idx = make_ids(B, L, V, lengths, 81)
    idx[0, 2] = 0
    idx[3, 0] = 0
    params = list(make_params("gru", E, V, dtype, seed=4))
    params[0] = params[0].clone()
    params[0][0] = torch.randn(E, generator=torch.Generator().manual_seed(82)).to(dtype).float()
    gout = torch.randn(B, 1, E, generator=torch.Generator().manual_seed(83)).to(dtype).float()
    got = _run(dev, dtype, params, idx, lengths, "gru", "avg_pooling", gout, padding_idx=0)
    ref = list(_restate(params, idx, lengths, "gru", "avg_pooling", gout))
    assert float(ref[1][0].abs().max()) > 0          # the restatement has no padding row: it does give that row a gradient
    ref[1] = ref[1].clone()
    ref[1][0] = 0
    assert not bool(got[1][0].any())
    assert max(_errs(got, ref)) <= TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("cell", CELLS)
def test_ids_past_the_lengths_change_nothing(dev, cell, dtype):
    """garbage ids from each sample's length on -- in range, out of range and negative -- against zeros there: equal bits
    in the output and the five gradients (_paired_case), in the kernels' own blocks (h, dgates, dgates_h), and no index
    flag"""
    from torecsys_amd import functional as F_
    shape = (17, 5, 32)
    params, idx, lengths, gout = _paired_case(shape, cell, dtype)
    V = params[0].shape[0]
    junk = torch.randint(-3, V + 4, idx.shape, generator=torch.Generator().manual_seed(91))
    dirty = torch.where(torch.arange(shape[1]).unsqueeze(0) < lengths.unsqueeze(1), idx, junk)
    assert not torch.equal(dirty, idx)
    F_.index_errors_seen()
    clean = _run(dev, dtype, params, idx, lengths, cell, "avg_pooling", gout)
    got = _run(dev, dtype, params, dirty, lengths, cell, "avg_pooling", gout)
    _assert_same_bits(got, clean)
    for a, b in zip(_raw(dev, dtype, params, dirty, lengths, cell, gout), _raw(dev, dtype, params, idx, lengths, cell, gout)):
        assert torch.equal(a, b)
    assert not F_.index_errors_seen()


@pytest.mark.parametrize("what", ["length_zero", "length_past_L", "id_equal_V"])
def test_flagged_inputs(dev, what, monkeypatch):
    """a length outside [1, L] is clamped to [0, L], an id outside [0, V) reads as a zero row and gets no gradient; both
    raise the index flag; everything stays finite and equals the restatement under the same rules"""
    from torecsys_amd import functional as F_
    monkeypatch.setattr(F_, "CHECK_INDICES", False)      # (with it on, the call raises instead: the test below)
    B, L, E, V = 6, 5, 16, 12
    lengths = torch.tensor([5, 3, 1, 4, 2, 5])
    idx = make_ids(B, L, V, lengths, 95)
    if what == "length_zero":
        lengths[1] = 0
    elif what == "length_past_L":
        lengths[1] = L + 3
        idx[1] = torch.randint(1, V, (L,), generator=torch.Generator().manual_seed(96))
    else:
        idx[1, 1] = V
    params = make_params("lstm", E, V, seed=6)
    gout = torch.randn(B, 1, E, generator=torch.Generator().manual_seed(97))
    F_.index_errors_seen()
    got = _run(dev, torch.float32, params, idx, lengths, "lstm", "avg_pooling", gout)
    assert F_.index_errors_seen()
    ref = _restate(params, idx, lengths, "lstm", "avg_pooling", gout)
    if what == "length_zero":
        assert not bool(got[0][1].any())
    assert max(_errs(got, ref)) <= 1e-5


def test_check_indices_raises_index_error(dev, monkeypatch):
    from torecsys_amd import functional as F_
    monkeypatch.setattr(F_, "CHECK_INDICES", True)
    B, L, E, V = 4, 3, 8, 7
    lengths = torch.tensor([3, 2, 1, 3])
    idx = make_ids(B, L, V, lengths, 99)
    params = [p.to(dev) for p in make_params("rnn", E, V)]
    F_.seq_rnn(params[0], idx.to(dev), lengths.to(dev), *params[1:], cell="rnn", mode="avg")
    idx[0, 1] = V
    with pytest.raises(IndexError, match="seq_rnn"):
        F_.seq_rnn(params[0], idx.to(dev), lengths.to(dev), *params[1:], cell="rnn", mode="avg")


# ------------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("cell", CELLS)
def test_two_runs_are_bit_identical(dev, cell, dtype):
    """forward + backward twice: equal bits in the output and the five gradients (_paired_case), and in the kernels' own
    blocks.  With many lookups per table row (the ids of _case: about 20 per row) the bits of the table gradient are those
    of dX and of one bucket order: dX = dgates W_ih of the two runs through ONE set of row buckets gives equal bits."""
    from torecsys_amd import functional as F_
    shape = (67, 64, 64)
    params, idx, lengths, gout = _paired_case(shape, cell, dtype)
    a = _run(dev, dtype, params, idx, lengths, cell, "avg_pooling", gout)
    b = _run(dev, dtype, params, idx, lengths, cell, "avg_pooling", gout)
    _assert_same_bits(a, b)
    params, idx, lengths, gout, _ = _case(shape, cell, dtype)
    raws = [_raw(dev, dtype, params, idx, lengths, cell, gout) for _ in range(2)]
    for s, t in zip(*raws):
        assert torch.equal(s, t)
    w, w_ih = params[0].to(dev).to(dtype), params[1].to(dev).to(dtype)
    B, L, E = shape
    rb = F_.row_buckets(idx.to(dev), None, w.shape[0], skip_row=0)      # (the ids past the lengths are the padding id 0)
    walks = [F_.scatter_rows(rb, w, g_rows=torch.mm(r[2].view(B * L, -1), w_ih).view(B, L, E), padding_row=0) for r in raws]
    assert bool(walks[0].any()) and torch.equal(walks[0], walks[1])


@pytest.mark.parametrize("need", [(False, True, True, True, True), (True, False, False, False, False),
                                  (True, True, False, True, False)], ids=["table_frozen", "rnn_frozen", "mixed"])
def test_frozen_operands_get_no_gradient(dev, need):
    shape = (17, 5, 32)
    params, idx, lengths, gout, ref = _case(shape, "gru", torch.float32)
    got = _run(dev, torch.float32, params, idx, lengths, "gru", "avg_pooling", gout, need=need)
    assert rel_err_both(got[0].cpu(), ref[0]) <= 1e-5
    for name, n, g, r in zip(NAMES[1:], need, got[1:], ref[1:]):
        if not n:
            assert g is None, name
        else:
            assert (rel_err_both if name == "g_table" else rel_err)(g.cpu(), r) <= 1e-5, name


def test_raw_entries_refuse_strided_operands_and_uncovered_shapes(dev, calls):
    from torecsys_amd import functional as F_, inputs as I
    E, V, B, L = 8, 10, 3, 4
    w, idx = torch.zeros(V, E, device=dev), torch.zeros(B, L, dtype=torch.int64, device=dev)
    lens = torch.ones(B, dtype=torch.int64, device=dev)
    p = [torch.zeros(4 * E, E, device=dev), torch.zeros(4 * E, E, device=dev), torch.zeros(4 * E, device=dev),
         torch.zeros(4 * E, device=dev)]
    with pytest.raises(ValueError, match="w_ih must be contiguous"):
        F_.seq_rnn_forward_raw(w, idx, lens, torch.zeros(4 * E, 2 * E, device=dev)[:, ::2], *p[1:], "lstm", 0)
    with pytest.raises(ValueError, match="lengths must be contiguous"):
        F_.seq_rnn_forward_raw(w, idx, torch.ones(2 * B, dtype=torch.int64, device=dev)[::2], *p, "lstm", 0)
    with pytest.raises(TypeError, match="table's dtype"):
        F_.seq_rnn(w, idx, lens, p[0].bfloat16(), *p[1:], cell="lstm")
    with pytest.raises(NotImplementedError, match="does not cover"):
        F_.seq_rnn(torch.zeros(V, 129, device=dev), idx, lens, torch.zeros(129, 129, device=dev),
                   torch.zeros(129, 129, device=dev), torch.zeros(129, device=dev), torch.zeros(129, device=dev), cell="rnn")
    assert not calls
    # E = 129 is outside the kernels' envelope: the module runs the composition and matches the restatement
    E, V, B, L = 129, 9, 3, 4
    lengths = torch.tensor([4, 1, 2])
    ids = make_ids(B, L, V, lengths, 5)
    params = make_params("rnn", E, V, seed=8)
    m = I.SequenceIndicesEmbedding(embed_size=E, field_size=V, rnn_method="rnn").to(dev)
    m.load_state_dict(dict(zip(PARAM_KEYS, params)))
    y = m(ids.to(dev), lengths.to(dev))
    assert FWD not in calls and y.names == ("B", "N", "E")
    assert rel_err_both(y.rename(None).detach().cpu(), _restate(params, ids, lengths, "rnn", "avg_pooling",
                                                                 torch.zeros(B, 1, E))[0]) <= 1e-5


def test_empty_batch(dev):
    from torecsys_amd import inputs as I
    m = I.SequenceIndicesEmbedding(embed_size=16, field_size=9).to(dev)
    y = m(torch.zeros(0, 5, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev))
    assert tuple(y.shape) == (0, 1, 16) and y.names == ("B", "N", "E")


# ------------------------------------------------------------------------------------------------ hipGraph capture
def test_avg_pooling_captures_into_a_graph(dev):
    """one forward + backward of the fused avg_pooling path at (33, 7, 64) in bf16 under torch.cuda.graph (a single chain on
    one stream), replayed with new ids and lengths copied into the static tensors, equals the eager result bit for bit.  A
    host read of the lengths anywhere on that path would fail the capture."""
    from torecsys_amd import functional as F_
    B, L, E = 33, 7, 64
    dtype = torch.bfloat16
    V = B * L // 2 + 2      # room for the ids of every draw below
    params = [p.to(dev).to(dtype) for p in make_params("lstm", E, V, dtype, seed=9)]
    gout = torch.randn(B, 1, E, generator=torch.Generator().manual_seed(12)).to(dev).to(dtype)

    def draw(n):
        # (a replay builds its row buckets anew: ids at no more than two live positions, see _paired_case)
        _, idx, lengths, _ = _paired_case((B, L, E), "lstm", dtype, seed=20 + n)
        assert int(idx.max()) < V
        return idx.to(dev), lengths.to(dev)

    def run(idx, lengths):
        ps = [p.detach().requires_grad_() for p in params]
        out = F_.seq_rnn(ps[0], idx, lengths, *ps[1:], cell="lstm", mode="avg", padding_idx=0)
        return [out.detach()] + list(torch.autograd.grad(out, ps, gout))

    sets = [draw(n) for n in range(3)]
    eager = [[t.clone() for t in run(*s)] for s in sets]
    assert not torch.equal(eager[1][0], eager[2][0])
    static = [t.clone() for t in sets[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(*static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        results = run(*static)
    for s, want in list(zip(sets, eager))[1:]:
        for dst, src in zip(static, s):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same_bits(results, want)


# ------------------------------------------------------------------------------------------------ the switch
_CHILD = """
import sys, torch
from torecsys_amd import inputs as I
assert I.SEQ_RNN_FUSED is False
calls = []
from torecsys_amd import _abi, functional as F_
orig = _abi.call
def spy(name, *a):
    calls.append(name)
    return orig(name, *a)
_abi.call = F_.call = spy
d = torch.load(sys.argv[1])
dev = torch.device("cuda:0")
res = {}
for cell, sd in d["state"].items():
    m = I.SequenceIndicesEmbedding(embed_size=d["E"], field_size=d["V"], rnn_method=cell).to(dev)
    m.load_state_dict(sd)
    y = m(d["idx"].to(dev), d["lengths"].to(dev))
    assert y.names == ("B", "N", "E")
    (y.rename(None) * d["gout"].to(dev)).sum().backward()
    g = m.state_dict(keep_vars=True)
    res[cell] = [y.rename(None).detach().cpu()] + [g[k].grad.cpu() for k in d["keys"]]
assert "trs_gather_rows" in calls and not any(c.startswith("trs_seq_rnn") for c in calls), calls
torch.save(res, sys.argv[2])
print("SEQ-COMPOSITION OK")
"""


def test_switch_selects_the_composition(dev, tmp_path):
    """TRS_SEQ_RNN=0 is read at import, so the composition (HIP gather, the module's own RNN on a packed sequence, ATen
    pooling) runs in a process of its own: it calls no trs_seq_rnn_* entry and meets the fp32 bound against the same fp64
    restatement"""
    shape = (17, 5, 32)
    B, L, E = shape
    cases = {cell: _case(shape, cell, torch.float32) for cell in CELLS}
    params, idx, lengths, gout, _ = cases["lstm"]
    src, dst = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save({"state": {cell: dict(zip(PARAM_KEYS, c[0])) for cell, c in cases.items()}, "idx": idx, "lengths": lengths,
                "gout": gout, "E": E, "V": params[0].shape[0], "keys": PARAM_KEYS}, src)
    env = dict(os.environ, TRS_SEQ_RNN="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CHILD, src, dst], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "SEQ-COMPOSITION OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    res = torch.load(dst)
    for cell, c in cases.items():
        errs = _errs(res[cell], c[4])
        print(f"seq composition {cell} fp32: {_fmt(errs)}")
        assert max(errs) <= 1e-5, (cell, errs)

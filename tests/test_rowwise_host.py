"""Host side of FusedSparseRowWiseAdagrad (no GPU): constructor validation, the (V,) state and its checkpoint round trip,
which tables the optimizer accepts, and the optimizer tail ``2 | TRS_OPT_ROWWISE`` of both fused-update entries of the
built library."""
import ctypes

import pytest
import torch

from torecsys_amd import functional as F_
from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseRowWiseAdagrad

ROWWISE = 2 | 16


def test_constructor_validation_and_capturable_typing():
    opt = FusedSparseRowWiseAdagrad()
    assert (opt.lr, opt.eps, opt.initial, opt.capturable) == (1e-2, 1e-10, 0.0, False)
    assert opt.kind == 2 and opt.rowwise is True and not getattr(FusedSparseAdagrad(), "rowwise", False)
    assert FusedSparseRowWiseAdagrad(0.1, capturable=True).capturable is True
    with pytest.raises(TypeError):
        FusedSparseRowWiseAdagrad(0.1, capturable=1)
    with pytest.raises(TypeError):
        FusedSparseRowWiseAdagrad(0.1, capturable="yes")
    with pytest.raises(ValueError):
        FusedSparseRowWiseAdagrad(-0.1)
    with pytest.raises(ValueError):
        opt.set_lr(-1.0)
    with pytest.raises(RuntimeError):
        opt.lr_tensor("cpu")                        # by value: no device scalar
    cap = FusedSparseRowWiseAdagrad(0.5, capturable=True)
    t = cap.lr_tensor("cpu")
    cap.set_lr(0.125)
    assert t.dtype == torch.float32 and t.shape == (1,) and float(t) == 0.125
    assert F_.TRS_OPT_ROWWISE == 16


def test_state_is_one_fp32_per_row_and_round_trips():
    p = torch.nn.Parameter(torch.zeros(6, 8))
    a = FusedSparseRowWiseAdagrad(0.05, eps=1e-9, initial_accumulator_value=0.25)
    s = a.state_for(p.data, p)
    assert s.shape == (6,) and s.dtype == torch.float32 and torch.equal(s, torch.full((6,), 0.25))
    assert a.state_for(p.data, p) is s                                  # kept, keyed by the parameter
    s.copy_(torch.arange(6.0))
    sd = a.state_dict([("emb.weight", p)])
    assert sd["hyper"] == {"lr": 0.05, "eps": 1e-9, "initial": 0.25}
    assert sorted(sd["tables"]["emb.weight"]) == ["step", "sum"]
    assert sd["tables"]["emb.weight"]["sum"].shape == (6,)

    q = torch.nn.Parameter(torch.zeros(6, 8))
    b = FusedSparseRowWiseAdagrad(0.9)
    b.load_state_dict(sd, [("emb.weight", q)])
    assert (b.lr, b.eps, b.initial) == (0.05, 1e-9, 0.25)
    assert torch.equal(b.state_for(q.data, q), torch.arange(6.0))
    with pytest.raises(KeyError):
        b.load_state_dict(sd, [("other", q)])
    # the shape check is against (V,): an element-wise Adagrad checkpoint of the same table does not load, nor the reverse
    e = FusedSparseAdagrad(0.05)
    e.state_for(p.data, p)
    with pytest.raises(ValueError, match=r"shape \(6, 8\)"):
        b.load_state_dict(e.state_dict([("emb.weight", p)]), [("emb.weight", q)])
    with pytest.raises(ValueError, match=r"shape \(6,\)"):
        e.load_state_dict(sd, [("emb.weight", q)])
    wrong = {"hyper": {}, "tables": {"emb.weight": {"step": 0, "sum": torch.zeros(5)}}}
    with pytest.raises(ValueError, match=r"shape \(5,\)"):
        b.load_state_dict(wrong, [("emb.weight", q)])
    # rebuilt when V changes
    p2 = torch.nn.Parameter(torch.zeros(9, 8))
    assert b._entry(p2.data, q)["sum"].shape == (9,)


def test_sink_args_hand_over_the_flag_and_the_row_state():
    opt = FusedSparseRowWiseAdagrad(0.5, eps=1e-6)
    w = torch.zeros(7, 16)
    assert w.data_ptr() % 16 == 0
    kind, lr, lr_dev, eps, b1, b2, state, state2 = F_._sink_args(opt, w, None)
    assert kind == ROWWISE and lr == 0.5 and eps == pytest.approx(1e-6) and (b1, b2) == (0.0, 0.0)
    assert state.value == opt.state_for(w, None).data_ptr() and opt.state_for(w, None).shape == (7,)
    assert not lr_dev and not state2
    # E == 1 takes the element walk, where the rule IS element-wise Adagrad on the (V,) state seen as (V, 1)
    w1 = torch.zeros(7, 1)
    kind, *_, state, state2 = F_._sink_args(opt, w1, None)
    assert kind == 2 and state.value == opt.state_for(w1, None).data_ptr() and opt.state_for(w1, None).shape == (7,)
    # the element-wise optimizer is what it was
    assert F_._sink_args(FusedSparseAdagrad(0.5), w, None)[0] == 2


@pytest.mark.parametrize("E", [10, 12])
def test_widths_of_the_element_walk_are_refused_before_the_c_call(E):
    """E = 10 fp32 is no whole number of 16-byte vectors; E = 12 fp32 is three of them, not a power of two"""
    opt = FusedSparseRowWiseAdagrad(0.5)
    with pytest.raises(NotImplementedError) as ei:
        F_._sink_args(opt, torch.zeros(5, E), None)
    msg = str(ei.value)
    assert f"{E} x" in msg and "whole 16-byte vectors, 1..64 of them a power of two" in msg
    assert not opt._state                                          # refused before any state was made


def test_a_misaligned_operand_is_refused_before_the_c_call():
    """the library's choice of walk also looks at the alignment of the gradient operands (and of the table): the Python
    check is the same predicate, so the refusal is the documented NotImplementedError, not an error code of the call"""
    opt = FusedSparseRowWiseAdagrad(0.5)
    w = torch.zeros(5, 16)
    off = torch.zeros(5 * 16 + 1)[1:].view(5, 16)                  # starts 4 bytes behind a 16-byte boundary
    assert w.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    for table, operands in ((w, (off, None, None)), (w, (None, off, None)), (w, (w, None, off)), (off, ())):
        with pytest.raises(NotImplementedError, match="16-byte aligned"):
            F_._sink_args(opt, table, None, operands)
    assert F_._sink_args(opt, w, None, (w, None, w))[0] == ROWWISE


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_rowwise_tail_is_validated_without_gpu(lib):
    """optimizer = kind | flags: 2 | 16 is the one value with a flag that passes; a missing state is TRS_EINVAL, a row the
    element walk would take TRS_ESHAPE, all before any launch and with the entry's name in front; a mapped update of no
    rows is TRS_OK.  No call here carries a fully valid argument set with non-zero sizes."""
    from torecsys_amd import _abi
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    EINVAL, ESHAPE = -1, -3
    good = dict(optimizer=ROWWISE, state=p, state2=null, E=16, U=5, table=p)

    def tail(a):
        return (a["optimizer"], 0.1, null, 1e-8, 0.0, 0.0, a["state"], a["state2"], p, 1 << 20, null)

    def plain(**kw):
        a = {**good, **kw}
        return lib.trs_scatter_rows_update(p, 0, null, 0, null, a["table"], p, p, 40, 10, a["E"], 4, 0, -1, *tail(a))

    def mapped(**kw):
        a = {**good, **kw}
        return lib.trs_scatter_rows_update_mapped(p, a["table"], p, p, p, 40, a["U"], 10, a["E"], 0, *tail(a))

    for name, entry in (("scatter_rows_update", plain), ("scatter_rows_update_mapped", mapped)):
        for kw in (dict(state=null), dict(optimizer=16), dict(optimizer=1 | 16), dict(optimizer=3 | 16, state2=p),
                   dict(optimizer=2 | 32), dict(optimizer=2 | 16 | 32), dict(optimizer=0 | 16 | 64), dict(table=null)):
            assert entry(**kw) == EINVAL, (name, kw)
            assert _abi.last_error().startswith(name + ":"), (name, kw, _abi.last_error())
        for E in (10, 12):                       # fp32: 40 bytes; 48 bytes = three vectors
            assert entry(E=E) == ESHAPE, (name, E)
            assert _abi.last_error().startswith(name + ":"), (name, E, _abi.last_error())
    # a misaligned table pointer takes the element walk too
    assert plain(table=ctypes.c_void_p(20)) == ESHAPE
    assert mapped(U=0) == 0
    assert mapped(U=0, state2=p) == 0            # state2 is ignored
    assert mapped(U=0, state=null) == EINVAL     # a bad tail is refused even where there is nothing to update
    assert mapped(U=0, optimizer=1 | 16) == EINVAL

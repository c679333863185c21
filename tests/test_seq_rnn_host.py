"""SequenceIndicesEmbedding, host side (no GPU): the plain torch restatement against the reference's fixture
(tests/golden/seq_rnn.npz, seq_rnn_e64.npz), the path function, argument validation of the new C-ABI entries, constructor /
state_dict parity of the drop-in, patch() / unpatch()."""
import ctypes
import sys
import types

import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from seq_rnn_ref import (GATES, GOLDEN_CASES, GOLDEN_SHAPES, PARAM_KEYS, golden_file, seq_rnn, seq_rnn_grads, shape_tag)

CASES = [(s, c, m) for s in GOLDEN_SHAPES for c, m in GOLDEN_CASES]


def _case(golden, shape, cell, method):
    G = golden(golden_file(shape))
    pre = shape_tag(shape)
    tag = f"{pre}/{cell}_{method}"
    params = [G(f"{pre}/{cell}/param/{k}") for k in PARAM_KEYS]
    grads = [G(f"{tag}/grad/{k}") for k in PARAM_KEYS]
    return G, tag, G(pre + "/idx"), G(pre + "/lengths"), params, grads


@pytest.mark.parametrize("shape,cell,method", CASES, ids=lambda v: shape_tag(v) if isinstance(v, tuple) else v)
def test_fixture_equals_the_plain_torch_restatement(golden, shape, cell, method):
    """fp32 restatement against the reference's own output and its five gradients: 1e-5 in the max norm, the project's
    fp32 contract"""
    B, L, E, V = shape
    G, tag, idx, lengths, params, grads = _case(golden, shape, cell, method)
    longest = int(lengths.max())
    assert tuple(idx.shape) == (B, L) and tuple(lengths.shape) == (B,) and int(lengths.min()) == 1
    assert longest == (5 if shape == (5, 7, 64, 20) else L)
    assert bool((idx[torch.arange(L).unsqueeze(0) >= lengths.unsqueeze(1)] == 0).all())
    assert G(tag + "/names") == ["B", "N", "E"] and G(tag + "/keys") == PARAM_KEYS
    want = {"avg_pooling": (B, 1, E), "none": (B, longest, E), "max_pooling": (B, longest, 1)}[method]
    assert tuple(G(tag + "/out").shape) == tuple(G(tag + "/gout").shape) == want
    assert tuple(params[1].shape) == tuple(params[2].shape) == (GATES[cell] * E, E)
    out, got = seq_rnn_grads(params, idx, lengths, cell, method, G(tag + "/gout"))
    errs = [rel_err(out, G(tag + "/out"))] + [rel_err(a, b) for a, b in zip(got, grads)]
    print(f"seq restatement {tag}: out {errs[0]:.2e} grads " + " ".join(f"{e:.2e}" for e in errs[1:]))
    assert max(errs) <= 1e-5, errs
    # positions past a sample's length take no part: the padding row gets no gradient from them (it is not looked up)
    assert float(grads[0][0].abs().max()) == 0.0


def test_restatement_pooling_rules():
    """the divisor is max(lengths) of the batch; mean == avg_pooling; sum == avg_pooling * max(lengths); garbage ids past
    the lengths change nothing"""
    from seq_rnn_ref import make_ids, make_params
    B, L, E, V = 5, 6, 8, 11
    lengths = torch.tensor([4, 1, 3, 2, 4])
    idx = make_ids(B, L, V, lengths, 1)
    p = [t.double() for t in make_params("gru", E, V)]
    avg = seq_rnn(*p[:1], idx, lengths, *p[1:], "gru", "avg_pooling")
    steps = seq_rnn(*p[:1], idx, lengths, *p[1:], "gru", "none")
    assert tuple(steps.shape) == (B, 4, E) and float(steps[1, 1:].abs().max()) == 0.0
    assert rel_err(avg, steps.sum(1, keepdim=True) / 4) <= 1e-14
    assert torch.equal(avg, seq_rnn(*p[:1], idx, lengths, *p[1:], "gru", "mean"))
    assert rel_err(seq_rnn(*p[:1], idx, lengths, *p[1:], "gru", "sum"), avg * 4) <= 1e-14
    junk = torch.where(torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1), idx, torch.full_like(idx, 7))
    assert torch.equal(avg, seq_rnn(*p[:1], junk, lengths, *p[1:], "gru", "avg_pooling"))
    assert tuple(seq_rnn(*p[:1], idx, lengths, *p[1:], "gru", "max_pooling").shape) == (B, 4, 1)


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


# (cell, L, E, dtype code) -> path.  2: the matrix-core path, bf16 with E in {16, 32, 64}, all three cells; 1: the vector
# path (fp32 FMA) for fp32 operands and for every other covered E in bf16 (8, 24, 48, 128: off the 16 grid, or a count
# of 16-unit tiles that the four waves do not divide, or past the register budget); 0: not covered (dtype code 2 stands
# for fp16, which the library has no code for)
PATHS = [((1, 50, 64, 0), 1), ((1, 50, 64, 1), 2), ((0, 1, 16, 1), 2), ((2, 7, 32, 1), 2), ((0, 50, 8, 0), 1),
         ((0, 50, 64, 1), 2), ((2, 50, 64, 1), 2), ((1, 50, 16, 1), 2), ((2, 50, 16, 1), 2), ((0, 50, 32, 1), 2),
         ((1, 50, 32, 1), 2), ((1, 50, 16, 0), 1), ((2, 50, 32, 0), 1), ((1, 50, 48, 1), 1), ((1, 50, 8, 1), 1),
         ((2, 50, 24, 0), 1), ((2, 50, 24, 1), 1), ((1, 3, 128, 0), 1), ((1, 3, 128, 1), 1), ((0, 100000, 1, 0), 1),
         ((1, 50, 129, 0), 0), ((1, 50, 129, 1), 0), ((2, 50, 0, 0), 0), ((1, 0, 64, 0), 0), ((3, 50, 64, 0), 0),
         ((-1, 50, 64, 1), 0), ((1, 50, 64, 2), 0), ((1, 50, 64, 7), 0)]


def test_path_function(lib):
    from torecsys_amd import functional as F_
    for args, want in PATHS:
        assert lib.trs_seq_rnn_path(*args) == want, args
    assert F_.SEQ_RNN_PATH_VECTOR == 1 and F_.SEQ_RNN_PATH_MATRIX == 2
    for cell, code in (("rnn", 0), ("lstm", 1), ("gru", 2)):
        assert F_.SEQ_RNN_CELLS[cell] == code
        assert F_.seq_rnn_path(cell, 50, 64, torch.float32) == F_.seq_rnn_path(code, 50, 24, torch.bfloat16) == 1
        assert F_.seq_rnn_path(cell, 50, 64, torch.bfloat16) == F_.seq_rnn_path(code, 7, 16, torch.bfloat16) == 2
        assert F_.seq_rnn_path(cell, 50, 129, torch.float32) == 0
        assert F_.seq_rnn_path(cell, 50, 64, torch.float16) == 0
        assert lib.trs_seq_rnn_workspace_bytes(code, 64) == 2 * GATES[cell] * 64 * 64 * 4
    assert lib.trs_seq_rnn_workspace_bytes(1, 129) == 0 and lib.trs_seq_rnn_workspace_bytes(5, 64) == 0
    with pytest.raises(ValueError, match="cell"):
        F_.seq_rnn_path("elman", 50, 64, torch.float32)


def test_seq_entries_validate_arguments_without_gpu(lib):
    from torecsys_amd import _abi
    for name in ("trs_seq_rnn_path", "trs_seq_rnn_workspace_bytes", "trs_seq_rnn_fwd", "trs_seq_rnn_bwd"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    assert lib.trs_version() == 3
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    WS = 1 << 20

    def fwd(table=one, V=10, E=16, dtype=0, idx=one, idt=0, lens=one, ldt=0, B=2, L=5, w_ih=one, w_hh=one, b_ih=one,
            b_hh=one, cell=1, mode=0, average=1, scale=one, out=one, h=null, c=null, ws=one, ws_bytes=WS, flag=null):
        return lib.trs_seq_rnn_fwd(table, V, E, dtype, idx, idt, lens, ldt, B, L, w_ih, w_hh, b_ih, b_hh, cell, mode, average,
                                   scale, out, h, c, ws, ws_bytes, flag, null)

    def bwd(table=one, V=10, E=16, dtype=0, idx=one, idt=0, lens=one, ldt=0, B=2, L=5, w_ih=one, w_hh=one, b_ih=one,
            b_hh=one, cell=1, mode=0, scale=one, h=one, c=one, gout=one, dg=one, dgh=null, ws=one, ws_bytes=WS):
        return lib.trs_seq_rnn_bwd(table, V, E, dtype, idx, idt, lens, ldt, B, L, w_ih, w_hh, b_ih, b_hh, cell, mode, scale,
                                   h, c, gout, dg, dgh, ws, ws_bytes, null)

    everything_null = dict(table=null, idx=null, lens=null, w_ih=null, w_hh=null, b_ih=null, b_hh=null, scale=null, ws=null)
    assert fwd(B=0, out=null, **everything_null) == 0                      # B == 0: nothing is touched
    assert bwd(B=0, h=null, c=null, gout=null, dg=null, **everything_null) == 0
    for hole in ("table", "idx", "lens", "w_ih", "w_hh", "b_ih", "b_hh", "scale", "out", "ws"):
        assert fwd(**{hole: null}) == -1 and "NULL" in _abi.last_error(), hole
    for hole in ("table", "idx", "lens", "w_ih", "w_hh", "b_ih", "b_hh", "scale", "h", "gout", "dg", "ws"):
        assert bwd(**{hole: null}) == -1 and "NULL" in _abi.last_error(), hole
    for entry, name in ((fwd, "seq_rnn_fwd"), (bwd, "seq_rnn_bwd")):
        assert entry(cell=3) == -1 and "cell 3" in _abi.last_error() and _abi.last_error().startswith(name)
        assert entry(cell=-1) == -1 and "cell" in _abi.last_error()
        assert entry(mode=2) == -1 and "mode 2" in _abi.last_error()
        assert entry(idt=5) == -1 and entry(ldt=2) == -1 and "index dtype" in _abi.last_error()
        assert entry(B=-1) == -1 and "B=-1" in _abi.last_error()
        assert entry(dtype=7) == -2 and "dtype" in _abi.last_error()
        assert entry(dtype=2) == -2                                        # fp16 has no code
        assert entry(E=129) == -3 and "E=129" in _abi.last_error()
        assert entry(E=0) == -3 and entry(L=0) == -3 and "L=0" in _abi.last_error()
        assert entry(E=129, dtype=1) == -3
        assert entry(ws_bytes=2 * 4 * 16 * 16 * 4 - 1) == -6 and "workspace" in _abi.last_error()
    assert bwd(c=null) == -1 and "c_save" in _abi.last_error()              # the lstm's cell state
    assert bwd(cell=2, dgh=null) == -1 and "dgates_h" in _abi.last_error()  # the gru's hidden-side block
    with pytest.raises(RuntimeError, match="trs_seq_rnn_fwd failed"):
        _abi.call("trs_seq_rnn_fwd", null, 10, 16, 0, null, 0, null, 0, 2, 5, null, null, null, null, 1, 0, 1, null, null,
                  null, null, null, 0, null, null)


def test_functional_validation_without_gpu():
    from torecsys_amd import functional as F_
    E, V, B, L = 8, 10, 3, 4
    w, idx, lens = torch.zeros(V, E), torch.zeros(B, L, dtype=torch.int64), torch.ones(B, dtype=torch.int64)
    p = [torch.zeros(4 * E, E), torch.zeros(4 * E, E), torch.zeros(4 * E), torch.zeros(4 * E)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.seq_rnn(w, idx, lens, *p, cell="lstm", mode="avg")
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.seq_rnn_forward_raw(w, idx, lens, *p, "lstm", 0)
    with pytest.raises(ValueError, match="mode must be one of"):
        F_.seq_rnn(w, idx, lens, *p, cell="lstm", mode="median")
    with pytest.raises(ValueError, match="cell must be one of"):
        F_.seq_rnn(w, idx, lens, *p, cell="elman")
    # the raw calls read dense rows: a strided operand is refused, not misread
    with pytest.raises(ValueError, match="weight must be contiguous"):
        F_.seq_rnn_forward_raw(torch.zeros(V, 2 * E)[:, ::2], idx, lens, *p, "lstm", 0)
    with pytest.raises(ValueError, match="idx must be contiguous"):
        F_.seq_rnn_forward_raw(w, torch.zeros(B, 2 * L, dtype=torch.int64)[:, ::2], lens, *p, "lstm", 0)
    with pytest.raises(ValueError, match="w_hh must be contiguous"):
        F_.seq_rnn_forward_raw(w, idx, lens, p[0], torch.zeros(4 * E, 2 * E)[:, ::2], p[2], p[3], "lstm", 0)
    with pytest.raises(ValueError, match="gout must be contiguous"):
        F_.seq_rnn_backward_raw(w, idx, lens, *p, "lstm", 0, torch.ones(1), torch.zeros(B, L, E), torch.zeros(B, L, E),
                                torch.zeros(B, 2 * E)[:, ::2])


def test_constructor_parity_with_the_reference(golden):
    import torecsys_amd
    from torecsys_amd import inputs as I
    assert torecsys_amd.SequenceIndicesEmbedding is I.SequenceIndicesEmbedding
    m = I.SequenceIndicesEmbedding(embed_size=8, field_size=9)
    assert isinstance(m.rnn_layers, nn.LSTM) and m.output_method == "avg_pooling" and m.length == 8 == len(m)
    assert m.embedding.padding_idx == 0 and list(m.state_dict().keys()) == PARAM_KEYS
    r = m.rnn_layers
    assert (r.input_size, r.hidden_size, r.num_layers, r.bias, r.batch_first, r.bidirectional) == (8, 8, 1, True, True, False)
    for cell, cls in (("rnn", nn.RNN), ("lstm", nn.LSTM), ("gru", nn.GRU)):
        assert type(I.SequenceIndicesEmbedding(8, 9, rnn_method=cell).rnn_layers) is cls
    for method in ("avg_pooling", "max_pooling", "mean", "none", "sum"):
        assert I.SequenceIndicesEmbedding(8, 9, output_method=method).output_method == method
    with pytest.raises(ValueError, match="rnn_method only allows"):
        I.SequenceIndicesEmbedding(8, 9, rnn_method="elman")
    with pytest.raises(ValueError, match="output_method only allows"):
        I.SequenceIndicesEmbedding(8, 9, output_method="median")
    for kw in (dict(num_layers=2), dict(bias=False), dict(bidirectional=True), dict(dropout=0.1)):
        with pytest.raises(TypeError, match="unexpected keyword argument"):
            I.SequenceIndicesEmbedding(8, 9, **kw)
    with pytest.raises(NotImplementedError, match="max_norm"):
        I.SequenceIndicesEmbedding(8, 9, max_norm=1.0)
    # a reference checkpoint loads
    for shape in GOLDEN_SHAPES:
        B, L, E, V = shape
        G = golden(golden_file(shape))
        for cell in ("lstm", "gru", "rnn"):
            m = I.SequenceIndicesEmbedding(embed_size=E, field_size=V, rnn_method=cell)
            sd = {k: G(f"{shape_tag(shape)}/{cell}/param/{k}") for k in PARAM_KEYS}
            res = m.load_state_dict(sd, strict=True)
            assert not res.missing_keys and not res.unexpected_keys
            assert list(m.state_dict().keys()) == G(f"{shape_tag(shape)}/{cell}_avg_pooling/keys")
    # the schema carries the lengths column; the fused optimizer is refused
    m = I.SequenceIndicesEmbedding(8, 9)
    with pytest.raises(ValueError):
        m.set_schema("clicks")
    m.set_schema("clicks", lengths="n_clicks")
    assert m.schema.inputs == ["clicks"] and m.schema.lengths == "n_clicks"
    assert m.set_fused_optimizer(None).fused_optimizer is None
    with pytest.raises(NotImplementedError, match="fused sparse optimizer"):
        m.set_fused_optimizer(object())
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 3, dtype=torch.int64), torch.ones(2, dtype=torch.int64))


def test_router_hands_the_lengths_column_over():
    """Inputs.forward gives an entry whose class is named SequenceIndicesEmbedding (or, as the reference spells it,
    SequenceIndexEmbedding) ``inputs[schema.lengths]`` as its second argument"""
    from torecsys_amd import inputs as I
    seen = {}

    def make(name):
        def forward(self, inputs, lengths):
            seen[name] = (inputs, lengths)
            return torch.zeros(inputs.shape[0], 1, 4)
        cls = type(name, (I.BaseInput,), {"forward": forward, "set_schema": I.SequenceIndicesEmbedding.set_schema})
        m = cls()
        m.length = 4
        m.set_schema("clicks", lengths="n_clicks")
        return m

    router = I.Inputs({"a": make("SequenceIndicesEmbedding"), "b": make("SequenceIndexEmbedding")})
    batch = {"clicks": torch.arange(6).view(2, 3), "n_clicks": torch.tensor([3, 1])}
    out = router(batch)
    assert list(out) == ["a", "b"]
    for name in ("SequenceIndicesEmbedding", "SequenceIndexEmbedding"):
        assert torch.equal(seen[name][0], batch["clicks"]) and seen[name][1] is batch["n_clicks"]


def test_patch_rebinds_and_restores_the_sequence_embedding():
    import torecsys_amd
    from torecsys_amd import inputs as I, patching
    assert patching._SEQUENCE_NAMES == ["SequenceIndicesEmbedding"]
    assert "SequenceIndicesEmbedding" not in patching._INPUT_NAMES + patching._LAYER_NAMES + patching._ROUTER_NAMES
    pkg = types.ModuleType("fake_seq_trs")
    inp = types.ModuleType("fake_seq_trs.inputs")
    base = types.ModuleType("fake_seq_trs.inputs.base")
    old = type("SequenceIndicesEmbedding", (nn.Module,), {"__module__": base.__name__})
    inp.SequenceIndicesEmbedding = base.SequenceIndicesEmbedding = old
    pkg.inputs, inp.base = inp, base
    mods = (pkg, inp, base)
    for m in mods:
        sys.modules[m.__name__] = m
    try:
        torecsys_amd.patch(pkg, heads=False)
        assert inp.SequenceIndicesEmbedding is I.SequenceIndicesEmbedding
        assert base.SequenceIndicesEmbedding is I.SequenceIndicesEmbedding
        assert I.SequenceIndicesEmbedding.__name__ == "SequenceIndicesEmbedding"      # the router dispatches on the name
        assert I.SequenceIndicesEmbedding not in I._SIDE_LOOKUPS
        torecsys_amd.unpatch()
        assert inp.SequenceIndicesEmbedding is old and base.SequenceIndicesEmbedding is old
    finally:
        torecsys_amd.unpatch()
        for m in mods:
            sys.modules.pop(m.__name__, None)

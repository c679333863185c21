"""MixtureOfExpertsLayer (MoE / MMoE), host side (no GPU): the plain torch restatement against the reference's fixture
(tests/golden/moe.npz), constructor / state_dict parity of the drop-in, its two ValueErrors, patch() / unpatch(), argument
validation of the new C-ABI entries."""
import ctypes
import sys
import types

import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from moe_ref import (DEEPMOE_ARGS, KINK_MARGIN, MMOE_ARGS, MODEL_BATCH, MOE_SHAPES, deep_moe, gate, gate_backward,
                     kink_margin, layer_kwargs, mmoe, moe_layer, shape_tag)


def _params(G, pre, **kw):
    return {k: G(f"{pre}/param/{k}").clone().requires_grad_(**kw) for k in G(pre + "/keys")}


def _expected_keys(X, G, hidden):
    keys = []
    for i in range(X):
        for j in range(len(hidden)):
            keys += [f"experts.Expert_{i}.model.Linear_{j}.weight", f"experts.Expert_{i}.model.Linear_{j}.bias"]
        keys += [f"experts.Expert_{i}.model.LinearOutput.weight", f"experts.Expert_{i}.model.LinearOutput.bias"]
    for g in range(G):
        keys += [f"gates.Gate_{g}.Linear.weight", f"gates.Gate_{g}.Linear.bias"]
    return keys


@pytest.mark.parametrize("shape", MOE_SHAPES, ids=shape_tag)
def test_fixture_equals_the_plain_torch_composition(golden, shape):
    """experts -> cat -> softmax(x2 W_g^T + b_g) * experts (moe_ref.moe_layer) reproduces the reference's own output
    (<= 1e-6) and gradients (<= 1e-5), and the written-out gate backward agrees with autograd."""
    G = golden("moe")
    B, N, E, X, Oi, Gn, hidden = shape
    pre = shape_tag(shape)
    assert G(pre + "/names") == ["B", "N", "O"]
    assert G(pre + "/keys") == _expected_keys(X, Gn, hidden)          # experts first, then the gates: the reference's order
    x = G(pre + "/x").clone().requires_grad_()
    P = _params(G, pre)
    assert tuple(x.shape) == (B, N, E) and tuple(G(pre + "/out").shape) == (B, Gn, X * Oi)
    acts = []
    y = moe_layer(x, P, pre=acts)
    assert rel_err(y, G(pre + "/out")) <= 1e-6
    assert kink_margin(acts) >= KINK_MARGIN                           # what the generator asserted
    (y * G(pre + "/gout")).sum().backward()
    assert rel_err(x.grad, G(pre + "/gx")) <= 1e-5
    for k, p in P.items():
        assert rel_err(p.grad, G(f"{pre}/grad/{k}")) <= 1e-5, k
    # the gate alone: forward and the backward formulas the kernel implements, against autograd
    g0 = torch.Generator().manual_seed(B + Gn)
    K = X * Oi
    logits = torch.randn(B, Gn * K, generator=g0).requires_grad_()
    bias = torch.randn(Gn * K, generator=g0)
    e = torch.randn(B, K, generator=g0).requires_grad_()
    gout = torch.randn(B, Gn, K, generator=g0)
    out = gate(logits, bias, e)
    (out * gout).sum().backward()
    gl, ge, mag = gate_backward(logits.detach(), bias, e.detach(), gout)
    assert rel_err(gl, logits.grad) <= 1e-5 and rel_err(ge, e.grad) <= 1e-5
    assert tuple(mag.shape) == (B, Gn) and bool((mag > 0).all())


@pytest.mark.parametrize("name", ["mmoe", "deep_moe"])
def test_model_fixture_equals_the_plain_torch_composition(golden, name):
    G = golden("moe")
    pre = "model/" + name
    P = {k: G(f"{pre}/param/{k}") for k in G(pre + "/keys")}
    args = MMOE_ARGS if name == "mmoe" else DEEPMOE_ARGS
    x = G(pre + "/x").clone().requires_grad_()
    assert tuple(x.shape) == (MODEL_BATCH, args["num_fields"], args["embed_size"])
    acts = []
    y = (mmoe if name == "mmoe" else deep_moe)(x, P, pre=acts)
    assert tuple(y.shape) == tuple(G(pre + "/out").shape) == (MODEL_BATCH, 1)
    assert rel_err(y, G(pre + "/out")) <= 1e-6
    assert kink_margin(acts) >= KINK_MARGIN
    y.sum().backward()
    assert rel_err(x.grad, G(pre + "/gx")) <= 1e-5


@pytest.mark.parametrize("shape", MOE_SHAPES, ids=shape_tag)
def test_dropin_class_parity_with_the_reference(golden, shape):
    from torecsys_amd import layers as L
    G = golden("moe")
    B, N, E, X, Oi, Gn, hidden = shape
    pre = shape_tag(shape)
    m = L.MixtureOfExpertsLayer(expert_func=L.DNNLayer, **layer_kwargs(shape))
    assert list(m.state_dict().keys()) == G(pre + "/keys")
    assert list(m._modules) == ["experts", "gates"]
    assert isinstance(m.experts, nn.ModuleDict) and list(m.experts) == [f"Expert_{i}" for i in range(X)]
    assert isinstance(m.gates, nn.ModuleDict) and list(m.gates) == [f"Gate_{g}" for g in range(Gn)]
    for gate_mod in m.gates.values():
        assert isinstance(gate_mod, nn.Sequential) and list(gate_mod._modules) == ["Linear", "Softmax"]
        assert (gate_mod.Linear.in_features, gate_mod.Linear.out_features) == (N * E, X * Oi)
        assert isinstance(gate_mod.Softmax, nn.Softmax) and gate_mod.Softmax.dim == 1      # explicit: no implicit-dim warning
    assert all(type(ex) is L.MultilayerPerceptionLayer for ex in m.experts.values())
    assert m.inputs_size == {"inputs": ("B", "N", "E")}
    res = m.load_state_dict({k: G(f"{pre}/param/{k}") for k in G(pre + "/keys")}, strict=True)     # a reference checkpoint
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.gates.Gate_0.Linear.weight.detach(), G(pre + "/param/gates.Gate_0.Linear.weight"))


class _Recorder(nn.Module):
    """an expert that records its constructor keywords and returns ``width`` columns (or ``shape`` as it is)"""
    seen = []

    def __init__(self, width=3, shape=None, **kwargs):
        super().__init__()
        _Recorder.seen.append(dict(width=width, shape=shape, **kwargs))
        self.width, self.shape = width, shape
        self.lin = nn.Linear(1, 1)

    def forward(self, x):
        if self.shape is not None:
            return x.new_zeros(self.shape)
        return x.new_zeros(x.shape[0], self.width)


def test_alias_and_constructor_kwargs_forwarding():
    from torecsys_amd import layers as L
    assert L.MOELayer is L.MixtureOfExpertsLayer and L.MixtureOfExpertsLayer.__name__ == "MixtureOfExpertsLayer"
    _Recorder.seen = []
    m = L.MOELayer(12, 6, 2, _Recorder, expert_width=3, expert_tag="t", other=5, experts=7)
    # `expert_` is stripped, anything else is dropped; num_gates defaults to 1
    assert _Recorder.seen == [dict(width=3, shape=None, tag="t")] * 2
    assert list(m.gates) == ["Gate_0"] and list(m.experts) == ["Expert_0", "Expert_1"]
    assert list(m.state_dict().keys()) == ["experts.Expert_0.lin.weight", "experts.Expert_0.lin.bias",
                                           "experts.Expert_1.lin.weight", "experts.Expert_1.lin.bias",
                                           "gates.Gate_0.Linear.weight", "gates.Gate_0.Linear.bias"]
    m = L.MixtureOfExpertsLayer(inputs_size=8, output_size=4, num_experts=1, expert_func=L.DNNLayer, num_gates=3,
                                expert_inputs_size=8, expert_output_size=4, expert_layer_sizes=[5],
                                expert_dropout_p=[0.5], expert_activation=None)
    assert list(m.gates) == ["Gate_0", "Gate_1", "Gate_2"]
    assert list(m.experts.Expert_0.model._modules) == ["Linear_0", "Dropout_0", "LinearOutput"]
    assert m.experts.Expert_0.model.Dropout_0.p == 0.5


def test_the_two_value_errors_and_no_cpu_path():
    from torecsys_amd import functional as F_, layers as L
    # experts' widths (2 x 3) against the gates' output_size (8): both numbers in the message
    m = L.MOELayer(12, 8, 2, _Recorder, expert_width=3)
    with pytest.raises(ValueError, match=r"6 columns.*output_size = 8"):
        m(torch.zeros(4, 3, 4))
    # an expert that returns anything but (B, O)
    with pytest.raises(ValueError, match=r"Expert_0 must return \(4, O\), got \(4, 2, 3\)"):
        L.MOELayer(12, 6, 2, _Recorder, expert_shape=(4, 2, 3))(torch.zeros(4, 3, 4))
    with pytest.raises(ValueError, match=r"Expert_0 must return \(4, O\), got \(5, 3\)"):
        L.MOELayer(12, 6, 2, _Recorder, expert_shape=(5, 3))(torch.zeros(4, 3, 4))
    with pytest.raises(ValueError, match="expected"):
        L.MOELayer(12, 6, 2, _Recorder, expert_width=3)(torch.zeros(4, 12))
    # a CPU tensor reaches the kernel call and is refused there; the caller's tensor keeps its names (the reference
    # renames its argument in place)
    good = L.MOELayer(12, 6, 2, _Recorder, expert_width=3)
    for names in ((None, None, None), ("B", "N", "E"), ("X", "Y", "Z")):
        x = torch.zeros(4, 3, 4, names=names)
        with pytest.raises(RuntimeError, match="no CPU path"):
            good(x)
        assert x.names == names
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.moe_gate(torch.zeros(4, 12), torch.zeros(6, 12), torch.zeros(6), torch.zeros(4, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.moe_gate_forward_raw(torch.zeros(4, 6), None, torch.zeros(4, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.moe_gate_backward_raw(torch.zeros(4, 6), None, torch.zeros(4, 6), torch.zeros(4, 1, 6))
    # the raw calls read dense rows: a strided operand is refused, not misread
    with pytest.raises(ValueError, match="logits must be contiguous"):
        F_.moe_gate_forward_raw(torch.zeros(6, 4).t(), None, torch.zeros(4, 6))
    with pytest.raises(ValueError, match="experts must be contiguous"):
        F_.moe_gate_forward_raw(torch.zeros(4, 6), None, torch.zeros(4, 12)[:, ::2])
    with pytest.raises(ValueError, match="bias must be contiguous"):
        F_.moe_gate_forward_raw(torch.zeros(4, 6), torch.zeros(12)[::2], torch.zeros(4, 6))
    with pytest.raises(ValueError, match="gout must be contiguous"):
        F_.moe_gate_backward_raw(torch.zeros(4, 6), None, torch.zeros(4, 6), torch.zeros(4, 1, 12)[:, :, ::2])


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_moe_entries_validate_arguments_without_gpu(lib):
    from torecsys_amd import _abi, functional as F_
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    fwd, bwd = lib.trs_moe_gate_fwd, lib.trs_moe_gate_bwd
    # (logits, bias, experts, B, G, K, dtype, out, stream)
    assert fwd(null, null, null, 0, 2, 8, 0, null, null) == 0                       # B == 0: nothing is touched
    assert fwd(null, null, null, 0, 0, 0, 9, null, null) == 0
    assert fwd(null, one, one, 2, 2, 8, 0, one, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, one, null, 2, 2, 8, 0, one, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, one, one, 2, 2, 8, 0, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, null, one, 2, 2, 8, 7, one, null) == -2 and "dtype" in _abi.last_error()
    assert fwd(one, null, one, 2, 0, 8, 0, one, null) == -1 and "G=0" in _abi.last_error()
    assert fwd(one, null, one, 2, 2, 0, 0, one, null) == -1 and "K=0" in _abi.last_error()
    assert fwd(one, null, one, 2, 2, -4, 1, one, null) == -1 and "K=-4" in _abi.last_error()
    assert fwd(one, null, one, -1, 2, 8, 0, one, null) == -1 and "B=-1" in _abi.last_error()
    # (logits, bias, experts, gout, B, G, K, dtype, glogits, gexperts, stream)
    assert bwd(null, null, null, null, 0, 2, 8, 0, null, null, null) == 0
    for hole in range(5):
        ptrs = [one] * 5
        ptrs[hole] = null
        lo, ex, go, gl, ge = ptrs
        assert bwd(lo, one, ex, go, 2, 2, 8, 0, gl, ge, null) == -1 and "NULL" in _abi.last_error(), hole
    assert bwd(one, null, one, one, 2, 2, 8, 3, one, one, null) == -2 and "dtype" in _abi.last_error()
    assert bwd(one, null, one, one, 2, -1, 8, 0, one, one, null) == -1 and "G=-1" in _abi.last_error()
    assert bwd(one, null, one, one, 2, 2, 0, 1, one, one, null) == -1 and "K=0" in _abi.last_error()
    with pytest.raises(RuntimeError, match="trs_moe_gate_fwd failed"):
        _abi.call("trs_moe_gate_fwd", null, null, null, 2, 1, 4, 0, null, null)
    # the shape half of the vector path's rule, and the exported cap
    vs = lib.trs_moe_gate_vector_shape
    cap = F_.MOE_GATE_MAX_K
    assert cap % 8 == 0 and vs(cap, 0) == 1 and vs(cap, 1) == 1 and vs(cap + 8, 0) == 0 and vs(cap + 8, 1) == 0
    assert vs(4, 0) == 1 and vs(4, 1) == 0 and vs(8, 1) == 1 and vs(12, 0) == 1 and vs(12, 1) == 0
    assert vs(1, 0) == 0 and vs(15, 0) == 0 and vs(0, 0) == 0 and vs(-8, 1) == 0 and vs(8, 5) == 0
    assert vs(2 * cap + 3, 0) == 0
    # no launch has happened in this process: the record of the dispatched path is still empty
    assert lib.trs_moe_gate_last_path() == 0 and F_.moe_gate_last_path() == 0
    assert (F_.MOE_PATH_VECTOR, F_.MOE_PATH_ELEMENT) == (1, 2)


_MODELS_SRC = '''
import torch.nn as nn


class MMoE(nn.Module):
    """the layer structure of the reference's multi-gate model, over whatever the module-level names are bound to"""

    def __init__(self, inputs_size, num_experts, width, num_tasks):
        super().__init__()
        self.moe_layer = MOELayer(inputs_size=inputs_size, output_size=num_experts * width, num_gates=num_tasks,
                                  num_experts=num_experts, expert_func=DNNLayer, expert_inputs_size=inputs_size,
                                  expert_output_size=width, expert_layer_sizes=[8])
'''


def _standin(name, dropin, module):
    """a stand-in layer class with the drop-in's constructor and parameter layout, but a class of the stand-in package"""
    def __init__(self, *args, **kwargs):
        nn.Module.__init__(self)
        for n, c in dropin(*args, **kwargs)._modules.items():
            self.add_module(n, c)
    return type(name, (nn.Module,), {"__init__": __init__, "__module__": module})


def test_patch_rebinds_and_restores_both_names():
    import torecsys_amd
    from torecsys_amd import layers as L, patching
    # the four lists tests/test_host.py iterates are what they were; the two new names have a list of their own
    assert patching._LAYER_NAMES == [
        "FactorizationMachineLayer", "FMLayer", "FieldAwareFactorizationMachineLayer", "FFMLayer", "CrossNetworkLayer",
        "CompressInteractionNetworkLayer", "CINLayer", "InnerProductNetworkLayer", "OuterProductNetworkLayer",
        "AttentionalFactorizationMachineLayer", "AFMLayer", "BilinearInteractionLayer", "FieldAllTypeBilinear",
        "FieldEachTypeBilinear", "ComposeExcitationNetworkLayer", "CENLayer", "SqueezeAndExcitationNetworkLayer",
        "SENETLayer"]
    assert patching._MLP_NAMES == ["MultilayerPerceptionLayer", "DNNLayer", "DenseLayer", "FullyConnectLayer",
                                   "FeedForwardLayer"]
    assert patching._INPUT_NAMES == ["SingleIndexEmbedding", "MultiIndicesEmbedding", "MultiIndicesFieldAwareEmbedding",
                                     "ListIndicesEmbedding"]
    assert patching._ROUTER_NAMES == ["Inputs"]
    assert patching._MOE_NAMES == ["MixtureOfExpertsLayer", "MOELayer"]
    names = ["MixtureOfExpertsLayer", "MOELayer"]
    pkg = types.ModuleType("fake_moe_trs")
    lay = types.ModuleType("fake_moe_trs.layers")
    mdl = types.ModuleType("fake_moe_trs.models")
    old = _standin("MixtureOfExpertsLayer", L.MixtureOfExpertsLayer, lay.__name__)
    old_dnn = _standin("MultilayerPerceptionLayer", L.MultilayerPerceptionLayer, lay.__name__)
    for n in names:
        setattr(lay, n, old)                          # the alias shares the class, as in the reference
    lay.DNNLayer = old_dnn
    mdl.MOELayer, mdl.DNNLayer = old, old_dnn         # `from torecsys.layers import DNNLayer, MOELayer` copies
    exec(_MODELS_SRC, mdl.__dict__)
    pkg.layers, pkg.models = lay, mdl
    mods = (pkg, lay, mdl)
    for m in mods:
        sys.modules[m.__name__] = m
    try:
        before = mdl.MMoE(12, 3, 4, 2)
        assert type(before.moe_layer) is old
        torecsys_amd.patch(pkg, heads=False)
        for n in names:
            assert getattr(lay, n) is L.MixtureOfExpertsLayer, n
        assert mdl.MOELayer is L.MixtureOfExpertsLayer and mdl.DNNLayer is L.MultilayerPerceptionLayer
        after = mdl.MMoE(12, 3, 4, 2)
        assert type(after.moe_layer) is L.MixtureOfExpertsLayer
        assert type(after.moe_layer).__module__ == "torecsys_amd.layers"
        assert type(after.moe_layer.experts.Expert_0) is L.MultilayerPerceptionLayer
        assert list(after.state_dict().keys()) == list(before.state_dict().keys())
        assert list(after.state_dict().keys()) == ["moe_layer." + k for k in _expected_keys(3, 2, [8])]
        assert after.load_state_dict(before.state_dict(), strict=True).missing_keys == []
        torecsys_amd.unpatch()
        for n in names:
            assert getattr(lay, n) is old, n
        assert mdl.MOELayer is old and mdl.DNNLayer is old_dnn
        # mlp=False leaves the experts' class with the package, the mixture is still rebound
        torecsys_amd.patch(pkg, heads=False, mlp=False)
        assert mdl.MOELayer is L.MixtureOfExpertsLayer and mdl.DNNLayer is old_dnn
    finally:
        torecsys_amd.unpatch()
        for m in mods:
            sys.modules.pop(m.__name__, None)

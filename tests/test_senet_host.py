"""ComposeExcitationNetworkLayer (SENET / CEN), host side (no GPU): the plain torch restatement against the reference's
fixture (tests/golden/senet.npz), constructor / state_dict parity of the drop-in, patch() / unpatch(), argument validation
of the new C-ABI entries, error behaviour."""
import ctypes
import sys
import types

import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from senet_ref import (FAT_ARGS, FIBINET_ARGS, FIBINET_TYPES, MODEL_BATCH, PARAM_KEYS, SENET_SHAPES, compose,
                       compose_chunked, fat_deep_ffm, fibinet, fields, near_boundary, pre_activations, shape_tag)


def _params(G, pre, **kw):
    return [G(f"{pre}/param/{k}").clone().requires_grad_(**kw) for k in PARAM_KEYS]


@pytest.mark.parametrize("shape", SENET_SHAPES, ids=shape_tag)
def test_fixture_equals_the_plain_torch_composition(golden, shape):
    """mean over E -> Linear + ReLU -> Linear + ReLU -> re-weighting (senet_ref.compose) reproduces the reference's own
    outputs and gradients, fp32 <= 1e-6; so does its chunked, graph-free form the full-size GPU test uses."""
    G = golden("senet")
    B, N, E, r, squared = shape
    pre = shape_tag(shape)
    M = fields(N, squared)
    x = G(pre + "/x").clone().requires_grad_()
    ps = _params(G, pre)
    assert tuple(x.shape) == (B, M, E) and tuple(ps[0].shape) == (M // r, M) and tuple(ps[2].shape) == (M, M // r)
    assert G(pre + "/names") == ["B", "N", "E"] and G(pre + "/keys") == PARAM_KEYS
    y = compose(x, *ps)
    assert rel_err(y, G(pre + "/out")) <= 1e-6
    (y * G(pre + "/gout")).sum().backward()
    assert rel_err(x.grad, G(pre + "/gx")) <= 1e-6
    for k, p in zip(PARAM_KEYS, ps):
        assert rel_err(p.grad, G(f"{pre}/grad/{k}")) <= 1e-6, k
    # what the generator asserted: gates of both kinds, and no ReLU decision inside float noise
    _, u, v = pre_activations(x.detach(), *(p.detach() for p in ps))
    assert 0.2 <= float((v > 0).float().mean()) <= 0.8
    assert min(float(u.abs().min()), float(v.abs().min())) >= 1e-4
    assert not bool(near_boundary(x.detach(), *(p.detach() for p in ps)).any())
    out, gx, grads, terms, near = compose_chunked(x.detach(), *(p.detach() for p in ps), G(pre + "/gout"), chunk=5)
    assert not bool(near.any())
    assert rel_err(out, G(pre + "/out")) <= 1e-6 and rel_err(gx, G(pre + "/gx")) <= 1e-6
    for k, gr, t in zip(PARAM_KEYS, grads, terms):
        assert rel_err(gr, G(f"{pre}/grad/{k}")) <= 1e-6, k
        assert bool((t + 1e-30 >= gr.abs()).all())


@pytest.mark.parametrize("name", ["fibinet_" + k for k in FIBINET_TYPES] + ["fat_deep_ffm"])
def test_model_fixture_equals_the_plain_torch_composition(golden, name):
    """FiBiNET and FAT-DeepFFM restated over senet_ref.compose: output and input gradient of the reference models <= 1e-5
    (the bound the model fixtures get: their GEMMs are not bit-stable across host thread counts)."""
    G = golden("senet")
    pre = "model/" + name
    P = {k: G(f"{pre}/param/{k}") for k in G(pre + "/keys")}
    x = G(pre + "/x").clone().requires_grad_()
    if name == "fat_deep_ffm":
        assert tuple(x.shape) == (MODEL_BATCH, FAT_ARGS["num_fields"] ** 2, FAT_ARGS["embed_size"])
        y = fat_deep_ffm(x, P, FAT_ARGS["num_fields"])
    else:
        assert tuple(x.shape) == (MODEL_BATCH, FIBINET_ARGS["num_fields"], FIBINET_ARGS["embed_size"])
        y = fibinet(x, P, name.split("_")[1])
    assert tuple(y.shape) == tuple(G(pre + "/out").shape) == (MODEL_BATCH, 1)
    assert rel_err(y, G(pre + "/out")) <= 1e-5
    y.sum().backward()
    assert rel_err(x.grad, G(pre + "/gx")) <= 1e-5


@pytest.mark.parametrize("shape", SENET_SHAPES, ids=shape_tag)
def test_dropin_class_parity_with_the_reference(golden, shape):
    from torecsys_amd import layers as L
    G = golden("senet")
    B, N, E, r, squared = shape
    pre = shape_tag(shape)
    M = fields(N, squared)
    m = L.ComposeExcitationNetworkLayer(N, r, squared=squared)
    assert list(m.state_dict().keys()) == G(pre + "/keys") == PARAM_KEYS
    assert list(m._modules) == ["pooling", "fc"]
    # (named_children() would list the shared activation once)
    assert list(m.fc._modules) == ["ReductionLinear", "ReductionActivation", "AdditionLinear", "AdditionActivation"]
    assert len(list(m.fc)) == 4
    assert isinstance(m.pooling, nn.AdaptiveAvgPool1d) and m.pooling.output_size == 1
    assert m.fc.ReductionActivation is m.fc.AdditionActivation and type(m.fc.ReductionActivation) is nn.ReLU
    assert (m.fc.ReductionLinear.in_features, m.fc.ReductionLinear.out_features) == (M, M // r)
    assert (m.fc.AdditionLinear.in_features, m.fc.AdditionLinear.out_features) == (M // r, M)
    assert m.inputs_size == {"inputs": ("B", "N^2", "E")} and m.outputs_size == {"outputs": ("B", "N^2", "E")}
    # a reference checkpoint loads as it is
    res = m.load_state_dict({k: G(f"{pre}/param/{k}") for k in PARAM_KEYS}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.fc.AdditionLinear.weight.detach(), G(pre + "/param/fc.AdditionLinear.weight"))


def test_aliases_defaults_and_other_activations():
    from torecsys_amd import layers as L
    assert L.CENLayer is L.SENETLayer is L.SqueezeAndExcitationNetworkLayer is L.ComposeExcitationNetworkLayer
    assert L.ComposeExcitationNetworkLayer.__name__ == "ComposeExcitationNetworkLayer"
    m = L.SENETLayer(3, 2)                                        # squared defaults to True: M = 9, H = 4
    assert m.fc.ReductionLinear.weight.shape == (4, 9)
    act = nn.Sigmoid()
    m = L.CENLayer(5, 2, squared=False, activation=act)
    assert m.fc.ReductionActivation is act and m.fc.AdditionActivation is act
    m = L.SENETLayer(2, 3, squared=False)                         # H = 0 is legal, as in the reference
    assert m.fc.ReductionLinear.weight.shape == (0, 2) and m.fc.AdditionLinear.weight.shape == (2, 0)
    y = compose(torch.randn(2, 2, 4), *(p.detach() for p in m.parameters()))
    assert tuple(y.shape) == (2, 2, 4)


def test_cpu_tensors_and_wrong_field_counts_are_rejected():
    from torecsys_amd import functional as F_, layers as L
    m = L.SENETLayer(4, 2, squared=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 4, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        L.SENETLayer(4, 2, squared=False, activation=nn.Sigmoid())(torch.zeros(2, 4, 8))
    with pytest.raises(ValueError, match="expected 4 fields, got 5"):
        m(torch.zeros(2, 5, 8))
    with pytest.raises(ValueError, match="expected 16 fields, got 4"):
        L.CENLayer(4, 2)(torch.zeros(2, 4, 8))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.senet_squeeze(torch.zeros(2, 4, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.senet_scale(torch.zeros(2, 4, 8), torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.senet(torch.zeros(2, 4, 8), *m.parameters())
    assert F_.senet_fused_supported(torch.zeros(2, 4, 8), *m.parameters()) is False


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_senet_entries_validate_arguments_without_gpu(lib):
    from torecsys_amd import _abi
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    fwd, bwd = lib.trs_senet_fwd, lib.trs_senet_bwd
    # (x, W1, b1, W2, b2, B, M, H, E, dtype, out, gates, hidden, stream)
    assert fwd(null, one, one, one, one, 2, 4, 2, 8, 0, one, null, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, one, one, one, one, 2, 4, 2, 8, 7, one, null, null, null) == -2 and "dtype" in _abi.last_error()
    assert fwd(one, one, one, one, one, 2, 0, 0, 8, 0, one, null, null, null) == -1 and "M=0" in _abi.last_error()
    assert fwd(one, one, one, one, one, 2, 4, -1, 8, 0, one, null, null, null) == -1 and "H=-1" in _abi.last_error()
    assert fwd(one, one, one, one, one, 2, 4, 2, 8, 0, one, one, null, null) == -1 and "together" in _abi.last_error()
    assert fwd(one, one, one, one, one, 2, 4, 2, 10, 0, one, null, null, null) == -3 and "16-byte" in _abi.last_error()
    assert fwd(one, one, one, one, one, 2, 4, 2, 12, 1, one, null, null, null) == -3 and "16-byte" in _abi.last_error()
    assert fwd(one, one, one, one, one, 2, 65, 5, 8, 0, one, null, null, null) == -3 and "M <= 64" in _abi.last_error()
    assert fwd(one, one, one, one, one, 2, 4, 0, 8, 0, one, null, null, null) == -3      # H = 0: the general family's
    assert fwd(one, one, one, one, one, 2, 64, 8, 128, 0, one, null, null, null) == -3 and "registers" in _abi.last_error()
    assert fwd(ctypes.c_void_p(8), one, one, one, one, 2, 4, 2, 8, 0, one, null, null, null) == -4
    # (x, g, gates, hidden, W1, W2, B, M, H, E, dtype, dx, dW1, db1, dW2, db2, workspace, ws_bytes, stream)
    ws = lib.trs_senet_bwd_workspace_bytes(2, 4, 2)
    assert bwd(null, one, one, one, one, one, 2, 4, 2, 8, 0, one, one, one, one, one, one, ws, null) == -1
    assert "NULL" in _abi.last_error()
    assert bwd(one, one, one, one, one, one, 2, 4, 2, 8, 5, one, one, one, one, one, one, ws, null) == -2
    assert bwd(one, one, one, one, one, one, 2, 4, 2, 10, 0, one, one, one, one, one, one, ws, null) == -3
    assert "16-byte" in _abi.last_error()
    assert bwd(one, one, one, one, one, one, 2, 4, 2, 8, 0, one, one, one, one, one, one, ws - 1, null) == -6
    assert "workspace" in _abi.last_error()
    assert bwd(one, one, one, one, one, one, 2, 4, 2, 8, 0, one, null, null, one, null, null, 0, null) == -6
    # the workspace query: positive, non-decreasing in M and H
    q = lib.trs_senet_bwd_workspace_bytes
    assert q(65536, 39, 13) >= (2 * 39 * 13 + 39 + 13) * 4 > 0
    sizes = [[q(1024, M, H) for H in range(1, M + 1)] for M in range(1, 65)]
    assert all(s > 0 for row in sizes for s in row)
    assert all(a <= b for row in sizes for a, b in zip(row, row[1:]))                       # in H
    assert all(sizes[m][h] <= sizes[m + 1][h] for m in range(63) for h in range(m + 1))     # in M
    assert q(1024, 0, 0) == 0
    # the general family: (x, B, M, E, dtype, z, stream) / (x, a, B, M, E, dtype, out, stream) /
    # (x, g, a, gz, B, M, E, dtype, ga, dx, stream)
    assert lib.trs_senet_squeeze(null, 2, 400, 10, 0, one, null) == -1 and "NULL" in _abi.last_error()
    assert lib.trs_senet_squeeze(one, 2, 400, 10, 3, one, null) == -2 and "dtype" in _abi.last_error()
    assert lib.trs_senet_squeeze(one, 2, 0, 10, 0, one, null) == -1
    assert lib.trs_senet_scale_fwd(one, null, 2, 400, 10, 0, one, null) == -1 and "NULL" in _abi.last_error()
    assert lib.trs_senet_scale_fwd(one, one, 2, 400, 10, 9, one, null) == -2
    sb = lib.trs_senet_scale_bwd
    assert sb(one, one, null, null, 2, 400, 10, 0, null, null, null) == -1 and "NULL" in _abi.last_error()
    assert sb(null, one, null, null, 2, 400, 10, 0, one, null, null) == -1          # ga needs x
    assert sb(null, one, null, null, 2, 400, 10, 0, null, one, null) == -1          # dx = g * a needs a
    assert sb(one, one, one, one, 2, 400, 10, 4, one, one, null) == -2 and "dtype" in _abi.last_error()
    assert lib.trs_senet_fused_supported(39, 13, 64, 1) == 1 and lib.trs_senet_fused_supported(39, 13, 64, 0) == 1
    assert lib.trs_senet_fused_supported(64, 64, 16, 0) == 1 and lib.trs_senet_fused_supported(65, 13, 16, 0) == 0
    assert lib.trs_senet_fused_supported(5, 2, 10, 0) == 0 and lib.trs_senet_fused_supported(2, 0, 16, 0) == 0
    with pytest.raises(RuntimeError, match="trs_senet_fwd failed"):
        _abi.call("trs_senet_fwd", null, null, null, null, null, 2, 4, 2, 8, 0, null, null, null, null)


_MODELS_SRC = '''
import torch
import torch.nn as nn


class FiBiNET(nn.Module):
    """the layer structure of the reference's FiBiNET model, over whatever the module-level names are bound to"""

    def __init__(self, embed_size, num_fields, senet_reduction):
        super().__init__()
        self.senet = SENETLayer(num_fields, senet_reduction, squared=False)
        self.cen = CENLayer(num_fields, senet_reduction)
'''


def _standin(name, dropin, module):
    """a stand-in layer class with the drop-in's constructor and parameter layout, but a class of the stand-in package"""
    def __init__(self, *args, **kwargs):
        nn.Module.__init__(self)
        for n, c in dropin(*args, **kwargs)._modules.items():
            self.add_module(n, c)
    return type(name, (nn.Module,), {"__init__": __init__, "__module__": module})


def test_patch_rebinds_and_restores_the_four_names():
    import torecsys_amd
    from torecsys_amd import layers as L
    names = ["ComposeExcitationNetworkLayer", "CENLayer", "SqueezeAndExcitationNetworkLayer", "SENETLayer"]
    pkg = types.ModuleType("fake_senet_trs")
    lay = types.ModuleType("fake_senet_trs.layers")
    mdl = types.ModuleType("fake_senet_trs.models")
    old = _standin("ComposeExcitationNetworkLayer", L.ComposeExcitationNetworkLayer, lay.__name__)
    for n in names:
        setattr(lay, n, old)                          # aliases share one class, as in the reference
    mdl.SENETLayer = mdl.CENLayer = old               # `from torecsys.layers import SENETLayer, CENLayer` copies
    exec(_MODELS_SRC, mdl.__dict__)
    pkg.layers, pkg.models = lay, mdl
    mods = (pkg, lay, mdl)
    for m in mods:
        sys.modules[m.__name__] = m
    try:
        before = mdl.FiBiNET(16, 6, 3)
        assert type(before.senet) is old
        torecsys_amd.patch(pkg, heads=False)
        for n in names:
            assert getattr(lay, n) is L.ComposeExcitationNetworkLayer, n
        assert mdl.SENETLayer is L.ComposeExcitationNetworkLayer and mdl.CENLayer is L.ComposeExcitationNetworkLayer
        after = mdl.FiBiNET(16, 6, 3)
        assert type(after.senet) is L.ComposeExcitationNetworkLayer and type(after.senet).__module__ == "torecsys_amd.layers"
        assert type(after.cen) is L.ComposeExcitationNetworkLayer
        assert list(after.state_dict().keys()) == list(before.state_dict().keys())
        assert list(after.state_dict().keys()) == [f"{c}.{k}" for c in ("senet", "cen") for k in PARAM_KEYS]
        assert after.load_state_dict(before.state_dict(), strict=True).missing_keys == []
        torecsys_amd.unpatch()
        for n in names:
            assert getattr(lay, n) is old, n
        assert mdl.SENETLayer is old and mdl.CENLayer is old
    finally:
        torecsys_amd.unpatch()
        for m in mods:
            sys.modules.pop(m.__name__, None)

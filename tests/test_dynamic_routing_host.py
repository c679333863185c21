"""DynamicRoutingLayer (MIND behaviour-to-interest capsule routing), host side (no GPU): the plain torch restatement
against the reference's fixture (tests/golden/dynamic_routing.npz), the rule for the number of capsules, constructor /
state_dict parity of the drop-in, its default noise, patch() / unpatch(), argument validation of the new C-ABI entries."""
import ctypes
import sys
import types

import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from dynamic_routing_ref import (ROUTING_SHAPES, dynamic_routing, dynamic_routing_grads, num_caps, routing_state,
                                 shape_tag, squash)


@pytest.mark.parametrize("shape", ROUTING_SHAPES, ids=shape_tag)
def test_fixture_equals_the_plain_torch_restatement(golden, shape):
    """fp32 restatement with the recorded noise against the reference's own output and gradients: 1e-5 in the max norm,
    the project's fp32 contract"""
    G = golden("dynamic_routing")
    B, N, E, R, caps, iters = shape
    pre = shape_tag(shape)
    K = int(G(pre + "/num_caps")[0])
    assert K == num_caps(N, caps)
    assert G(pre + "/names") == ["B", "N", "O"] and G(pre + "/keys") == ["S"]
    x, S, noise, gout = G(pre + "/x"), G(pre + "/S"), G(pre + "/noise"), G(pre + "/gout")
    assert tuple(x.shape) == (B, N, E) and tuple(S.shape) == (E, R) and tuple(noise.shape) == (B, K, N, R)
    assert tuple(G(pre + "/out").shape) == tuple(gout.shape) == (B, K, R)
    out, gx, gS = dynamic_routing_grads(x, S, noise, iters, gout)
    errs = (rel_err(out, G(pre + "/out")), rel_err(gx, G(pre + "/gx")), rel_err(gS, G(pre + "/gS")))
    print(f"routing restatement {pre}: out {errs[0]:.2e} gx {errs[1]:.2e} gS {errs[2]:.2e}")
    assert max(errs) <= 1e-5, errs


def test_the_written_out_backward_equals_autograd():
    """what the backward kernel computes -- dpri = sum_k w dz with w a constant and dz the squash backward in closed form --
    against autograd through the restatement, in fp64"""
    B, N, E, R, K, iters = 5, 12, 8, 16, 3, 3
    g = torch.Generator().manual_seed(3)
    x = (0.3 * torch.randn(B, N, E, generator=g)).double().requires_grad_()
    S = torch.randn(E, R, generator=g).double().requires_grad_()
    noise = torch.randn(B, K, N, R, generator=g).double()
    gout = torch.randn(B, K, R, generator=g).double()
    out = dynamic_routing(x, S, noise, iters)
    gx, gS = torch.autograd.grad(out, (x, S), gout)
    pri = (x @ S).detach()
    c = routing_state(pri, noise, iters)
    w = torch.softmax(noise + c.unsqueeze(-1), dim=1)
    z = (w * pri.unsqueeze(1)).sum(dim=2)
    assert rel_err(squash(z), out) <= 1e-12
    n2 = (z * z).sum(-1, keepdim=True)
    s = n2.sqrt()
    den = (1 + n2) * (s + 1e-8)
    f = n2 / den
    f1 = ((s + 1e-8) - 0.5 * s * (1 + n2)) / den ** 2
    dz = f * gout + 2 * f1 * (gout * z).sum(-1, keepdim=True) * z
    dpri = (w * dz.unsqueeze(2)).sum(dim=1)
    assert rel_err(dpri @ S.detach().t(), gx) <= 1e-10
    assert rel_err(torch.einsum("bne,bnr->er", x.detach(), dpri), gS) <= 1e-10


@pytest.mark.parametrize("N,want", [(1, 1), (2, 1), (3, 1), (4, 2), (7, 2), (8, 3), (50, 5), (64, 6)])
def test_number_of_capsules(N, want):
    from torecsys_amd import layers as L
    m = L.DynamicRoutingLayer(4, 4, 8, 3)
    assert m._dynamic_interest_number(N) == want == num_caps(N, 8)
    for cap in (1, 2, 4):
        assert L.DynamicRoutingLayer(4, 4, cap, 3)._dynamic_interest_number(N) == min(want, cap) == num_caps(N, cap)


def test_dropin_class_parity_with_the_reference(golden):
    import torecsys_amd
    from torecsys_amd import layers as L
    assert torecsys_amd.DynamicRoutingLayer is L.DynamicRoutingLayer
    G = golden("dynamic_routing")
    for shape in ROUTING_SHAPES:
        B, N, E, R, caps, iters = shape
        pre = shape_tag(shape)
        m = L.DynamicRoutingLayer(embed_size=E, routed_size=R, max_num_caps=caps, num_iter=iters)
        assert list(m.state_dict().keys()) == G(pre + "/keys") == ["S"]
        assert isinstance(m.S, nn.Parameter) and tuple(m.S.shape) == (E, R)
        assert (m.max_num_caps, m.num_iter, m.num_caps) == (caps, iters, None)
        assert m.inputs_size == {"inputs": ("B", "N", "E")}
        assert m.outputs_size == {"inputs": ("B", "Number of Caps", "Routed Size")}
        res = m.load_state_dict({"S": G(pre + "/S")}, strict=True)          # a reference checkpoint
        assert not res.missing_keys and not res.unexpected_keys and torch.equal(m.S.detach(), G(pre + "/S"))
    # positional constructor, S = randn from the global generator as in the reference
    torch.manual_seed(11)
    m = L.DynamicRoutingLayer(6, 5, 4, 3)
    torch.manual_seed(11)
    assert torch.equal(m.S.detach(), torch.randn(6, 5))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_default_noise_is_randn_of_the_noise_shape(dtype):
    """on the CPU the module runs the ATen composition: without ``noise`` it equals the same module with
    ``torch.randn(B, K', N, R)`` drawn after the same seed, bit for bit, and leaves the generator where that draw does"""
    from torecsys_amd import layers as L
    B, N, E, R = 4, 12, 8, 16
    m = L.DynamicRoutingLayer(E, R, 4, 3).to(dtype)
    x = (0.3 * torch.randn(B, N, E)).to(dtype)
    torch.manual_seed(5)
    y = m(x)
    after = torch.get_rng_state()
    assert m.num_caps == 3 and y.names == ("B", "N", "O") and tuple(y.shape) == (B, 3, R) and not x.has_names()
    torch.manual_seed(5)
    noise = torch.randn(B, 3, N, R, dtype=dtype)
    assert torch.equal(torch.get_rng_state(), after)
    y2 = m(x, noise)
    assert torch.equal(y.rename(None), y2.rename(None))
    if dtype == torch.float32:          # and that composition is the restatement
        assert rel_err(y.rename(None), dynamic_routing(x, m.S.detach(), noise, 3)) <= 1e-5
    with pytest.raises(ValueError, match="noise"):
        m(x, noise[:, :2])
    with pytest.raises(ValueError, match="expected"):
        m(x[0])


def test_golden_through_the_module_on_the_cpu(golden):
    """the ATen composition the module keeps off the kernels' envelope reproduces the fixture, gradients included"""
    from torecsys_amd import layers as L
    G = golden("dynamic_routing")
    for shape in ROUTING_SHAPES:
        B, N, E, R, caps, iters = shape
        pre = shape_tag(shape)
        m = L.DynamicRoutingLayer(E, R, caps, iters)
        m.load_state_dict({"S": G(pre + "/S")})
        x = G(pre + "/x").requires_grad_()
        y = m(x, G(pre + "/noise"))
        assert m.num_caps == int(G(pre + "/num_caps")[0]) and y.names == ("B", "N", "O")
        (y.rename(None) * G(pre + "/gout")).sum().backward()
        assert rel_err(y.rename(None), G(pre + "/out")) <= 1e-5
        assert rel_err(x.grad, G(pre + "/gx")) <= 1e-5 and rel_err(m.S.grad, G(pre + "/gS")) <= 1e-5


def test_functional_validation_without_gpu():
    from torecsys_amd import functional as F_
    x, S, noise = torch.zeros(4, 6, 8), torch.zeros(8, 16), torch.zeros(4, 2, 6, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.dynamic_routing(x, S, noise, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.dynamic_routing_forward_raw(torch.zeros(4, 6, 16), noise, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.dynamic_routing_backward_raw(noise, torch.zeros(4, 2, 6), torch.zeros(4, 2, 16), torch.zeros(4, 2, 16))
    with pytest.raises(ValueError, match="expected"):
        F_.dynamic_routing(x[0], S, noise, 3)
    with pytest.raises(ValueError, match="expected"):
        F_.dynamic_routing(x, torch.zeros(7, 16), noise, 3)
    # the raw calls read dense rows: a strided operand is refused, not misread
    with pytest.raises(ValueError, match="priors must be contiguous"):
        F_.dynamic_routing_forward_raw(torch.zeros(4, 6, 32)[:, :, ::2], noise, 3)
    with pytest.raises(ValueError, match="noise must be contiguous"):
        F_.dynamic_routing_forward_raw(torch.zeros(4, 6, 16), torch.zeros(4, 2, 6, 32)[..., ::2], 3)
    with pytest.raises(ValueError, match="gout must be contiguous"):
        F_.dynamic_routing_backward_raw(noise, torch.zeros(4, 2, 6), torch.zeros(4, 2, 16), torch.zeros(4, 2, 32)[..., ::2])
    assert (F_.ROUTING_PATH_VECTOR, F_.ROUTING_PATH_ELEMENT) == (1, 2)


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_routing_entries_validate_arguments_without_gpu(lib):
    from torecsys_amd import _abi, functional as F_
    for name in ("trs_dynamic_routing_path", "trs_dynamic_routing_fwd", "trs_dynamic_routing_bwd"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    assert lib.trs_version() == 3
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    fwd, bwd, path = lib.trs_dynamic_routing_fwd, lib.trs_dynamic_routing_bwd, lib.trs_dynamic_routing_path
    # (priors, noise, B, N, R, K, num_iter, dtype, out, c_out, z_out, stream)
    assert fwd(null, null, 0, 50, 64, 5, 3, 0, null, null, null, null) == 0          # B == 0: nothing is touched
    assert fwd(null, null, 0, 0, 0, 0, 0, 9, null, null, null, null) == 0
    assert fwd(null, one, 2, 50, 64, 5, 3, 0, one, null, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, null, 2, 50, 64, 5, 3, 0, one, null, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, one, 2, 50, 64, 5, 3, 0, null, null, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, one, 2, 50, 64, 5, 3, 0, one, one, null, null) == -1 and "together" in _abi.last_error()
    assert fwd(one, one, 2, 50, 64, 5, 3, 7, one, null, null, null) == -2 and "dtype" in _abi.last_error()
    assert fwd(one, one, -1, 50, 64, 5, 3, 0, one, null, null, null) == -1 and "B=-1" in _abi.last_error()
    assert fwd(one, one, 2, 129, 64, 5, 3, 0, one, null, null, null) == -3 and "N=129" in _abi.last_error()
    assert fwd(one, one, 2, 0, 64, 5, 3, 0, one, null, null, null) == -3 and "N=0" in _abi.last_error()
    assert fwd(one, one, 2, 50, 130, 5, 3, 1, one, null, null, null) == -3 and "R=130" in _abi.last_error()
    assert fwd(one, one, 2, 50, 64, 9, 3, 1, one, null, null, null) == -3 and "K=9" in _abi.last_error()
    assert fwd(one, one, 2, 50, 64, 0, 3, 1, one, null, null, null) == -3 and "K=0" in _abi.last_error()
    assert fwd(one, one, 2, 50, 64, 5, 0, 0, one, null, null, null) == -1 and "num_iter=0" in _abi.last_error()
    # (noise, c, z, gout, B, N, R, K, dtype, dpri, stream)
    assert bwd(null, null, null, null, 0, 50, 64, 5, 0, null, null) == 0
    for hole in range(5):
        ptrs = [one] * 5
        ptrs[hole] = null
        nz, c, z, go, dp = ptrs
        assert bwd(nz, c, z, go, 2, 50, 64, 5, 0, dp, null) == -1 and "NULL" in _abi.last_error(), hole
    assert bwd(one, one, one, one, 2, 50, 64, 5, 3, one, null) == -2 and "dtype" in _abi.last_error()
    assert bwd(one, one, one, one, 2, 200, 64, 5, 0, one, null) == -3 and "N=200" in _abi.last_error()
    assert bwd(one, one, one, one, 2, 50, 64, 12, 1, one, null) == -3 and "K=12" in _abi.last_error()
    with pytest.raises(RuntimeError, match="trs_dynamic_routing_fwd failed"):
        _abi.call("trs_dynamic_routing_fwd", null, null, 2, 50, 64, 5, 3, 0, null, null, null, null)
    # the path function: 0 none, 1 rows of whole 16-byte vectors, 2 element loads
    assert path(50, 64, 5, 1) == 1 and path(50, 64, 5, 0) == 1
    assert path(7, 5, 2, 0) == 2 and path(7, 5, 2, 1) == 2
    assert path(129, 64, 5, 1) == 0 and path(129, 64, 5, 0) == 0
    assert path(50, 4, 5, 0) == 1 and path(50, 4, 5, 1) == 2 and path(50, 8, 5, 1) == 1 and path(33, 40, 5, 1) == 1
    assert path(128, 128, 8, 0) == 1 and path(128, 132, 8, 0) == 0 and path(1, 1, 1, 1) == 2
    assert path(50, 64, 9, 0) == 0 and path(50, 64, 0, 0) == 0 and path(0, 64, 5, 0) == 0 and path(50, 64, 5, 4) == 0
    assert F_.dynamic_routing_path(50, 64, 5, torch.bfloat16) == F_.ROUTING_PATH_VECTOR
    assert F_.dynamic_routing_path(7, 5, 2, torch.float32) == F_.ROUTING_PATH_ELEMENT
    assert F_.dynamic_routing_path(129, 64, 5, torch.float32) == 0
    assert F_.dynamic_routing_path(50, 64, 5, torch.float16) == 0


_MODELS_SRC = '''
import torch.nn as nn


class Interests(nn.Module):
    """a user tower over whatever the module-level name is bound to"""

    def __init__(self, embed_size, routed_size):
        super().__init__()
        self.routing = DynamicRoutingLayer(embed_size, routed_size, max_num_caps=4, num_iter=3)
'''


def test_patch_rebinds_and_restores_the_routing_layer():
    import torecsys_amd
    from torecsys_amd import layers as L, patching
    assert patching._ROUTING_NAMES == ["DynamicRoutingLayer"]
    assert "DynamicRoutingLayer" not in patching._LAYER_NAMES + patching._MLP_NAMES + patching._MOE_NAMES
    pkg = types.ModuleType("fake_routing_trs")
    lay = types.ModuleType("fake_routing_trs.layers")
    mdl = types.ModuleType("fake_routing_trs.models")

    def __init__(self, embed_size, routed_size, max_num_caps, num_iter):
        nn.Module.__init__(self)
        self.S = nn.Parameter(torch.randn(embed_size, routed_size))

    old = type("DynamicRoutingLayer", (nn.Module,), {"__init__": __init__, "__module__": lay.__name__})
    lay.DynamicRoutingLayer = old
    mdl.DynamicRoutingLayer = old          # `from torecsys.layers import DynamicRoutingLayer` copies
    exec(_MODELS_SRC, mdl.__dict__)
    pkg.layers, pkg.models = lay, mdl
    mods = (pkg, lay, mdl)
    for m in mods:
        sys.modules[m.__name__] = m
    try:
        before = mdl.Interests(8, 16)
        assert type(before.routing) is old
        torecsys_amd.patch(pkg, heads=False)
        assert lay.DynamicRoutingLayer is L.DynamicRoutingLayer and mdl.DynamicRoutingLayer is L.DynamicRoutingLayer
        after = mdl.Interests(8, 16)
        assert type(after.routing) is L.DynamicRoutingLayer
        assert list(after.state_dict().keys()) == list(before.state_dict().keys()) == ["routing.S"]
        assert after.load_state_dict(before.state_dict(), strict=True).missing_keys == []
        torecsys_amd.unpatch()
        assert lay.DynamicRoutingLayer is old and mdl.DynamicRoutingLayer is old
    finally:
        torecsys_amd.unpatch()
        for m in mods:
            sys.modules.pop(m.__name__, None)

"""The kernels of csrc/senet.hip against float64 autograd BIT FOR BIT: senet_fwd_kernel / senet_bwd_kernel at all seven
vectors-per-lane steps in both dtypes, the backward's three wave counts, slab counts that leave segments of
senet_finish_kernel empty or short, a wave's second sample; senet_rowsum_kernel / senet_rowscale_kernel at every group
width, on element rows, from an unaligned pointer and on a second trip; and a whole general-family layer.

tests/gate_exact_ref.py makes the operands (sparse integers, parameters in [-1, 1]: every value of the layer a multiple
of 1 / E), tests/test_gate_exact_host.py holds every sum below 2**24 quanta and the cases to the conditions that keep them
from being degenerate: a fifth to four fifths of the hidden units and of the gates live, pre-activations of exactly 0 in
both layers, a dead hidden unit beside live ones, no parameter gradient zero.  The reference is senet_ref.compose under
autograd: torch.relu has derivative 0 at 0, which is what the kernels' ``a > 0.f``, ``hv > 0.f`` and the ``hh == 0.f`` skip
give.  Nothing is left out of any comparison: out, dx, dW1, db1, dW2, db2, whole tensors, ``torch.equal``."""
import pytest
import torch

import gate_exact_ref as R

pytestmark = pytest.mark.gpu

F32, BF16, F64 = R.F32, R.BF16, R.F64
KEYS = ("fc.ReductionLinear.weight", "fc.ReductionLinear.bias", "fc.AdditionLinear.weight", "fc.AdditionLinear.bias")
GRADS = ("dW1", "db1", "dW2", "db2")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


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


def _layer(dev, o):
    """a SENETLayer of M fields and H hidden units holding the case's parameters"""
    from torecsys_amd.layers import SENETLayer
    m = SENETLayer(o.M, 1, squared=False)
    m.fc.ReductionLinear = torch.nn.Linear(o.M, o.H)
    m.fc.AdditionLinear = torch.nn.Linear(o.H, o.M)
    m.load_state_dict(dict(zip(KEYS, (o.W1, o.b1, o.W2, o.b2))), strict=True)
    return m.to(dev).to(o.dtype)


def _params(m):
    return [dict(m.named_parameters())[k] for k in KEYS]


def _fused_rule(M, H, E, dtype):
    """M <= 64 fields, 1 <= H <= M, rows of whole 16-byte vectors, a sample of at most 16 KiB"""
    row = E * (4 if dtype == F32 else 2)
    return M <= 64 and 1 <= H <= M and row % 16 == 0 and M * row <= 16384


def _run_fused(dev, case, calls):
    from torecsys_amd import functional as F_
    o = R.senet_case(*case)
    r = R.senet_ref(o)
    where = f"senet {R.senet_id(case)} [K {R.senet_vec_per_lane(o.M, o.E, o.dtype)}, " \
            f"nw {R.senet_bwd_waves(o.M, o.H, o.E, o.dtype)}]:"
    assert _fused_rule(o.M, o.H, o.E, o.dtype)
    m = _layer(dev, o)
    x = o.x.to(o.dtype).to(dev).requires_grad_()
    assert F_.senet_fused_supported(x, *_params(m))
    out = F_.senet(x, *_params(m))
    out.backward(o.gout.to(o.dtype).to(dev))
    torch.cuda.synchronize()
    assert calls == ["trs_senet_fwd", "trs_senet_bwd"], calls
    d = R.Diffs()
    d.check(where, "out", out.detach(), r.out)
    d.check(where, "dx", x.grad, r.dx)
    for name, p in zip(GRADS, _params(m)):
        d.check(where, name, p.grad, getattr(r, name))
    return o, r, m, d


@pytest.mark.parametrize("case", R.SENET_STEP_CASES, ids=R.senet_id)
def test_fused_every_step_exact(dev, calls, case):
    """K = 1, 2, 4, 5, 8, 10, 16 vectors per lane, M and H of every residue modulo 4 (the zero-padded quads of the LDS
    weights), H from 1 to M, E without a power of two"""
    _run_fused(dev, case, calls)[3].done()


@pytest.mark.parametrize("case", R.SENET_WAVE_CASES, ids=R.senet_id)
def test_fused_backward_wave_counts_exact(dev, calls, case):
    """64 x 64 hidden units: one wave per workgroup and more than 64 KiB of dynamic LDS; 64 x 32: two waves"""
    o, _, _, d = _run_fused(dev, case, calls)
    assert R.senet_bwd_waves(o.M, o.H, o.E, o.dtype) == (1 if o.H == 64 else 2)
    d.done()


@pytest.mark.parametrize("case", R.SENET_SLAB_CASES, ids=R.senet_id)
def test_fused_slab_counts_exact(dev, calls, case):
    """1, 1, 2, 7, 8, 9 and 17 slabs: the finish kernel's eight segments are partly empty, full, and short at the end"""
    _run_fused(dev, case, calls)[3].done()


@pytest.mark.parametrize("case", R.SENET_TRIP_CASES, ids=R.senet_id)
def test_fused_second_sample_exact(dev, calls, case):
    """8197 samples: past the 8192 a resident forward grid holds and the 4096 of the backward's 1024 workgroups, so a
    wave's LDS strips are re-used and its accumulators carry on"""
    assert case[4] > 8 * 256 * 4 and case[4] > 1024 * 4
    _run_fused(dev, case, calls)[3].done()


@pytest.mark.parametrize("case", R.SENET_PARTIAL_CASES, ids=R.senet_id)
def test_fused_partial_gradients_and_no_grad_exact(dev, case):
    """the input gradient alone (no slabs, no finish kernel), the parameter gradients alone (dx NULL), and a forward
    that keeps neither gates nor hidden activations"""
    from torecsys_amd import functional as F_
    o = R.senet_case(*case)
    r = R.senet_ref(o)
    where = f"senet {R.senet_id(case)}"
    d = R.Diffs()
    g = o.gout.to(o.dtype).to(dev)
    m = _layer(dev, o)
    x = o.x.to(o.dtype).to(dev).requires_grad_()
    F_.senet(x, *[p.detach() for p in _params(m)]).backward(g)
    d.check(where, "dx (input only)", x.grad, r.dx)
    assert all(p.grad is None for p in _params(m))
    out = F_.senet(x.detach(), *_params(m))
    out.backward(g)
    d.check(where, "out (parameters only)", out.detach(), r.out)
    for name, p in zip(GRADS, _params(m)):
        d.check(where, name + " (parameters only)", p.grad, getattr(r, name))
    m2 = _layer(dev, o)
    for p in _params(m2)[2:]:
        p.requires_grad_(False)
    F_.senet(x.detach(), *_params(m2)).backward(g)
    d.check(where, "dW1 (first layer only)", _params(m2)[0].grad, r.dW1)
    d.check(where, "db1 (first layer only)", _params(m2)[1].grad, r.db1)
    with torch.no_grad():
        out = m(x)
    assert not out.requires_grad
    d.check(where, "out (no_grad)", out.rename(None), r.out)
    torch.cuda.synchronize()
    d.done()


# ---------------------------------------------------------------------------------------------------------------------
# general family
# ---------------------------------------------------------------------------------------------------------------------
def _place(t, off):
    """``t`` on the device, ``off``: one element (4 bytes of fp32) past a 16-byte boundary"""
    if not off:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


@pytest.mark.parametrize("case", R.SENET_ROW_CASES, ids=R.senet_row_id)
def test_squeeze_and_scale_exact(dev, case):
    """z, out, ga, and the input gradient in its three forms: from senet_scale alone (g a), from senet_squeeze alone
    (gz / E) and, with a SENetLink, written once as g a + gz / E"""
    from torecsys_amd import functional as F_
    dtype, E, B, M, off = case
    o = R.senet_row_case(*case)
    vec, units, lg = R.senet_row_path(E, dtype, aligned=not off)
    where = f"senet rows {R.senet_row_id(case)} [{'vector' if vec else 'element'}, lg {lg}]:"
    d = R.Diffs()
    up = lambda t, dt=dtype: t.to(dt).to(dev)                                 # noqa: E731
    g, gz = up(o.gout), up(o.gz, F32)
    for link in (None, F_.SENetLink()):
        tag = "" if link is None else " (link)"
        x = _place(up(o.x), off).requires_grad_()
        a = up(o.a, F32).requires_grad_()
        z = F_.senet_squeeze(x, link)
        out = F_.senet_scale(x, a, link)
        assert z.dtype == F32 and out.dtype == dtype
        d.check(where, "z" + tag, z.detach(), o.z)
        d.check(where, "out" + tag, out.detach(), o.out)
        if link is None:
            out.backward(g)
            d.check(where, "ga", a.grad, o.ga)
            d.check(where, "dx of senet_scale", x.grad, o.dx_scale)
            x.grad = None
            z.backward(gz)
            d.check(where, "dx of senet_squeeze", x.grad, o.dx_squeeze)
        else:
            torch.autograd.backward([z, out], [gz, g])
            d.check(where, "ga (link)", a.grad, o.ga)
            d.check(where, "dx (link): g a + gz / E written once", x.grad, o.dx)
    torch.cuda.synchronize()
    d.done()


@pytest.mark.parametrize("case", R.SENET_LAYER_CASES, ids=R.senet_layer_id)
def test_general_family_layer_exact(dev, calls, case):
    """65 fields are past the fused family: squeeze, an fp32 excitation in ATen (13 hidden units, or none: gates relu(b2))
    and the re-weighting.  bf16 modules stay exact as well: the layer runs the excitation on ``weight.float()`` from fp32
    means, and the parameter gradients are rounded once on their way back through the cast"""
    from torecsys_amd.layers import SENETLayer
    dtype, M, reduction, E, B = case
    o = R.senet_layer_case(*case)
    r = R.senet_ref(o)
    m = SENETLayer(M, reduction, squared=False)
    assert m.fc.ReductionLinear.out_features == o.H
    m.load_state_dict(dict(zip(KEYS, (o.W1, o.b1, o.W2, o.b2))), strict=True)
    m = m.to(dev).to(dtype)
    x = o.x.to(dtype).to(dev).requires_grad_()
    out = m(x).rename(None)
    out.backward(o.gout.to(dtype).to(dev))
    torch.cuda.synchronize()
    assert "trs_senet_squeeze" in calls and "trs_senet_scale_fwd" in calls and "trs_senet_fwd" not in calls
    where = f"senet layer {R.senet_id((dtype, M, o.H, E, B))}:"
    d = R.Diffs()
    d.check(where, "out", out.detach(), r.out)
    d.check(where, "dx", x.grad, r.dx)
    for name, p in zip(GRADS, _params(m)):
        assert p.grad.dtype == dtype
        d.check(where, name, p.grad, getattr(r, name))
    d.done()

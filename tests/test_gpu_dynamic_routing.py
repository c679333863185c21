"""GPU parity of DynamicRoutingLayer and functional.dynamic_routing* (csrc/dynamic_routing.hip): against the reference's
own outputs and gradients (tests/golden/dynamic_routing.npz) and, at sizes the fixture does not hold, against the plain
torch restatement run on the CPU in fp64 on the SAME dtype-rounded x, S and noise (tests/dynamic_routing_ref.py, pinned to
the fixture by tests/test_dynamic_routing_host.py) -- never against the ATen composition on the device.  Tolerances are the
project's own for num_iter <= 3: fp32 1e-5, bf16 1e-2, in conftest.rel_err_both (max norm and per-sample norm) for the
output and the gradient of x, in the max norm for the gradient of S.  The bf16 bound rests on the priors being the GEMM's
fp32 result and on the kernels rounding nothing between their loads and their final stores."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import rel_err, rel_err_both
from dynamic_routing_ref import (EXTRA_SHAPES, FIVE_ITER_SHAPE, ROUTING_SHAPES, X_SCALE, dynamic_routing_grads,
                                 make_inputs, num_caps, shape_tag)

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
DTYPES = [torch.float32, torch.bfloat16]
ALL_SHAPES = ROUTING_SHAPES + [s for s in EXTRA_SHAPES if s not in ROUTING_SHAPES]
FWD, BWD = "trs_dynamic_routing_fwd", "trs_dynamic_routing_bwd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dt(d):
    return "fp32" if d == torch.float32 else "bf16"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
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


def _expected_path(R, dtype):
    """rows of whole 16-byte vectors (written out here, not taken from the library)"""
    return 1 if (R * (4 if dtype == torch.float32 else 2)) % 16 == 0 else 2


_REF = {}


def _case(shape, dtype):
    """inputs of a case (fp32 images of values representable in ``dtype``) and the fp64 restatement on them, computed
    once and shared; callers leave them unchanged"""
    key = (shape, dtype)
    if key not in _REF:
        x, S, noise, gout = make_inputs(shape, dtype)
        ref = dynamic_routing_grads(x.double(), S.double(), noise.double(), shape[5], gout.double())
        _REF[key] = (x, S, noise, gout, ref)
    return _REF[key]


def _run(dev, dtype, x, S, noise, gout, iters):
    from torecsys_amd import functional as F_
    xd, Sd = (t.to(dev).to(dtype).requires_grad_() for t in (x, S))
    out = F_.dynamic_routing(xd, Sd, noise.to(dev).to(dtype), iters)
    gx, gS = torch.autograd.grad(out, (xd, Sd), gout.to(dev).to(dtype))
    assert out.dtype == gx.dtype == gS.dtype == dtype
    return out.detach(), gx, gS


def _errs(got, ref):
    (out, gx, gS), (rout, rgx, rgS) = got, ref
    assert out.shape == rout.shape and gx.shape == rgx.shape and gS.shape == rgS.shape
    assert all(bool(torch.isfinite(t).all()) for t in got)
    return (rel_err_both(out.float().cpu(), rout), rel_err_both(gx.float().cpu(), rgx), rel_err(gS.float().cpu(), rgS))


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("shape", ROUTING_SHAPES, ids=shape_tag)
def test_routing_layer_golden(golden, dev, calls, shape):
    from torecsys_amd import functional as F_, layers as L
    G = golden("dynamic_routing")
    B, N, E, R, caps, iters = shape
    pre = shape_tag(shape)
    m = L.DynamicRoutingLayer(embed_size=E, routed_size=R, max_num_caps=caps, num_iter=iters).to(dev)
    assert list(m.state_dict().keys()) == G(pre + "/keys")
    m.load_state_dict({"S": G(pre + "/S")}, strict=True)
    x = G(pre + "/x").to(dev).requires_grad_()
    out = m(x, G(pre + "/noise").to(dev))
    K = int(G(pre + "/num_caps")[0])
    assert m.num_caps == K and F_.dynamic_routing_path(N, R, K, torch.float32) == _expected_path(R, torch.float32)
    assert calls.count(FWD) == 1
    assert out.names == tuple(G(pre + "/names")) == ("B", "N", "O") and not x.has_names()
    y = out.rename(None)
    (y * G(pre + "/gout").to(dev)).sum().backward()
    assert calls.count(BWD) == 1
    errs = (rel_err_both(y.cpu(), G(pre + "/out")), rel_err_both(x.grad.cpu(), G(pre + "/gx")),
            rel_err(m.S.grad.cpu(), G(pre + "/gS")))
    print(f"routing golden {pre}: out {errs[0]:.2e} gx {errs[1]:.2e} gS {errs[2]:.2e}")
    assert max(errs) <= 1e-5, errs


# ------------------------------------------------------------------------------------------------ the restatement, fp64
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=shape_tag)
def test_routing_against_the_fp64_restatement(dev, calls, shape, dtype):
    from torecsys_amd import functional as F_
    B, N, E, R, caps, iters = shape
    K = num_caps(N, caps)
    assert F_.dynamic_routing_path(N, R, K, dtype) == _expected_path(R, dtype)
    x, S, noise, gout, ref = _case(shape, dtype)
    got = _run(dev, dtype, x, S, noise, gout, iters)
    assert calls == [FWD, BWD]
    errs = _errs(got, ref)
    print(f"routing {shape_tag(shape)} K'={K} {_dt(dtype)}: out {errs[0]:.2e} gx {errs[1]:.2e} gS {errs[2]:.2e}")
    assert max(errs) <= TOL[dtype], errs


def test_five_iterations_fp32(dev):
    """(8, 50, 64, 64, 8, 5): the routing amplifies rounding with every iteration, so the bound is taken from the fp32
    restatement itself: max(1e-5, 4 x its error against fp64 on the same inputs, computed here).  The factor is for a
    different summation order and exp.  Observed on an MI355X: out 1.30e-06, gx 5.19e-06, gS 8.94e-07 against the bound
    5.00e-05 (CPU fp32 restatement 1.25e-05 in the same norms)."""
    shape = FIVE_ITER_SHAPE
    x, S, noise, gout, ref = _case(shape, torch.float32)
    cpu32 = dynamic_routing_grads(x, S, noise, shape[5], gout)
    base = max(rel_err_both(cpu32[0], ref[0]), rel_err_both(cpu32[1], ref[1]), rel_err(cpu32[2], ref[2]))
    bound = max(1e-5, 4.0 * base)
    errs = _errs(_run(dev, torch.float32, x, S, noise, gout, shape[5]), ref)
    print(f"routing 5 iterations fp32: out {errs[0]:.2e} gx {errs[1]:.2e} gS {errs[2]:.2e}; CPU fp32 restatement "
          f"{base:.2e}, bound {bound:.2e}")
    assert max(errs) <= bound, (errs, bound)          # observed 5.19e-06 <= 5.00e-05


# ------------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("N", [1, 2])
def test_one_capsule_does_not_see_the_noise(dev, dtype, N):
    """K' = 1: the softmax over one capsule is 1 whatever the noise -- bit-identical output and gradients"""
    shape = (5, N, 8, 8, 4, 3)
    assert num_caps(N, 4) == 1
    x, S, noise, gout = make_inputs(shape, dtype)
    a = _run(dev, dtype, x, S, noise, gout, 3)
    b = _run(dev, dtype, x, S, 3.0 * torch.randn(noise.shape, generator=torch.Generator().manual_seed(1)) + 1.0, gout, 3)
    for name, s, t in zip(("out", "gx", "gS"), a, b):
        assert torch.equal(s, t), name
    assert float(a[0].abs().max()) > 0


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", [(16, 50, 64, 64, 4, 3), (7, 33, 24, 40, 8, 2), (4099, 12, 16, 16, 3, 2)], ids=shape_tag)
def test_two_runs_are_bit_identical(dev, shape, dtype):
    x, S, noise, gout, _ = _case(shape, dtype)
    a = _run(dev, dtype, x, S, noise, gout, shape[5])
    b = _run(dev, dtype, x, S, noise, gout, shape[5])
    for name, s, t in zip(("out", "gx", "gS"), a, b):
        assert torch.equal(s, t), name


def test_the_noise_receives_no_gradient(dev):
    from torecsys_amd import functional as F_
    shape = (6, 12, 16, 16, 3, 2)
    x, S, noise, gout, _ = _case(shape, torch.float32)
    xd, Sd, nd = (t.to(dev).requires_grad_() for t in (x, S, noise))
    out = F_.dynamic_routing(xd, Sd, nd, shape[5])
    (out * gout.to(dev)).sum().backward()
    assert nd.grad is None and xd.grad is not None and Sd.grad is not None


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_a_sample_of_zero_rows(dev, dtype):
    """n2 == 0: zero output and a finite, zero gradient for that sample (the reference's autograd gives NaN there); the
    other samples are what the restatement gives"""
    shape = (6, 12, 16, 16, 3, 3)
    x, S, noise, gout = make_inputs(shape, dtype)
    x = x.clone()
    x[2] = 0
    out, gx, gS = _run(dev, dtype, x, S, noise, gout, 3)
    assert not bool(out[2].any()) and not bool(gx[2].any())
    assert bool(torch.isfinite(out).all() and torch.isfinite(gx).all() and torch.isfinite(gS).all())
    keep = [0, 1, 3, 4, 5]
    ref = dynamic_routing_grads(x[keep].double(), S.double(), noise[keep].double(), 3, gout[keep].double())
    errs = _errs((out[keep], gx[keep], gS), ref)
    assert max(errs) <= TOL[dtype], errs


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_default_noise_is_randn_on_the_device(dev, dtype):
    """torch.manual_seed(s); layer(x) equals functional.dynamic_routing with torch.randn drawn on the device after the same
    seed, bit for bit"""
    from torecsys_amd import functional as F_, layers as L
    B, N, E, R = 9, 50, 16, 32
    m = L.DynamicRoutingLayer(E, R, 8, 3).to(dev).to(dtype)
    x = (X_SCALE * torch.randn(B, N, E)).to(dev).to(dtype)
    torch.manual_seed(77)
    y = m(x)
    assert m.num_caps == 5 and y.names == ("B", "N", "O") and tuple(y.shape) == (B, 5, R)
    torch.manual_seed(77)
    noise = torch.randn(B, 5, N, R, dtype=dtype, device=dev)
    assert torch.equal(y.rename(None), F_.dynamic_routing(x, m.S, noise, 3))
    assert torch.equal(y.rename(None), m(x, noise).rename(None))


_CHILD = """
import sys, torch
from torecsys_amd import layers as L
assert L.DYNAMIC_ROUTING is False
calls = []
from torecsys_amd import _abi, functional as F_
orig = _abi.call
def spy(name, *a):
    calls.append(name)
    return orig(name, *a)
_abi.call = F_.call = spy
d = torch.load(sys.argv[1])
dev = torch.device("cuda:0")
m = L.DynamicRoutingLayer(d["S"].shape[0], d["S"].shape[1], d["caps"], d["iters"]).to(dev)
m.load_state_dict({"S": d["S"]})
x = d["x"].to(dev).requires_grad_()
y = m(x, d["noise"].to(dev))
assert y.names == ("B", "N", "O")
(y.rename(None) * d["gout"].to(dev)).sum().backward()
assert not any(c.startswith("trs_dynamic_routing") for c in calls), calls
torch.save({"out": y.rename(None).detach().cpu(), "gx": x.grad.cpu(), "gS": m.S.grad.cpu()}, sys.argv[2])
print("ROUTING-ATEN OK")
"""


def test_switch_selects_the_aten_composition(dev, tmp_path):
    """TRS_DYNAMIC_ROUTING=0 is read at import, so the ATen composition runs in a process of its own; in fp32 it agrees
    with the fused path within the fp32 tolerance.  (In bf16 the composition rounds the priors to bf16, which moves the
    output by about 1e-2 at 3 iterations: that comparison would not be a check of the kernels.)"""
    shape = (16, 50, 64, 64, 4, 3)
    x, S, noise, gout, _ = _case(shape, torch.float32)
    fused = _run(dev, torch.float32, x, S, noise, gout, shape[5])
    src, dst = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save({"x": x, "S": S, "noise": noise, "gout": gout, "caps": shape[4], "iters": shape[5]}, src)
    env = dict(os.environ, TRS_DYNAMIC_ROUTING="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CHILD, src, dst], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "ROUTING-ATEN OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    aten = torch.load(dst)
    errs = (rel_err_both(fused[0].cpu(), aten["out"]), rel_err_both(fused[1].cpu(), aten["gx"]),
            rel_err(fused[2].cpu(), aten["gS"]))
    print(f"routing fused against ATen fp32: out {errs[0]:.2e} gx {errs[1]:.2e} gS {errs[2]:.2e}")
    assert max(errs) <= TOL[torch.float32], errs


# ------------------------------------------------------------------------------------------------ hipGraph capture
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_routing_captures_into_a_graph(dev, dtype):
    """one forward + backward of functional.dynamic_routing with explicit noise under torch.cuda.graph (a single chain:
    one stream, no side branch), replayed with new values copied into the static tensors, equals the eager result bit
    for bit"""
    from torecsys_amd import functional as F_
    B, N, E, R, K, iters = 67, 12, 16, 16, 3, 3
    g = torch.Generator().manual_seed(5)

    def draw():
        return [(sc * torch.randn(s, generator=g)).to(dev).to(dtype)
                for sc, s in ((X_SCALE, (B, N, E)), (1.0, (E, R)), (1.0, (B, K, N, R)), (1.0, (B, K, R)))]

    def run(x, S, noise, gout):
        ins = [t.detach().requires_grad_() for t in (x, S)]
        out = F_.dynamic_routing(ins[0], ins[1], noise, iters)
        return [out.detach()] + list(torch.autograd.grad(out, ins, gout))

    sets = [draw() for _ in range(3)]
    eager = [[t.clone() for t in run(*s)] for s in sets]
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
        for name, got, w in zip(("out", "gx", "gS"), results, want):
            assert torch.equal(got, w), name


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_empty_batch(dev, dtype):
    from torecsys_amd import functional as F_, layers as L
    m = L.DynamicRoutingLayer(8, 16, 4, 3).to(dev).to(dtype)
    x = torch.zeros(0, 12, 8, device=dev, dtype=dtype, requires_grad=True)
    y = m(x)
    assert tuple(y.shape) == (0, 3, 16) and y.dtype == dtype and y.names == ("B", "N", "O")
    y.rename(None).sum().backward()
    assert tuple(x.grad.shape) == (0, 12, 8) and not bool(m.S.grad.any())
    out = F_.dynamic_routing_forward_raw(torch.zeros(0, 12, 16, device=dev), torch.zeros(0, 3, 12, 16, device=dev, dtype=dtype), 3)
    assert tuple(out.shape) == (0, 3, 16)


def test_raw_entries_refuse_strided_operands_and_uncovered_shapes(dev):
    from torecsys_amd import functional as F_
    pri, noise = torch.zeros(4, 6, 16, device=dev), torch.zeros(4, 2, 6, 16, device=dev)
    with pytest.raises(ValueError, match="priors must be contiguous"):
        F_.dynamic_routing_forward_raw(torch.zeros(4, 6, 32, device=dev)[:, :, ::2], noise, 3)
    with pytest.raises(ValueError, match="noise must be contiguous"):
        F_.dynamic_routing_forward_raw(pri, torch.zeros(4, 2, 6, 32, device=dev)[..., ::2], 3)
    with pytest.raises(NotImplementedError, match="does not cover N=129"):
        F_.dynamic_routing(torch.zeros(2, 129, 8, device=dev), torch.zeros(8, 16, device=dev),
                           torch.zeros(2, 7, 129, 16, device=dev), 3)
    # unaligned pointers of a vector-path shape take the element loads and give the same bits
    buf = torch.zeros(noise.numel() + 1, device=dev)
    g = torch.Generator().manual_seed(2)
    pri.copy_(torch.randn(pri.shape, generator=g))
    noise.copy_(torch.randn(noise.shape, generator=g))
    off = buf[1:].view(noise.shape)
    off.copy_(noise)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    assert torch.equal(F_.dynamic_routing_forward_raw(pri, off, 3), F_.dynamic_routing_forward_raw(pri, noise, 3))


def test_layer_outside_the_envelope_keeps_the_aten_composition(dev, calls):
    """N = 130 is outside the kernels' envelope: the module runs the ATen composition and still matches the restatement"""
    from torecsys_amd import layers as L
    shape = (3, 130, 8, 16, 8, 2)
    x, S, noise, gout = make_inputs(shape, torch.float32)
    m = L.DynamicRoutingLayer(8, 16, 8, 2).to(dev)
    m.load_state_dict({"S": S})
    xd = x.to(dev).requires_grad_()
    y = m(xd, noise.to(dev))
    assert m.num_caps == 7 and not calls
    (y.rename(None) * gout.to(dev)).sum().backward()
    ref = dynamic_routing_grads(x.double(), S.double(), noise.double(), 2, gout.double())
    errs = _errs((y.rename(None).detach(), xd.grad, m.S.grad), ref)
    assert max(errs) <= 1e-5, errs

"""GPU parity of the residual self-attention block (functional.self_attn_residual, csrc/self_attn.hip) through
fused.residual_self_attention, and of PersonalizedReRankingModel through the harness model: against the reference's own
float64 outputs and gradients (tests/golden/prm.npz) and, at sizes the fixture does not hold, against
nn.MultiheadAttention on the CPU (tests/prm_ref.py, pinned to the fixture by tests/test_prm_host.py).
fp32 block: 1e-5 relative.  bf16: the reference is the fp32 composition on the bf16-rounded parameters and the bound
max(1e-2, 2 x e_aten), e_aten being the error of the same call with the fused path switched off (the ATen composition in
bf16) on the same inputs, as in test_gpu_list_attn.py.  Whole model: against float64, max(1e-5, 2 x e_aten) in fp32 -- the
reference's own fp32 sits 2.3e-6 .. 7.6e-6 from float64 through the batch-norms -- and the bf16 rule in bf16.

Worst bf16 pair measured over the grid of test_block_against_torch_composition: see profiles/self_attn_kernels.md."""
import pytest
import torch

from conftest import rel_err
from prm_ref import MHA_KEYS, OUT_BIAS, OUT_WEIGHT, PRM_SHAPES, block_grads, block_mha, make_mha, model, prm_tag

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
TOLBF = 1e-2
ATTN0 = "layers.EncodingLayer.Transformer_0.MultiHeadAttention."


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


class _Spy:
    """counts the calls of functional.self_attn_residual (there is no CPU fallback to hide behind)"""

    def __init__(self, monkeypatch):
        from torecsys_amd import functional as F_
        self.calls, real = 0, F_.self_attn_residual

        def spy(*a, **k):
            self.calls += 1
            return real(*a, **k)

        monkeypatch.setattr(F_, "self_attn_residual", spy)


def _want_path(E, H, dtype):
    return 2 if dtype == torch.bfloat16 and E % 16 == 0 and (E // H) % 16 == 0 else 1


def _on_device(mha, dev, dtype):
    """a copy of the CPU attention on the device in ``dtype``"""
    m = torch.nn.MultiheadAttention(mha.embed_dim, mha.num_heads, dropout=mha.dropout, bias=mha.in_proj_bias is not None)
    m.load_state_dict(mha.state_dict())
    return m.to(dev).to(dtype)


def _reference(mha, x, gout):
    """the fp32 CPU composition: output, dx and {key: gradient}"""
    for p in mha.parameters():
        p.grad = None
    xr = x.detach().clone().requires_grad_()
    y = block_mha(xr, mha)
    (y * gout).sum().backward()
    want = {"out": y.detach(), "dx": xr.grad}
    want.update({k: p.grad.clone() for k, p in mha.named_parameters()})
    return want


def _run_block(dev, monkeypatch, mha, x, gout, dtype, want, fused, calls=1):
    from torecsys_amd import fused as FU
    monkeypatch.setattr(FU, "SELF_ATTN", fused)
    spy = _Spy(monkeypatch)
    m = _on_device(mha, dev, dtype)
    xd = x.to(dev).to(dtype).requires_grad_()
    y = FU.residual_self_attention(m, xd)
    assert spy.calls == (calls if fused else 0)
    assert tuple(y.shape) == tuple(x.shape) and y.dtype == dtype
    (y * gout.to(dev).to(dtype)).sum().backward()
    errs = {"out": rel_err(y.float().cpu(), want["out"]), "dx": rel_err(xd.grad.float().cpu(), want["dx"])}
    for k, p in m.named_parameters():
        errs[k] = rel_err(p.grad.float().cpu(), want[k])
    return errs


def _check(got, aten, dtype, what):
    if dtype == torch.float32:
        for k, e in got.items():
            assert e <= TOL32, (what, k, e)
        return
    for k in got:
        print(f"bf16 {what} {k}: fused {got[k]:.3e} aten {aten[k]:.3e}")
    for k in got:
        assert got[k] <= max(TOLBF, 2 * aten[k]), (what, k, got[k], aten[k])


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("shape", PRM_SHAPES, ids=prm_tag)
def test_block_against_the_fixture(golden, dev, monkeypatch, shape):
    from torecsys_amd import fused as FU
    G = golden("prm")
    B, L, emb, E, H, layers = shape
    tag = prm_tag(shape)
    monkeypatch.setattr(FU, "SELF_ATTN", True)          # fp32 is off by default
    spy = _Spy(monkeypatch)
    m = torch.nn.MultiheadAttention(E, H)
    m.load_state_dict({k: G(f"model/{tag}/param/{ATTN0}{k}").float() for k in MHA_KEYS})
    m = m.to(dev)
    x = G(f"block/{tag}/x").float().to(dev).requires_grad_()
    y = FU.residual_self_attention(m, x)
    assert spy.calls == 1
    assert rel_err(y.cpu(), G(f"block/{tag}/y")) <= TOL32
    (y * G(f"block/{tag}/gout").float().to(dev)).sum().backward()
    assert rel_err(x.grad.cpu(), G(f"block/{tag}/dx")) <= TOL32
    for k, p in m.named_parameters():
        assert rel_err(p.grad.cpu(), G(f"block/{tag}/grad/{k}")) <= TOL32, k


# ------------------------------------------------------------------------------------------------ the torch composition
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 31, 32, 33, 64])
@pytest.mark.parametrize("E,H", [(64, 4), (64, 1), (32, 2), (16, 1), (10, 5)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_block_against_torch_composition(dev, monkeypatch, dtype, E, H, L, bias):
    """B = 97 (several workgroups, an odd count); L at the 16-row tile edges and the 32-wide k-step of the MFMA products:
    the output, dx and the gradients of all attention parameters"""
    from torecsys_amd import functional as F_
    B = 97
    g = torch.Generator().manual_seed(977 + L * 7 + E + H)
    mha = make_mha(E, H, bias, generator=g)
    with torch.no_grad():
        for p in mha.parameters():
            p.copy_(p.to(dtype).float())                                  # the rounded parameters are THE parameters
    x = torch.randn(B, L, E, generator=g).to(dtype).float()
    gout = torch.randn(B, L, E, generator=g).to(dtype).float()
    want = _reference(mha, x, gout)
    assert F_.self_attn_path(L, E, H, dtype) == _want_path(E, H, dtype)
    got = _run_block(dev, monkeypatch, mha, x, gout, dtype, want, True)
    assert sorted(got) == sorted(["out", "dx"] + (MHA_KEYS if bias else [MHA_KEYS[0], MHA_KEYS[2]]))
    aten = _run_block(dev, monkeypatch, mha, x, gout, dtype, want, False) if dtype == torch.bfloat16 else None
    _check(got, aten, dtype, f"L={L} E={E} H={H} b{int(bias)}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_persistent_loop_and_slab_reduction(dev, monkeypatch, dtype):
    """B = 2 x grid + 1: every workgroup walks two samples and one walks three; the slabs of all of them are reduced"""
    from torecsys_amd import _abi
    L, E, H = 5, 16, 2
    code = _abi.TRS_F32 if dtype == torch.float32 else _abi.TRS_BF16
    blocks = _abi.size_query("trs_self_attn_blocks", 1 << 30, L, E, H, code, 1)
    assert blocks >= 1
    B = 2 * blocks + 1
    g = torch.Generator().manual_seed(19)
    mha = make_mha(E, H, True, generator=g)
    with torch.no_grad():
        for p in mha.parameters():
            p.copy_(p.to(dtype).float())
    x = torch.randn(B, L, E, generator=g).to(dtype).float()
    gout = torch.randn(B, L, E, generator=g).to(dtype).float()
    want = _reference(mha, x, gout)
    got = _run_block(dev, monkeypatch, mha, x, gout, dtype, want, True)
    aten = _run_block(dev, monkeypatch, mha, x, gout, dtype, want, False) if dtype == torch.bfloat16 else None
    _check(got, aten, dtype, f"B={B}")


@pytest.mark.parametrize("dtype,E,H", [(torch.float32, 16, 2), (torch.bfloat16, 16, 1)], ids=["vector", "mfma"])
def test_two_backward_calls_give_the_same_bits(dev, dtype, E, H):
    from torecsys_amd import _abi
    from torecsys_amd import functional as F_
    L = 5
    code = _abi.TRS_F32 if dtype == torch.float32 else _abi.TRS_BF16
    assert F_.self_attn_path(L, E, H, dtype) == _want_path(E, H, dtype)
    B = _abi.size_query("trs_self_attn_blocks", 1 << 30, L, E, H, code, 1) + 13          # above the grid size
    g = torch.Generator().manual_seed(23)
    mha = make_mha(E, H, True, generator=g).to(dev).to(dtype)
    x = torch.randn(B, L, E, generator=g).to(dev).to(dtype)
    gout = torch.randn(B, L, E, generator=g).to(dev).to(dtype)
    res = []
    for _ in range(2):
        ps = [p.detach().clone().requires_grad_() for p in (mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight,
                                                            mha.out_proj.bias)]
        xd = x.clone().requires_grad_()
        y = F_.self_attn_residual(xd, *ps, H)
        y.backward(gout)
        res.append([y.detach(), xd.grad] + [p.grad for p in ps])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert float(res[0][2].abs().max()) > 0 and float(res[0][4].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ operand placement
def test_operand_placement(dev):
    """x as a strided slice of a larger tensor; a frozen in_proj_weight (gradient None, the others unchanged); x without
    requires_grad (no dx is formed, the parameter gradients are unchanged)"""
    from torecsys_amd import functional as F_
    B, L, E, H = 37, 7, 16, 2
    g = torch.Generator().manual_seed(29)
    mha = make_mha(E, H, True, generator=g)
    big = torch.randn(B, L, 2 * E + 3, generator=g)
    x = big[:, :, 3:3 + E]
    gout = torch.randn(B, L, E, generator=g)
    want = _reference(mha, x, gout)
    names = ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]

    def run(x_grad=True, frozen=()):
        bigd = big.to(dev).requires_grad_(x_grad)
        xd = bigd[:, :, 3:3 + E]
        assert not xd.is_contiguous()
        ps = {k: p.detach().to(dev).requires_grad_(k not in frozen) for k, p in mha.named_parameters()}
        y = F_.self_attn_residual(xd, *(ps[k] for k in names), H)
        (y * gout.to(dev)).sum().backward()
        return y.detach(), bigd.grad, {k: p.grad for k, p in ps.items()}

    y, gbig, gp = run()
    assert rel_err(y.cpu(), want["out"]) <= TOL32
    assert rel_err(gbig[:, :, 3:3 + E].cpu(), want["dx"]) <= TOL32
    assert float(gbig[:, :, :3].abs().max()) == 0.0 and float(gbig[:, :, 3 + E:].abs().max()) == 0.0
    for k in names:
        assert rel_err(gp[k].cpu(), want[k]) <= TOL32, k
    y2, gbig2, gp2 = run(frozen=("in_proj_weight",))
    assert gp2["in_proj_weight"] is None and torch.equal(y2, y) and torch.equal(gbig2, gbig)
    for k in names[1:]:
        assert torch.equal(gp2[k], gp[k]), k
    y3, gbig3, gp3 = run(x_grad=False)
    assert gbig3 is None and torch.equal(y3, y)
    for k in names:
        assert torch.equal(gp3[k], gp[k]), k


# ------------------------------------------------------------------------------------------------ the whole model
def _model_errs(m, out, x, want_out, want_grads, want_after):
    errs = {"out": rel_err(out.float().cpu(), want_out), "input": rel_err(x.grad.float().cpu(), want_grads["input"])}
    grads = {k: p.grad.float().cpu() for k, p in m.named_parameters()}
    for k, g in grads.items():
        if k == OUT_BIAS:          # zero in exact arithmetic: measured against the weight's gradient, never its own
            errs[k] = float(g.abs().max()) / float(want_grads[OUT_WEIGHT].abs().max())
        else:
            errs[k] = rel_err(g, want_grads[k])
    for k, v in m.state_dict().items():
        if "running_" in k:
            errs["after/" + k] = rel_err(v.float().cpu(), want_after[k])
        elif "num_batches_tracked" in k:
            assert int(v) == int(want_after[k])
    return errs


def _run_model(dev, monkeypatch, shape, sd, x, gout, dtype, fused, want):
    from harness.ltr_models import PersonalizedReRankingModel
    from torecsys_amd import fused as FU
    B, L, emb, E, H, layers = shape
    monkeypatch.setattr(FU, "SELF_ATTN", fused)
    spy = _Spy(monkeypatch)
    m = PersonalizedReRankingModel(embed_size=emb, max_num_position=L, encoding_size=E, num_heads=H, num_layers=layers)
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()})
    m = m.to(dev).to(dtype).train()
    xd = x.to(dev).to(dtype).requires_grad_()
    out = m(xd)
    assert spy.calls == (layers if fused else 0)
    assert out.names == ("B", "O") and tuple(out.shape) == (B, L) and out.dtype == dtype
    (out.rename(None) * gout.to(dev).to(dtype)).sum().backward()
    errs = _model_errs(m, out.rename(None), xd, *want)
    assert sorted(k for k in errs if not k.startswith("after/") and k not in ("out", "input")) == \
        sorted(k for k, _ in m.named_parameters())          # no key is left out
    return errs


@pytest.mark.parametrize("shape", PRM_SHAPES, ids=prm_tag)
def test_model_against_the_float64_fixture(golden, dev, monkeypatch, shape):
    G = golden("prm")
    pre = "model/" + prm_tag(shape)
    keys = G(pre + "/keys")
    sd = {k: G(f"{pre}/param/{k}") for k in keys}
    want_grads = {k[len(pre) + 6:]: G(k) for k in G.keys() if k.startswith(pre + "/grad/")}
    want_after = {k: G(f"{pre}/after/{k}") for k in keys if G.has(f"{pre}/after/{k}")}
    want = (G(pre + "/out"), want_grads, want_after)
    args = (dev, monkeypatch, shape, sd, G(pre + "/input"), G(pre + "/gout"), torch.float32)
    got = _run_model(*args, True, want)
    aten = _run_model(*args, False, want)
    for k in got:
        print(f"fp32 model {prm_tag(shape)} {k}: fused {got[k]:.3e} aten {aten[k]:.3e}")
    for k in got:
        assert got[k] <= max(TOL32, 2 * aten[k]), (k, got[k], aten[k])


def test_model_bf16_against_the_float64_restatement(dev, monkeypatch):
    from harness.ltr_models import PersonalizedReRankingModel
    shape = (97, 30, 24, 64, 4, 2)
    B, L, emb, E, H, layers = shape
    torch.manual_seed(31)
    g = torch.Generator().manual_seed(37)
    ref = PersonalizedReRankingModel(embed_size=emb, max_num_position=L, encoding_size=E, num_heads=H, num_layers=layers)
    with torch.no_grad():
        for k, p in ref.named_parameters():
            if k.endswith("bias") and "BatchNorm" not in k and "PositionEmbedding" not in k:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            p.copy_(p.bfloat16().float())                                 # the rounded parameters are THE parameters
    sd = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    x = torch.randn(B, L, emb, generator=g).bfloat16().float()
    gout = torch.randn(B, L, generator=g).bfloat16().float()
    sd64 = {k: (v.double().requires_grad_("running_" not in k) if v.is_floating_point() else v) for k, v in sd.items()}
    x64 = x.double().requires_grad_()
    out64, after64 = model(sd64, x64, H)
    (out64 * gout.double()).sum().backward()
    want_grads = {k: v.grad for k, v in sd64.items() if v.is_floating_point() and v.requires_grad}
    want_grads["input"] = x64.grad
    want = (out64.detach(), want_grads, after64)
    args = (dev, monkeypatch, shape, sd, x, gout, torch.bfloat16)
    got = _run_model(*args, True, want)
    aten = _run_model(*args, False, want)
    for k in got:
        print(f"bf16 model {k}: fused {got[k]:.3e} aten {aten[k]:.3e}")
    for k in got:
        assert got[k] <= max(TOLBF, 2 * aten[k]), (k, got[k], aten[k])


def test_default_switch_is_per_dtype(dev, monkeypatch):
    """without TRS_SELF_ATTN: bf16 runs the kernel, fp32 keeps the composition (measured slower there)"""
    from torecsys_amd import fused as FU
    assert FU.SELF_ATTN is None
    g = torch.Generator().manual_seed(43)
    cpu = make_mha(16, 1, True, generator=g)
    x = torch.randn(5, 6, 16, generator=g)
    spy = _Spy(monkeypatch)
    FU.residual_self_attention(_on_device(cpu, dev, torch.float32), x.to(dev))
    assert spy.calls == 0
    FU.residual_self_attention(_on_device(cpu, dev, torch.bfloat16), x.to(dev).bfloat16())
    assert spy.calls == 1


# ------------------------------------------------------------------------------------------------ eval mode and dropout
def test_dropout_keeps_the_composition_in_training_and_the_kernel_in_eval(dev, monkeypatch):
    from torecsys_amd import fused as FU
    g = torch.Generator().manual_seed(41)
    E, H = 16, 2
    cpu = make_mha(E, H, True, generator=g)
    m = torch.nn.MultiheadAttention(E, H, dropout=0.1)
    m.load_state_dict(cpu.state_dict())
    m = m.to(dev)
    x = torch.randn(9, 6, E, generator=g)
    monkeypatch.setattr(FU, "SELF_ATTN", True)          # fp32 is off by default
    spy = _Spy(monkeypatch)
    m.train()
    y = FU.residual_self_attention(m, x.to(dev))
    assert spy.calls == 0 and tuple(y.shape) == (9, 6, E)
    m.eval()
    y = FU.residual_self_attention(m, x.to(dev))
    assert spy.calls == 1
    assert rel_err(y.cpu(), block_mha(x, cpu.eval())) <= TOL32




# ------------------------------------------------------------------------------------------------ hipGraph capture
def test_graphed_forward_backward_matches_eager(dev, monkeypatch):
    """one forward + backward of the block captured by GraphedStep and replayed on three batches (two of them new input
    values): loss, dx and the four parameter gradients equal the eager step's bit for bit -- the kernels are the same and
    the slab reduction has a fixed order"""
    from torecsys_amd import fused as FU
    from torecsys_amd.graph import GraphedStep
    B, L, E, H = 300, 20, 32, 2
    g = torch.Generator().manual_seed(3)
    m = make_mha(E, H, True, generator=g).to(dev)
    params = list(m.parameters())
    batches = [(torch.randn(B, L, E, generator=g).to(dev), torch.randn(B, L, E, generator=g).to(dev)) for _ in range(3)]
    monkeypatch.setattr(FU, "SELF_ATTN", True)          # fp32 is off by default
    spy = _Spy(monkeypatch)

    def fn(x, gy):
        xl = x.detach().requires_grad_()
        loss = (FU.residual_self_attention(m, xl) * gy).sum()
        loss.backward()
        return loss.detach(), xl.grad

    eager = []
    for x, gy in batches:
        for p in params:
            p.grad = None
        loss, dx = fn(x, gy)
        eager.append((loss.clone(), dx.clone(), [p.grad.clone() for p in params]))
    del loss, dx
    assert spy.calls == 3
    step = GraphedStep(fn, batches[0], params=params, warmup=2)
    for (x, gy), (l0, dx0, g0) in zip(batches, eager):
        loss, dx = step(x, gy)
        torch.cuda.synchronize()
        print(f"replayed loss {float(loss)!r} eager {float(l0)!r}")
        assert torch.equal(loss, l0)
        assert torch.equal(dx, dx0)
        for p, gp in zip(params, g0):
            assert torch.equal(p.grad, gp)


# ------------------------------------------------------------------------------------------------ patch()
def test_patched_model_runs_the_kernel_on_the_device(dev, monkeypatch):
    """patch() on a stand-in package whose PersonalizedReRankingModel.forward is the composition: on HIP tensors the wrapped
    forward runs one fused call per encoder layer and returns the ('B', 'O')-named softmax of the original forward; a
    named input and a list of one item go to the original forward"""
    import sys
    import types
    import torecsys_amd
    from harness import ltr_models
    from torecsys_amd import fused as FU

    class Standin(ltr_models.PersonalizedReRankingModel):
        def forward(self, feat_inputs):
            if feat_inputs.has_names():
                raise RuntimeError("named input")
            was, FU.SELF_ATTN = FU.SELF_ATTN, False
            try:
                return ltr_models.PersonalizedReRankingModel.forward(self, feat_inputs)
            finally:
                FU.SELF_ATTN = was

    pkg, mdl = types.ModuleType("fake_prm_gpu"), types.ModuleType("fake_prm_gpu.models")
    Standin.__name__ = "PersonalizedReRankingModel"
    mdl.PersonalizedReRankingModel = Standin
    pkg.models = mdl
    for m in (pkg, mdl):
        sys.modules[m.__name__] = m
    monkeypatch.setattr(FU, "SELF_ATTN", True)
    spy = _Spy(monkeypatch)
    try:
        torch.manual_seed(47)
        model = Standin(12, 6, 16, 2, 2, dropout=0.0).to(dev)
        x = torch.randn(9, 6, 12, device=dev)
        want = model(x)
        assert spy.calls == 0
        torecsys_amd.patch(pkg)
        got = model(x)
        assert spy.calls == 2 and got.names == want.names == ("B", "O")
        assert rel_err(got.rename(None).cpu(), want.rename(None).cpu()) <= TOL32
        with pytest.raises(RuntimeError, match="named input"):
            model(x.refine_names("B", "L", "E"))
        one = Standin(12, 1, 16, 2, 1, dropout=0.0).to(dev).eval()
        one(torch.randn(4, 1, 12, device=dev))
        assert spy.calls == 2
    finally:
        torecsys_amd.unpatch()
        for m in (pkg, mdl):
            sys.modules.pop(m.__name__, None)

"""PersonalizedReRankingModel, host side (no GPU): the torch restatements of tests/prm_ref.py and the harness model on its
composition path against the reference's own float64 outputs, gradients and running statistics (tests/golden/prm.npz) at
1e-10; the path rule and the argument validation of the C-ABI entries of csrc/self_attn.hip; patch() / unpatch()."""
import ctypes
import os
import sys
import types

import pytest
import torch

from conftest import rel_err
from prm_ref import MHA_KEYS, OUT_BIAS, PRM_SHAPES, block, block_grads, block_mha, make_mha, model, prm_tag

TOL64 = 1e-10
ATTN0 = "layers.EncodingLayer.Transformer_0.MultiHeadAttention."


def _expected_keys(layers):
    keys = ["layers.InputLayer.PositionEmbedding.bias", "layers.InputLayer.FeedForward.weight",
            "layers.InputLayer.FeedForward.bias"]
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    for i in range(layers):
        t = f"layers.EncodingLayer.Transformer_{i}."
        keys += [t + "MultiHeadAttention." + k for k in MHA_KEYS]
        keys += [t + "AttentionBatchNorm." + k for k in bn]
        keys += [t + "FeedForward.FeedForward.weight", t + "FeedForward.FeedForward.bias"]
        keys += [t + "FNNBatchNorm." + k for k in bn]
    return keys + ["layers.OutputLayer.FeedForward.weight", "layers.OutputLayer.FeedForward.bias"]


@pytest.mark.parametrize("shape", PRM_SHAPES, ids=prm_tag)
def test_fixture_layout(golden, shape):
    G = golden("prm")
    B, L, emb, E, H, layers = shape
    pre = "model/" + prm_tag(shape)
    keys = G(pre + "/keys")
    assert keys == _expected_keys(layers)
    assert G(pre + "/names") == ["B", "O"] and tuple(G(pre + "/out").shape) == (B, L)
    assert G(pre + "/out").dtype == torch.float64
    assert float((G(pre + "/out").sum(1) - 1).abs().max()) <= 1e-12
    changed = [k for k in keys if k not in G(pre + "/unchanged")]
    assert changed == [k for k in keys if "running_" in k or "num_batches_tracked" in k]
    for k in keys:          # non-zero biases everywhere; bf16-representable parameters and inputs
        p = G(f"{pre}/param/{k}")
        if k.endswith("bias"):
            assert float(p.abs().min()) > 0, k
        if p.dtype == torch.float64 and "running_" not in k:
            assert torch.equal(p.to(torch.bfloat16).double(), p), k
    assert torch.equal(G(pre + "/input").to(torch.bfloat16).double(), G(pre + "/input"))


@pytest.mark.parametrize("shape", PRM_SHAPES, ids=prm_tag)
def test_block_restatements_equal_the_fixture(golden, shape):
    """the per-sample formula AND nn.MultiheadAttention on the transposed block reproduce the reference's x + MHA(x) and
    all five gradients in float64"""
    G = golden("prm")
    B, L, emb, E, H, layers = shape
    tag = prm_tag(shape)
    params = [G(f"model/{tag}/param/{ATTN0}{k}") for k in MHA_KEYS]
    x, gout = G(f"block/{tag}/x"), G(f"block/{tag}/gout")
    y, dx, gp = block_grads(lambda x_, *p: block(x_, *p, H), x, params, gout)
    mha = make_mha(E, H, True, dict(zip(MHA_KEYS, params)), dtype=torch.float64)
    y2 = block_mha(x, mha)
    assert rel_err(y2, G(f"block/{tag}/y")) <= TOL64
    assert rel_err(y, G(f"block/{tag}/y")) <= TOL64
    assert rel_err(dx, G(f"block/{tag}/dx")) <= TOL64
    for k, g in zip(MHA_KEYS, gp):
        assert rel_err(g, G(f"block/{tag}/grad/{k}")) <= TOL64, k


def _check_model(G, pre, keys, out, grads, after):
    assert rel_err(out, G(pre + "/out")) <= TOL64
    wmax = float(G(f"{pre}/grad/layers.OutputLayer.FeedForward.weight").abs().max())
    for k, g in grads.items():
        want = G(f"{pre}/grad/{k}")
        if k == OUT_BIAS:          # zero in exact arithmetic: never compared relatively
            assert float(g.abs().max()) <= TOL64 * wmax and float(want.abs().max()) <= TOL64 * wmax
        else:
            assert rel_err(g, want) <= TOL64, k
    for k in keys:
        if "running_" in k:
            assert rel_err(after[k], G(f"{pre}/after/{k}")) <= TOL64, k
        elif "num_batches_tracked" in k:
            assert int(after[k]) == int(G(f"{pre}/after/{k}")) == 1, k


@pytest.mark.parametrize("shape", PRM_SHAPES, ids=prm_tag)
def test_model_restatement_equals_the_fixture(golden, shape):
    G = golden("prm")
    B, L, emb, E, H, layers = shape
    pre = "model/" + prm_tag(shape)
    keys = G(pre + "/keys")
    sd = {k: G(f"{pre}/param/{k}") for k in keys}
    for k, v in sd.items():
        if "running_" not in k and "num_batches" not in k:
            v.requires_grad_()
    x = G(pre + "/input").requires_grad_()
    out, after = model(sd, x, H)
    (out * G(pre + "/gout")).sum().backward()
    grads = {k: v.grad for k, v in sd.items() if v.requires_grad}
    grads["input"] = x.grad
    assert sorted(grads) == sorted(k[len(pre) + 6:] for k in G.keys() if k.startswith(pre + "/grad/"))
    _check_model(G, pre, keys, out, grads, after)


@pytest.mark.parametrize("shape", PRM_SHAPES, ids=prm_tag)
def test_harness_model_on_cpu_equals_the_fixture(golden, shape):
    """the composition path of fused.residual_self_attention: keys, names, outputs, every gradient and the running
    statistics after one training-mode step"""
    from harness.ltr_models import PersonalizedReRankingModel
    G = golden("prm")
    B, L, emb, E, H, layers = shape
    pre = "model/" + prm_tag(shape)
    keys = G(pre + "/keys")
    m = PersonalizedReRankingModel(embed_size=emb, max_num_position=L, encoding_size=E, num_heads=H, num_layers=layers)
    assert m.layers["EncodingLayer"]["Transformer_0"]["MultiHeadAttention"].dropout == 0.0      # dropout=None is 0.0
    m = m.double().train()
    assert list(m.state_dict().keys()) == keys
    m.load_state_dict({k: G(f"{pre}/param/{k}") for k in keys})
    x = G(pre + "/input").requires_grad_()
    out = m(x)
    assert out.names == ("B", "O") and tuple(out.shape) == (B, L)
    (out.rename(None) * G(pre + "/gout")).sum().backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["input"] = x.grad
    _check_model(G, pre, keys, out.rename(None), grads, m.state_dict())
    for k in G(pre + "/unchanged"):
        assert torch.equal(m.state_dict()[k], G(f"{pre}/param/{k}")), k


def test_harness_model_refuses_use_bias_false():
    from harness.ltr_models import PersonalizedReRankingModel
    with pytest.raises(ValueError, match="use_bias=False"):
        PersonalizedReRankingModel(8, 4, 8, 2, 1, use_bias=False)


def test_position_embedding_layer():
    from torecsys_amd.layers import PositionEmbeddingLayer
    torch.manual_seed(0)
    m = PositionEmbeddingLayer(max_num_position=5)
    assert list(m.state_dict().keys()) == ["bias"] and tuple(m.bias.shape) == (1, 5, 1)
    assert m.inputs_size == {"inputs": ("B", "L", "E")} and m.outputs_size == {"outputs": ("B", "L", "E")}
    assert float(m.bias.detach().std()) > 0.1          # N(0, 1) init
    x = torch.randn(3, 5, 4)
    assert torch.equal(m(x), x + m.bias)


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def _bwd_floats(L, E):
    return 6 * L * E + 2 * L * L + 6 * L


def test_self_attn_path_rule(lib):
    from torecsys_amd import functional as F_
    for dtype, code in ((torch.float32, 0), (torch.bfloat16, 1)):
        for E, H in [(64, 1), (64, 4), (64, 2), (32, 2), (32, 1), (16, 1), (16, 2), (10, 5), (8, 1), (48, 3), (128, 8),
                     (128, 2), (96, 2)]:
            for L in range(1, 65):
                p = lib.trs_self_attn_path(L, E, H, code)
                assert F_.self_attn_path(L, E, H, dtype) == p
                if 4 * _bwd_floats(L, E) > 160 * 1024:          # the backward's working set does not fit the LDS
                    assert p == 0 and E > 64, (L, E, H)
                elif dtype == torch.bfloat16 and E % 16 == 0 and (E // H) % 16 == 0:
                    assert p == 2, (L, E, H)
                else:
                    assert p == 1, (L, E, H)
    assert lib.trs_self_attn_path(47, 128, 8, 1) == 2 and lib.trs_self_attn_path(48, 128, 8, 1) == 0
    for code in (0, 1):
        assert lib.trs_self_attn_path(65, 64, 4, code) == 0
        assert lib.trs_self_attn_path(0, 64, 4, code) == 0
        assert lib.trs_self_attn_path(30, 256, 4, code) == 0
        assert lib.trs_self_attn_path(30, 64, 3, code) == 0
        assert lib.trs_self_attn_path(30, 10, 4, code) == 0
        assert lib.trs_self_attn_path(30, 64, 0, code) == 0
    for code in (2, 3, 4, 7):          # no value dtype has these codes
        assert lib.trs_self_attn_path(30, 64, 4, code) == 0
    for dt in (torch.float16, torch.float64, torch.int32, torch.int64):
        assert F_.self_attn_path(30, 64, 4, dt) == 0


def test_self_attn_entries_validate_arguments_without_gpu(lib):
    from torecsys_amd import _abi
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    fwd, bwd = lib.trs_self_attn_fwd, lib.trs_self_attn_bwd
    # (x, B, L, E, H, dtype, w_in, b_in, w_out, b_out, y, stream)
    assert fwd(null, 2, 5, 16, 2, 0, one, null, one, null, one, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, 2, 5, 16, 2, 0, null, null, one, null, one, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, 2, 5, 16, 2, 0, one, null, null, null, one, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, 2, 5, 16, 2, 0, one, null, one, null, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, 2, 5, 16, 2, 0, one, one, one, null, one, null) == -1 and "b_in and b_out" in _abi.last_error()
    assert fwd(one, 2, 5, 16, 2, 0, one, null, one, one, one, null) == -1 and "b_in and b_out" in _abi.last_error()
    assert fwd(one, 2, 5, 16, 2, 7, one, null, one, null, one, null) == -2 and "dtype" in _abi.last_error()
    assert fwd(one, 2, 65, 16, 2, 0, one, null, one, null, one, null) == -2 and "L=65" in _abi.last_error()
    assert fwd(one, 2, 5, 256, 2, 0, one, null, one, null, one, null) == -2 and "E=256" in _abi.last_error()
    assert fwd(one, 2, 5, 16, 3, 0, one, null, one, null, one, null) == -2 and "H=3" in _abi.last_error()
    assert fwd(one, 2, 64, 128, 8, 1, one, null, one, null, one, null) == -2 and "LDS" in _abi.last_error()
    assert fwd(one, -1, 5, 16, 2, 0, one, null, one, null, one, null) == -1 and "B=-1" in _abi.last_error()
    assert fwd(null, 0, 5, 16, 2, 0, null, null, null, null, null, null) == 0          # an empty batch is a no-op
    # (x, B, L, E, H, dtype, w_in, b_in, w_out, b_out, gout, dx, workspace, ws_bytes, blocks, stream)
    big = 1 << 30
    assert bwd(one, 2, 5, 16, 2, 0, one, null, one, null, null, one, one, big, 2, null) == -1
    assert "NULL" in _abi.last_error()
    assert bwd(one, 2, 5, 16, 2, 0, one, null, one, null, one, one, null, big, 2, null) == -1
    assert "NULL" in _abi.last_error()
    assert bwd(one, 2, 5, 16, 2, 0, one, one, one, null, one, one, one, big, 2, null) == -1
    assert bwd(one, 2, 5, 16, 2, 9, one, null, one, null, one, one, one, big, 2, null) == -2
    assert "dtype" in _abi.last_error()
    assert bwd(one, 2, 70, 16, 2, 0, one, null, one, null, one, one, one, big, 2, null) == -2
    assert bwd(one, 2, 5, 16, 2, 0, one, null, one, null, one, one, one, big, 3, null) == -1
    assert "blocks" in _abi.last_error()
    assert bwd(one, 2, 5, 16, 2, 0, one, null, one, null, one, one, one, big, 0, null) == -1
    need = lib.trs_self_attn_bwd_workspace_bytes(2, 16)
    assert need == 2 * (4 * 16 * 16 + 4 * 16) * 4
    assert bwd(one, 2, 5, 16, 2, 0, one, null, one, null, one, null, one, need - 1, 2, null) == -6
    assert "workspace" in _abi.last_error()
    assert bwd(null, 0, 5, 16, 2, 0, null, null, null, null, null, null, null, 0, 0, null) == 0
    assert lib.trs_self_attn_bwd_workspace_bytes(0, 16) == 0
    assert lib.trs_self_attn_blocks(0, 5, 16, 2, 0, 1) == 0 and lib.trs_self_attn_blocks(8, 65, 16, 2, 0, 1) == 0
    with pytest.raises(RuntimeError, match="trs_self_attn_fwd failed"):
        _abi.call("trs_self_attn_fwd", null, 2, 5, 16, 2, 0, null, null, null, null, null, null)


def test_functional_argument_errors():
    from torecsys_amd import functional as F_
    x = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="x must be"):
        F_.self_attn_residual(torch.zeros(3, 8), torch.zeros(24, 8), None, torch.zeros(8, 8), None, 2)
    with pytest.raises(ValueError, match="in_proj_weight must be"):
        F_.self_attn_residual(x, torch.zeros(16, 8), None, torch.zeros(8, 8), None, 2)
    with pytest.raises(ValueError, match="both given or both None"):
        F_.self_attn_residual(x, torch.zeros(24, 8), torch.zeros(24), torch.zeros(8, 8), None, 2)
    with pytest.raises(TypeError, match="x's dtype"):
        F_.self_attn_residual(x, torch.zeros(24, 8, dtype=torch.bfloat16), None, torch.zeros(8, 8), None, 2)
    with pytest.raises(NotImplementedError, match="does not cover"):
        F_.self_attn_residual(x, torch.zeros(24, 8), None, torch.zeros(8, 8), None, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.self_attn_residual(x, torch.zeros(24, 8), None, torch.zeros(8, 8), None, 2)


def test_residual_self_attention_keeps_the_composition_off_the_device(monkeypatch):
    from torecsys_amd import functional as F_
    from torecsys_amd import fused

    def boom(*a, **k):
        raise AssertionError("the fused function must not run on CPU tensors")

    monkeypatch.setattr(F_, "self_attn_residual", boom)
    assert fused.SELF_ATTN is None          # no TRS_SELF_ATTN: on for bf16, off for fp32 (profiles/self_attn_kernels.md)
    assert fused.self_attn_enabled(torch.bfloat16) and not fused.self_attn_enabled(torch.float32)
    monkeypatch.setattr(fused, "SELF_ATTN", True)
    g = torch.Generator().manual_seed(5)
    mha = make_mha(8, 2, True, generator=g)
    x = torch.randn(3, 4, 8, generator=g)
    xt = x.transpose(0, 1)
    assert torch.equal(fused.residual_self_attention(mha, x), x + mha(xt, xt, xt)[0].transpose(0, 1))


# ------------------------------------------------------------------------------------------------ patch() / unpatch()
def _wrapped_forward_equals_original_on_cpu(pkg, cls, make):
    import torecsys_amd
    orig = cls.forward
    torch.manual_seed(3)
    m = make()
    x = torch.randn(4, 5, 6)
    want = m(x)
    try:
        torecsys_amd.patch(pkg)
        assert cls.forward is not orig and getattr(cls.forward, "_trs_head", False)
        got = m(x)
        assert got.names == want.names == ("B", "O")
        assert torch.equal(got.rename(None), want.rename(None))          # CPU tensors: the original forward, bit for bit
        torecsys_amd.patch(pkg)                                          # a second patch() wraps nothing twice
        torecsys_amd.unpatch()
        assert cls.forward is orig
    finally:
        torecsys_amd.unpatch()


def test_patch_wraps_and_restores_the_model_of_a_standin_package():
    from harness import ltr_models
    pkg = types.ModuleType("fake_prm_trs")
    mdl = types.ModuleType("fake_prm_trs.models")
    standin = type("PersonalizedReRankingModel", (ltr_models.PersonalizedReRankingModel,), {"__module__": mdl.__name__})
    mdl.PersonalizedReRankingModel = standin
    pkg.models = mdl
    for m in (pkg, mdl):
        sys.modules[m.__name__] = m
    try:
        _wrapped_forward_equals_original_on_cpu(pkg, standin, lambda: standin(6, 5, 8, 2, 2, dropout=0.0))
    finally:
        for m in (pkg, mdl):
            sys.modules.pop(m.__name__, None)


def test_patch_wraps_and_restores_the_reference_model():
    """runs where the reference checkout is present (the build container), as tests/golden/make_golden*.py do"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    try:
        import make_golden
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(make_golden.REF, "torecsys")):
        pytest.skip("no reference checkout on this machine")
    before = set(sys.modules)
    try:
        make_golden.import_reference()
        pkg = sys.modules["torecsys"]
        from torecsys.models.ltr.personalized_reranking import PersonalizedReRankingModel as Ref
        _wrapped_forward_equals_original_on_cpu(pkg, Ref, lambda: Ref(6, 5, 8, 2, 2, dropout=0.0))
    finally:
        for n in set(sys.modules) - before:
            if n.split(".")[0] in ("torecsys", "torchvision"):
                sys.modules.pop(n, None)

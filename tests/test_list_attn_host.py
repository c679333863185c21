"""Attention pooling of ListIndicesEmbedding, host side (no GPU): the two torch restatements of tests/list_attn_ref.py
against the reference's own outputs and gradients (tests/golden/list_attn.npz) and against each other at sizes the fixture
does not hold; the path rule and the argument validation of the C-ABI entries of csrc/attn_pool.hip."""
import ctypes

import pytest
import torch

from conftest import rel_err
from list_attn_ref import (ATTN_KEYS, ATTN_SHAPES, attn_tag, collapsed_with, make_attention, mha_compose,
                           reference_grads)

TOL32 = 1e-5


@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=attn_tag)
def test_fixture_equals_both_restatements(golden, shape):
    """nn.MultiheadAttention + mean through list_ref.compose AND the collapsed formula reproduce the reference's outputs
    and every gradient (all-padding bag, trailing padding, repeated id, non-zero padding row; with and without bias)"""
    G = golden("list_attn")
    B, L, E, V, H, bias = shape
    pre = attn_tag(shape)
    keys = G(pre + "/keys")
    assert keys == ["embedding.weight"] + (ATTN_KEYS if bias else [ATTN_KEYS[0], ATTN_KEYS[2]])
    assert G(pre + "/names") == ["B", "N", "E"] and tuple(G(pre + "/out").shape) == (B, 1, E)
    idx = G(pre + "/idx")
    assert int((idx[0] != 0).sum()) == 0 and float(G(pre + "/param/embedding.weight")[0].abs().max()) > 0
    attn = make_attention(E, H, bias, {k[len("attention."):]: G(f"{pre}/param/{k}") for k in keys[1:]})
    for fn in (mha_compose, collapsed_with):
        y, grads = reference_grads(lambda w, a: fn(w, idx, a, "mean", padding_idx=0), G(pre + "/param/embedding.weight"),
                                   attn, G(pre + "/gout"))
        assert rel_err(y, G(pre + "/out")) <= TOL32, fn.__name__
        for k in keys:
            assert rel_err(grads[k], G(f"{pre}/grad/{k}")) <= TOL32, (fn.__name__, k)
        assert float(grads["embedding.weight"][0].abs().max()) == 0.0


@pytest.mark.parametrize("B,L,E,H,bias", [(7, 50, 64, 4, False), (3, 64, 128, 8, True)])
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_collapsed_formula_equals_the_composition(B, L, E, H, bias, mode):
    g = torch.Generator().manual_seed(40 + L + E + H)
    V = 90
    idx = torch.randint(0, V, (B, L), generator=g)
    idx[0] = 0
    w = torch.randn(V, E, generator=g)
    attn = make_attention(E, H, bias, generator=g)
    gout = torch.randn(B, 1, E, generator=g)
    y0, g0 = reference_grads(lambda w_, a: mha_compose(w_, idx, a, mode, padding_idx=0), w, attn, gout)
    g0 = {k: v.clone() for k, v in g0.items()}
    y1, g1 = reference_grads(lambda w_, a: collapsed_with(w_, idx, a, mode, padding_idx=0), w, attn, gout)
    assert rel_err(y1, y0) <= TOL32
    assert sorted(g0) == sorted(g1) and len(g0) == (5 if bias else 3)
    for k in g0:
        assert rel_err(g1[k], g0[k]) <= TOL32, k


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_attn_pool_path_rule(lib):
    from torecsys_amd import functional as F_
    for dtype, code in ((torch.float32, 0), (torch.bfloat16, 1)):
        for E, H in [(64, 1), (64, 4), (128, 8), (16, 2), (10, 5), (8, 1)]:
            for L in range(1, 65):
                p = lib.trs_attn_pool_path(L, E, H, code)
                assert p in (1, 2), (L, E, H, dtype)
                assert F_.attn_pool_path(L, E, H, dtype) == p
                if dtype == torch.float32:
                    assert p == 1                    # exact fp32: vector FMA only
    for E, H in [(64, 1), (64, 4), (128, 8), (32, 2), (32, 1), (128, 1), (128, 2)]:
        assert lib.trs_attn_pool_path(50, E, H, 1) == 2, (E, H)      # bf16, E in {32, 64, 128}, d in {16, 32, 64, 128}: MFMA
    for code in (0, 1):
        assert lib.trs_attn_pool_path(65, 64, 4, code) == 0
        assert lib.trs_attn_pool_path(0, 64, 4, code) == 0
        assert lib.trs_attn_pool_path(50, 256, 4, code) == 0
        assert lib.trs_attn_pool_path(50, 64, 3, code) == 0
        assert lib.trs_attn_pool_path(50, 10, 4, code) == 0
    assert lib.trs_attn_pool_path(50, 64, 4, 7) == 0
    assert F_.attn_pool_path(50, 64, 4, torch.float16) == 0


def test_attn_pool_entries_validate_arguments_without_gpu(lib):
    from torecsys_amd import _abi
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    fwd, bwd = lib.trs_attn_pool_fwd, lib.trs_attn_pool_bwd
    # (table, V, E, dtype, idx, idx_dtype, B, L, w_qk, b_qk, H, mode, out, err_flag, stream)
    assert fwd(null, 10, 16, 0, one, 0, 2, 5, one, null, 2, 1, one, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, 10, 16, 0, one, 0, 2, 5, null, null, 2, 1, one, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, 10, 16, 0, one, 0, 2, 5, one, null, 2, 1, null, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, 10, 16, 7, one, 0, 2, 5, one, null, 2, 1, one, null, null) == -2 and "dtype" in _abi.last_error()
    assert fwd(one, 10, 16, 0, one, 5, 2, 5, one, null, 2, 1, one, null, null) == -2 and "idx dtype" in _abi.last_error()
    assert fwd(one, 10, 16, 0, one, 0, 2, 5, one, null, 2, 2, one, null, null) == -2 and "mode" in _abi.last_error()
    assert fwd(one, 10, 16, 0, one, 0, 2, 65, one, null, 2, 1, one, null, null) == -2 and "L=65" in _abi.last_error()
    assert fwd(one, 10, 256, 0, one, 0, 2, 5, one, null, 2, 1, one, null, null) == -2 and "E=256" in _abi.last_error()
    assert fwd(one, 10, 16, 0, one, 0, 2, 5, one, null, 3, 1, one, null, null) == -2 and "H=3" in _abi.last_error()
    assert fwd(null, 10, 16, 0, null, 0, 0, 5, null, null, 2, 1, null, null, null) == 0          # an empty batch is a no-op
    # (..., mode, gout, dx, dw_part, db_part, blocks, workspace, ws_bytes, err_flag, stream)
    assert bwd(one, 10, 16, 0, one, 0, 2, 5, one, null, 2, 1, null, one, one, one, 2, null, 0, null, null) == -1
    assert "NULL" in _abi.last_error()
    assert bwd(one, 10, 16, 0, one, 0, 2, 5, one, null, 2, 1, one, one, null, one, 2, null, 0, null, null) == -1
    assert bwd(one, 10, 16, 9, one, 0, 2, 5, one, null, 2, 1, one, one, one, one, 2, null, 0, null, null) == -2
    assert "dtype" in _abi.last_error()
    assert bwd(one, 10, 16, 0, one, 0, 2, 5, one, null, 2, 4, one, one, one, one, 2, null, 0, null, null) == -2
    assert bwd(one, 10, 16, 0, one, 0, 2, 70, one, null, 2, 1, one, one, one, one, 2, null, 0, null, null) == -2
    assert bwd(one, 10, 16, 0, one, 0, 2, 5, one, null, 2, 1, one, one, one, one, 3, null, 0, null, null) == -1
    assert "blocks" in _abi.last_error()
    # the probabilities of every head stay in LDS unless H * L floats do not fit beside the sample
    assert lib.trs_attn_pool_bwd_workspace_bytes(8, 50, 64, 4) == 0
    assert lib.trs_attn_pool_bwd_workspace_bytes(8, 64, 128, 128) == 8 * 128 * 64 * 4
    with pytest.raises(RuntimeError, match="trs_attn_pool_fwd failed"):
        _abi.call("trs_attn_pool_fwd", null, 10, 16, 0, null, 0, 2, 5, null, null, 2, 1, null, null, null)


def test_functional_argument_errors():
    from torecsys_amd import functional as F_
    w, ix = torch.zeros(5, 8), torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError, match="mode must be one of"):
        F_.attn_pool(w, ix, torch.zeros(16, 8), None, 2, "max")
    with pytest.raises(ValueError, match="w_qk must be"):
        F_.attn_pool(w, ix, torch.zeros(24, 8), None, 2, "mean")
    with pytest.raises(NotImplementedError, match="does not cover"):
        F_.attn_pool(w, ix, torch.zeros(16, 8), None, 3, "mean")
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.attn_pool(w, ix, torch.zeros(16, 8), None, 2, "mean")


def test_module_keeps_the_composition_off_the_device_and_when_switched_off(monkeypatch):
    """the module decides per call; a CPU module, a refused shape and TRS_ATTN_POOL=0 never reach attn_pool"""
    from torecsys_amd import inputs as I
    m = I.ListIndicesEmbedding(embed_size=8, field_size=9, use_attn=True, num_heads=2, output_method="avg_pooling")
    ix = torch.zeros(2, 3, dtype=torch.long)
    assert m._attn_pool_mode(ix) is None                                  # CPU table
    keys = list(m.state_dict().keys())
    assert keys == ["embedding.weight"] + ATTN_KEYS
    for method, want in (("max_pooling", None), ("none", None)):
        mm = I.ListIndicesEmbedding(embed_size=8, field_size=9, use_attn=True, num_heads=2, output_method=method)
        assert mm._attn_pool_mode(ix) is want
    assert I.ATTN_POOL is True

"""ListIndicesEmbedding / bag pooling, host side (no GPU): constructor parity with the reference (captured in
tests/golden/list.npz), error behaviour, the fixture against the plain torch composition the GPU tests use, argument
validation of the new C-ABI entries, patch() / unpatch()."""
import ctypes
import sys
import types

import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from list_ref import LIST_CASES, LIST_SHAPES, POOL, case_tag, compose, compose_chunked, shape_tag

ATTN_KEYS = ["attention.in_proj_weight", "attention.in_proj_bias", "attention.out_proj.weight", "attention.out_proj.bias"]


@pytest.mark.parametrize("shape", LIST_SHAPES)
@pytest.mark.parametrize("method,heads", LIST_CASES)
def test_constructor_parity_with_the_reference(golden, shape, method, heads):
    from torecsys_amd.inputs import ListIndicesEmbedding
    G = golden("list")
    B, L, E, V = shape
    pre = f"{shape_tag(shape)}/{case_tag(method, heads)}"
    kw = dict(use_attn=True, num_heads=heads) if heads else {}
    m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method, **kw)
    assert list(m.state_dict().keys()) == G(pre + "/keys")
    assert list(m.state_dict().keys()) == ["embedding.weight"] + (ATTN_KEYS if heads else [])
    assert [len(m), m.field_size, m.embed_size, m.padding_idx, m.length] == G(pre + "/attrs").tolist()
    assert m.use_attn is bool(heads) and m.output_method == method
    assert float(m.embedding.weight.detach()[0].abs().max()) == 0.0          # padding_idx defaults to 0: a zero row
    if heads:
        assert m.attn_args == {"embed_dim": E, "num_heads": heads, "dropout": 0.0, "bias": True, "add_bias_kv": False,
                               "add_zero_attn": False}
        assert isinstance(m.attention, nn.MultiheadAttention)
    for k in G(pre + "/keys"):
        assert tuple(m.state_dict()[k].shape) == tuple(G(f"{pre}/param/{k}").shape)


def test_constructor_errors_and_pretrained_table():
    from torecsys_amd.inputs import ListIndicesEmbedding
    with pytest.raises(ValueError, match="output_method only allows"):
        ListIndicesEmbedding(embed_size=4, field_size=5, output_method="median")
    with pytest.raises(ValueError, match="missing required arguments"):
        ListIndicesEmbedding(embed_size=4)
    with pytest.raises(ValueError, match="missing required arguments"):
        ListIndicesEmbedding(field_size=4)
    w = nn.Parameter(torch.randn(7, 12))
    m = ListIndicesEmbedding(nn_embedding=w)
    assert (m.field_size, m.embed_size, m.padding_idx, len(m)) == (7, 12, None, 12)
    assert torch.equal(m.embedding.weight, w) and not m.embedding.weight.requires_grad          # from_pretrained: frozen
    assert list(m.state_dict().keys()) == ["embedding.weight"]
    for method in ("mean", "sum"):      # the reference raises at forward for these; the drop-in builds and serves them
        assert ListIndicesEmbedding(embed_size=4, field_size=5, output_method=method).output_method == method
    with pytest.raises(NotImplementedError):
        m.show_attention(torch.zeros(1, 3, dtype=torch.long))
    from torecsys_amd.optim import FusedSparseSGD
    opt = FusedSparseSGD(lr=0.1)
    assert ListIndicesEmbedding(embed_size=4, field_size=5).set_fused_optimizer(opt).fused_optimizer is opt
    with pytest.raises(NotImplementedError, match="max_pooling"):
        ListIndicesEmbedding(embed_size=4, field_size=5, output_method="max_pooling").set_fused_optimizer(opt)


def test_cpu_tensors_are_rejected_not_served_by_eager_torch():
    from torecsys_amd.inputs import ListIndicesEmbedding
    m = ListIndicesEmbedding(embed_size=4, field_size=5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 3, dtype=torch.long))
    from torecsys_amd import functional as F_
    with pytest.raises(ValueError, match="mode must be one of"):
        F_.bag_pool(torch.zeros(5, 4), torch.zeros(2, 3, dtype=torch.long), "median")
    with pytest.raises(NotImplementedError, match="max pooling with a fused"):
        F_.bag_pool(torch.zeros(5, 4), torch.zeros(2, 3, dtype=torch.long), "max", opt=object())


@pytest.mark.parametrize("shape", LIST_SHAPES)
@pytest.mark.parametrize("method,heads", LIST_CASES)
def test_fixture_equals_the_plain_torch_composition(golden, shape, method, heads):
    """The restatement the GPU tests use at large sizes (F.embedding -> sum(1)/L | max(1), list_ref.compose) reproduces
    the reference's own outputs and gradients, fp32 <= 1e-6 -- ties, repeated ids, all-padding bags, non-zero padding row."""
    G = golden("list")
    B, L, E, V = shape
    pre = f"{shape_tag(shape)}/{case_tag(method, heads)}"
    idx = G(f"{shape_tag(shape)}/idx")
    assert int((idx[0] != 0).sum()) == 0                                         # the all-padding bag is there
    w = G(pre + "/param/embedding.weight").clone().requires_grad_()
    assert float(w.detach()[0].abs().max()) > 0 and torch.equal(w[3], w[4])               # non-zero padding row, the tie rows
    attn = None
    if heads:
        attn = nn.MultiheadAttention(embed_dim=E, num_heads=heads)
        attn.load_state_dict({k[len("attention."):]: G(f"{pre}/param/{k}") for k in ATTN_KEYS})
    y = compose(w, idx, POOL[method], padding_idx=0, attention=attn)
    assert G(pre + "/names") == ["B", "N", "E"]
    assert tuple(y.shape) == tuple(G(pre + "/out").shape) == ((B, L, E) if method == "none" else (B, 1, E))
    assert rel_err(y, G(pre + "/out")) <= 1e-6
    (y * G(pre + "/gout")).sum().backward()
    assert rel_err(w.grad, G(pre + "/grad/embedding.weight")) <= 1e-6
    assert float(w.grad[0].abs().max()) == 0.0 == float(G(pre + "/grad/embedding.weight")[0].abs().max())
    if not heads and method != "none":      # the chunked, graph-free form of the same composition (full-size GPU test)
        yc, gc = compose_chunked(w, idx, POOL[method], G(pre + "/gout"), padding_idx=0, chunk=4)
        assert rel_err(yc, G(pre + "/out")) <= 1e-6 and rel_err(gc, G(pre + "/grad/embedding.weight")) <= 1e-6
    if heads:
        for k in ATTN_KEYS:
            assert rel_err(dict(attn.named_parameters())[k[len("attention."):]].grad, G(f"{pre}/grad/{k}")) <= 1e-6
    if method == "max_pooling" and not heads and L >= 4:
        # rows 3 and 4 are equal and the largest: the FIRST position of the bag that holds the maximum takes the gradient
        g, go = G(pre + "/grad/embedding.weight"), G(pre + "/gout")
        first3 = [b for b in range(B) if 3 in idx[b].tolist() and (4 not in idx[b].tolist()
                                                                 or idx[b].tolist().index(3) < idx[b].tolist().index(4))]
        first4 = [b for b in range(B) if 4 in idx[b].tolist() and (3 not in idx[b].tolist()
                                                                 or idx[b].tolist().index(4) < idx[b].tolist().index(3))]
        assert first3 and first4                                                 # both orders occur
        assert rel_err(g[3], go[first3, 0].sum(0)) <= 1e-6 and rel_err(g[4], go[first4, 0].sum(0)) <= 1e-6


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_bag_entries_validate_arguments_without_gpu(lib):
    from torecsys_amd import _abi
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    fwd = lib.trs_bag_pool_fwd
    assert fwd(null, 10, 4, 0, one, 0, 2, 3, 0, one, null, null, null) == -1 and "NULL" in _abi.last_error()
    assert fwd(one, 10, 4, 0, one, 0, 2, 3, 2, one, null, null, null) == -1 and "argmax" in _abi.last_error()
    assert fwd(one, 10, 4, 7, one, 0, 2, 3, 0, one, null, null, null) == -2 and "dtype" in _abi.last_error()
    assert fwd(one, 10, 4, 0, one, 5, 2, 3, 0, one, null, null, null) == -2 and "idx dtype" in _abi.last_error()
    assert fwd(one, 10, 4, 0, one, 0, 2, 3, 3, one, one, null, null) == -1 and "mode" in _abi.last_error()
    assert fwd(one, 10, 4, 0, one, 0, 2, 0, 0, one, null, null, null) == -1 and "L=0" in _abi.last_error()
    assert fwd(one, 10, 4, 0, one, 0, 2, 65536, 0, one, null, null, null) == -1 and "65535" in _abi.last_error()
    assert fwd(null, 10, 4, 0, null, 0, 0, 3, 0, null, null, null, null) == 0          # an empty batch is a no-op
    bwd = lib.trs_scatter_rows_argmax
    ws = lib.trs_scatter_argmax_workspace_bytes(600, 4)
    assert ws >= 8 + 4 * 4
    assert bwd(null, one, one, one, 600, 10, 4, 3, 0, -1, one, one, ws, null) == -1 and "NULL" in _abi.last_error()
    assert bwd(one, one, one, one, 600, 10, 4, 3, 9, -1, one, one, ws, null) == -2 and "dtype" in _abi.last_error()
    assert bwd(one, one, one, one, 600, 10, 4, 0, 0, -1, one, one, ws, null) == -1 and "L=0" in _abi.last_error()
    assert bwd(one, one, one, one, 601, 10, 4, 3, 0, -1, one, one, ws, null) == -1 and "multiple" in _abi.last_error()
    assert bwd(one, one, one, one, 600, 10, 4, 3, 0, -1, one, one, 8, null) == -6 and "workspace" in _abi.last_error()
    skip = lib.trs_csr_build_skip
    cws = lib.trs_csr_workspace_bytes(10, 600)
    assert skip(one, 0, null, 200, 3, 10, 10, one, one, one, cws, null, null) == -1 and "skip_row" in _abi.last_error()
    assert skip(one, 0, null, 200, 3, 10, -2, one, one, one, cws, null, null) == -1 and "skip_row" in _abi.last_error()
    assert skip(null, 0, null, 200, 3, 10, 0, one, one, one, cws, null, null) == -1 and "NULL" in _abi.last_error()
    assert skip(one, 4, null, 200, 3, 10, 0, one, one, one, cws, null, null) == -2 and "dtype" in _abi.last_error()
    with pytest.raises(RuntimeError, match="trs_bag_pool_fwd failed"):
        _abi.call("trs_bag_pool_fwd", null, 10, 4, 0, null, 0, 2, 3, 0, null, null, null, null)


def test_patch_rebinds_and_restores_list_indices_embedding():
    import torecsys_amd
    from torecsys_amd import inputs as I
    pkg = types.ModuleType("fake_list_trs")
    inp = types.ModuleType("fake_list_trs.inputs")
    base = types.ModuleType("fake_list_trs.inputs.base")

    class Old:      # stand-in for the reference class
        pass

    inp.ListIndicesEmbedding = base.ListIndicesEmbedding = Old
    inp.SingleIndexEmbedding = Old
    mods = (pkg, inp, base)
    for m in mods:
        sys.modules[m.__name__] = m
    try:
        torecsys_amd.patch(pkg, heads=False)
        assert inp.ListIndicesEmbedding is I.ListIndicesEmbedding and base.ListIndicesEmbedding is I.ListIndicesEmbedding
        assert I.ListIndicesEmbedding.__name__ == "ListIndicesEmbedding"      # the router dispatches on the class name
        assert I.ListIndicesEmbedding not in I._SIDE_LOOKUPS
        torecsys_amd.unpatch()
        assert inp.ListIndicesEmbedding is Old and base.ListIndicesEmbedding is Old and inp.SingleIndexEmbedding is Old
    finally:
        torecsys_amd.unpatch()
        for m in mods:
            sys.modules.pop(m.__name__, None)

"""Host side of bag_pool(exclude_padding=, per_sample_weights=): the CPU restatement the GPU tests compare against
(tests/bag_masked_ref.py) is pinned to torch.nn.functional.embedding_bag + autograd in fp64; every argument error of
functional.bag_pool, of ListIndicesEmbedding and of the new C entries is raised before a device is needed; Inputs hands
the ``weights`` column of the schema to the module."""
import ctypes

import pytest
import torch

from bag_masked_ref import embedding_bag_ref, masked_bag


def _bags(g, B, L, V, pad):
    idx = torch.randint(0, V - 1, (B, L), generator=g)
    idx = idx + (idx >= pad).long()                      # any id but the padding one
    keep = torch.randint(0, L + 1, (B,), generator=g)
    idx = torch.where(torch.arange(L).view(1, L) < keep.view(B, 1), idx, torch.full_like(idx, pad))
    idx[0] = pad                                         # an empty bag
    idx[1] = torch.where(idx[1] == pad, torch.full_like(idx[1], (pad + 1) % V), idx[1])      # a full one
    if L > 1:
        idx[2, 0::2] = pad                               # padding in between
    return idx


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("pad", [0, 12])
@pytest.mark.parametrize("L", [1, 7])
@pytest.mark.parametrize("mode,weighted", [("sum", False), ("mean", False), ("max", False), ("sum", True)])
def test_restatement_equals_embedding_bag_fp64(mode, weighted, L, pad):
    B, V, E = 9, 13, 5
    g = torch.Generator().manual_seed(3 + L + pad)
    idx = _bags(g, B, L, V, pad)
    w = torch.randn(V, E, generator=g, dtype=torch.float64)
    psw = torch.randn(B, L, generator=g, dtype=torch.float64) if weighted else None
    gout = torch.randn(B, E, generator=g, dtype=torch.float64)
    out, grad, dw = masked_bag(w, idx, mode, pad=pad, exclude=True, psw=psw, gout=gout)
    want_out, want_grad, want_dw = embedding_bag_ref(w, idx, mode, pad, psw, gout)
    assert torch.allclose(out, want_out, rtol=1e-13, atol=1e-13)
    assert torch.allclose(grad, want_grad, rtol=1e-13, atol=1e-13)
    assert float(out[0].abs().max()) == 0.0 and float(grad[pad].abs().max()) == 0.0
    if weighted:
        assert torch.allclose(dw, want_dw, rtol=1e-13, atol=1e-13)
        assert float(dw[idx == pad].abs().max()) == 0.0 and float(want_dw[idx == pad].abs().max()) == 0.0


def test_restatement_weighted_sum_without_exclusion_fp64():
    """every position counts and the padding row is read; it only receives no gradient"""
    B, L, V, E, pad = 9, 7, 13, 5, 0
    g = torch.Generator().manual_seed(8)
    idx = _bags(g, B, L, V, pad)
    w = torch.randn(V, E, generator=g, dtype=torch.float64)
    psw = torch.randn(B, L, generator=g, dtype=torch.float64)
    gout = torch.randn(B, E, generator=g, dtype=torch.float64)
    out, grad, dw = masked_bag(w, idx, "sum", pad=pad, exclude=False, psw=psw, gout=gout)
    want_out, want_grad, want_dw = embedding_bag_ref(w, idx, "sum", None, psw, gout)
    assert torch.allclose(out, want_out, rtol=1e-13, atol=1e-13)
    assert torch.allclose(dw, want_dw, rtol=1e-13, atol=1e-13)
    assert float(out[0].abs().max()) > 0.0 and float(dw[0].abs().max()) > 0.0
    assert float(grad[pad].abs().max()) == 0.0 and float(want_grad[pad].abs().max()) > 0.0
    want_grad[pad] = 0
    assert torch.allclose(grad, want_grad, rtol=1e-13, atol=1e-13)


def test_restatement_out_of_range_id_is_a_live_zero_row():
    w = torch.arange(12, dtype=torch.float64).reshape(4, 3) + 1
    idx = torch.tensor([[1, 9, 0, 0], [0, 0, 0, 0]])
    out, grad, _ = masked_bag(w, idx, "mean", pad=0, exclude=True, gout=torch.ones(2, 3, dtype=torch.float64))
    assert torch.equal(out[0], w[1] / 2) and float(out[1].abs().max()) == 0.0
    assert torch.equal(grad[1], torch.full((3,), 0.5, dtype=torch.float64)) and float(grad[[0, 2, 3]].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ argument errors
def test_bag_pool_argument_errors_on_cpu_tensors():
    from torecsys_amd import functional as F_
    from torecsys_amd.optim import FusedSparseSGD
    w = torch.randn(10, 8)
    idx = torch.zeros(2, 3, dtype=torch.long)
    psw = torch.ones(2, 3)
    with pytest.raises(ValueError, match="padding_idx"):
        F_.bag_pool(w, idx, "sum", exclude_padding=True)
    with pytest.raises(ValueError, match="padding row"):
        F_.bag_pool(w, idx, "sum", padding_idx=10, exclude_padding=True)
    for mode in ("mean", "max"):
        with pytest.raises(ValueError, match="per_sample_weights"):
            F_.bag_pool(w, idx, mode, padding_idx=0, per_sample_weights=psw)
        with pytest.raises(ValueError, match="per_sample_weights"):
            F_.bag_pool(w, idx, mode, padding_idx=0, exclude_padding=True, per_sample_weights=psw)
    with pytest.raises(ValueError, match=r"\(B, L\)"):
        F_.bag_pool(w, idx, "sum", per_sample_weights=torch.ones(2, 4))
    with pytest.raises(ValueError, match=r"\(B, L\)"):
        F_.bag_pool(w, idx, "sum", per_sample_weights=torch.ones(6))
    with pytest.raises(ValueError, match="dtype"):
        F_.bag_pool(w, idx, "sum", per_sample_weights=psw.double())
    with pytest.raises(ValueError, match="dtype"):
        F_.bag_pool(w.bfloat16(), idx, "sum", per_sample_weights=psw)
    with pytest.raises(ValueError, match="device"):
        F_.bag_pool(w, idx, "sum", per_sample_weights=torch.ones(2, 3, device="meta"))
    long_idx = torch.zeros(1, 65535, dtype=torch.long)
    with pytest.raises(ValueError, match="65534"):
        F_.bag_pool(w, long_idx, "max", padding_idx=0, exclude_padding=True)
    with pytest.raises(NotImplementedError, match="per_sample_weights"):
        F_.bag_pool(w, idx, "sum", padding_idx=0, opt=FusedSparseSGD(0.1), per_sample_weights=psw)
    with pytest.raises(NotImplementedError, match="max pooling"):
        F_.bag_pool(w, idx, "max", padding_idx=0, opt=FusedSparseSGD(0.1), exclude_padding=True)
    # valid arguments get as far as the device check: there is no CPU path
    for kw in (dict(exclude_padding=True), dict(per_sample_weights=psw), dict(exclude_padding=True, per_sample_weights=psw)):
        with pytest.raises(RuntimeError, match="HIP"):
            F_.bag_pool(w, idx, "sum", padding_idx=-1, **kw)
    with pytest.raises(RuntimeError, match="HIP"):
        F_.bag_pool(w, long_idx[:, :65534], "max", padding_idx=0, exclude_padding=True)


def test_module_argument_errors_on_cpu():
    from torecsys_amd.inputs import ListIndicesEmbedding
    from torecsys_amd.optim import FusedSparseSGD
    idx = torch.zeros(2, 3, dtype=torch.long)
    psw = torch.ones(2, 3)
    with pytest.raises(NotImplementedError, match="use_attn"):
        ListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, exclude_padding=True)
    with pytest.raises(ValueError, match="none"):
        ListIndicesEmbedding(embed_size=8, field_size=10, output_method="none", exclude_padding=True)
    with pytest.raises(ValueError, match="padding_idx"):
        ListIndicesEmbedding(embed_size=8, field_size=10, padding_idx=None, exclude_padding=True)
    with pytest.raises(ValueError, match="padding_idx"):
        ListIndicesEmbedding(nn_embedding=torch.nn.Parameter(torch.randn(10, 8)), exclude_padding=True)
    with pytest.raises(NotImplementedError, match="use_attn"):
        ListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, output_method="sum")(idx, psw)
    with pytest.raises(ValueError, match="none"):
        ListIndicesEmbedding(embed_size=8, field_size=10, output_method="none")(idx, per_sample_weights=psw)
    for method in ("avg_pooling", "mean", "max_pooling"):
        with pytest.raises(ValueError, match="per_sample_weights"):
            ListIndicesEmbedding(embed_size=8, field_size=10, output_method=method)(idx, psw)
    m = ListIndicesEmbedding(embed_size=8, field_size=10, output_method="sum")
    m.set_schema("tags", weights="tag_weights")
    assert m.schema.inputs == ["tags"] and m.schema.weights == "tag_weights"
    with pytest.raises(NotImplementedError, match="per_sample_weights"):
        m.set_fused_optimizer(FusedSparseSGD(0.1))
    m.set_fused_optimizer(None)
    m2 = ListIndicesEmbedding(embed_size=8, field_size=10, output_method="sum", exclude_padding=True)
    m2.set_fused_optimizer(FusedSparseSGD(0.1))          # masked sum / mean: the existing update walk
    with pytest.raises(NotImplementedError, match="per_sample_weights"):
        m2(idx, psw)
    with pytest.raises(NotImplementedError):
        ListIndicesEmbedding(embed_size=8, field_size=10, output_method="max_pooling",
                             exclude_padding=True).set_fused_optimizer(FusedSparseSGD(0.1))
    # the options add no parameter and no buffer
    plain = ListIndicesEmbedding(embed_size=8, field_size=10)
    assert list(m2.state_dict().keys()) == list(plain.state_dict().keys()) == ["embedding.weight"]
    assert plain.exclude_padding is False and m2.exclude_padding is True
    m3 = ListIndicesEmbedding(embed_size=8, field_size=10)
    m3.set_schema("tags")
    assert m3.schema.inputs == ["tags"] and not hasattr(m3.schema, "weights")


# ------------------------------------------------------------------------------------------------ the C entries
@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_new_entries_reject_bad_arguments_without_a_device(lib):
    from torecsys_amd import _abi
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    EINVAL, EDTYPE = -1, -2

    def fwd(table=p, idx=p, out=p, dtype=0, idt=0, L=4, mode=0, excl=0, wts=null, amax=null, inv=null, V=10):
        return lib.trs_bag_pool_masked_fwd(table, V, 8, dtype, idx, idt, 2, L, mode, excl, wts, out, amax, inv, null, null)

    for kw in (dict(table=null), dict(idx=null), dict(out=null), dict(mode=3), dict(excl=-2), dict(excl=10),
               dict(excl=-1), dict(mode=1, wts=p, inv=p), dict(mode=2, wts=p, amax=p), dict(mode=2), dict(mode=1),
               dict(L=0), dict(L=65536), dict(mode=2, amax=p, L=65535), dict(V=0)):
        assert fwd(**kw) == EINVAL, kw
        assert _abi.last_error().startswith("bag_pool_masked_fwd:"), (kw, _abi.last_error())
    for kw in (dict(dtype=7), dict(idt=7), dict(wts=p, excl=-1, dtype=7)):
        assert fwd(**kw) == EDTYPE, kw
        assert _abi.last_error().startswith("bag_pool_masked_fwd:"), (kw, _abi.last_error())
    assert lib.trs_bag_pool_masked_fwd(null, 10, 8, 0, null, 0, 0, 4, 0, 0, null, null, null, null, null, null) == 0

    def walk(g=p, wts=p, rs=p, perm=p, grad=p, ws=p, BN=8, N=4, dtype=0, ws_bytes=1 << 20, V=10):
        return lib.trs_scatter_rows_weighted(g, wts, rs, perm, BN, V, 8, N, dtype, -1, grad, ws, ws_bytes, null)

    for kw in (dict(g=null), dict(wts=null), dict(rs=null), dict(perm=null), dict(grad=null), dict(ws=null), dict(N=0),
               dict(N=65536), dict(BN=9), dict(V=0)):
        assert walk(**kw) == EINVAL, kw
        assert _abi.last_error().startswith("scatter_rows_weighted:"), (kw, _abi.last_error())
    assert walk(dtype=7) == EDTYPE and _abi.last_error().startswith("scatter_rows_weighted:")
    assert walk(ws_bytes=8) == -6 and _abi.last_error().startswith("scatter_rows_weighted:")       # TRS_EWORKSPACE
    assert walk(BN=1 << 31, N=1) == -3 and _abi.last_error().startswith("scatter_rows_weighted:")  # TRS_ESHAPE
    assert lib.trs_scatter_weighted_workspace_bytes(3200, 64) == lib.trs_scatter_argmax_workspace_bytes(3200, 64) > 0

    def wgrad(g=p, table=p, idx=p, dw=p, dtype=0, idt=0, L=4, excl=0, V=10):
        return lib.trs_bag_weight_grad(g, table, V, 8, dtype, idx, idt, 2, L, excl, dw, null)

    for kw in (dict(g=null), dict(table=null), dict(idx=null), dict(dw=null), dict(L=0), dict(L=65536), dict(excl=-2),
               dict(excl=10), dict(V=0)):
        assert wgrad(**kw) == EINVAL, kw
        assert _abi.last_error().startswith("bag_weight_grad:"), (kw, _abi.last_error())
    for kw in (dict(dtype=7), dict(idt=7)):
        assert wgrad(**kw) == EDTYPE, kw
        assert _abi.last_error().startswith("bag_weight_grad:"), (kw, _abi.last_error())


# ------------------------------------------------------------------------------------------------ Inputs routing
def test_inputs_hands_the_weights_column_to_the_module():
    """a stub with ListIndicesEmbedding's schema: no kernel runs"""
    from torecsys_amd.inputs import Inputs, ListIndicesEmbedding

    class Stub(ListIndicesEmbedding):
        def forward(self, inputs, per_sample_weights=None):
            self.seen = (inputs, per_sample_weights)
            return torch.zeros(inputs.shape[0], 1, self.embed_size).refine_names('B', 'N', 'E')

    weighted = Stub(embed_size=4, field_size=10, output_method="sum")
    weighted.set_schema("tags", weights="tag_weights")
    plain = Stub(embed_size=4, field_size=10, output_method="sum")
    plain.set_schema("cats")
    inp = Inputs(schema={"tags_emb": weighted, "cats_emb": plain})
    batch = {"tags": torch.tensor([[1, 2, 0], [3, 0, 0]]), "tag_weights": torch.tensor([[0.5, 2.0, 0.0], [1.0, 0.0, 0.0]]),
             "cats": torch.tensor([[4, 5], [6, 0]])}
    out = inp(batch)
    assert list(out) == ["tags_emb", "cats_emb"] and out["tags_emb"].names == ("B", "N", "E")
    assert weighted.seen[0] is batch["tags"] and weighted.seen[1] is batch["tag_weights"]
    assert plain.seen[0] is batch["cats"] and plain.seen[1] is None
    with pytest.raises(KeyError):
        inp({"tags": batch["tags"], "cats": batch["cats"]})

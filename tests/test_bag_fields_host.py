"""Ragged bag pooling over F fields of one table, host side (no GPU): the fp64 restatement tests/bag_fields_ref.py pinned
to torch.nn.functional.embedding_bag + autograd per field, the argument checks of the new C entries (error codes and
messages that name the entry, before any launch), and the Python-side validation of functional.bag_pool_fields and
RaggedMultiListIndicesEmbedding."""
import ctypes

import pytest
import torch

from bag_fields_ref import (cut_pow2, embedding_bag_fields, field_major_lengths, field_starts, fields_bag,
                            one_id_long_bags, values_for)
from bag_ragged_ref import boundary_lengths

SIZES = (7, 1, 50)
NF, B, E = 3, 13, 6


def _batch(seed, T=16, trailing=4):
    g = torch.Generator().manual_seed(seed)
    per_field = [boundary_lengths(g, T, B=B) for _ in range(NF)]
    per_field = [ls[f:] + ls[:f] for f, ls in enumerate(per_field)]
    offsets = field_major_lengths(per_field)
    values = values_for(g, offsets, SIZES, trailing)
    w = torch.randn(sum(SIZES), E, generator=g, dtype=torch.float64)
    gout = torch.randn(B, NF, E, generator=g, dtype=torch.float64)
    psw = torch.rand(values.numel(), generator=g, dtype=torch.float64) + 0.5
    return values, offsets, w, gout, psw


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
@pytest.mark.parametrize("mode,weighted", [("sum", False), ("mean", False), ("max", False), ("sum", True)])
def test_restatement_equals_embedding_bag_per_field(mode, weighted, idt):
    values, offsets, w, gout, psw = _batch(1)
    assert offsets.numel() == NF * B + 1 and int(offsets[-1]) == values.numel() - 4
    lens = (offsets[1:] - offsets[:-1]).reshape(NF, B)
    assert bool((lens == 0).any(dim=1).all())                                # every field holds an empty bag
    p = psw if weighted else None
    want = embedding_bag_fields(w, values.to(idt), offsets.to(idt), SIZES, mode, p, gout)
    got = fields_bag(w, values.to(idt), offsets.to(idt), SIZES, mode, p, gout)
    assert tuple(got[0].shape) == (B, NF, E)
    assert _close(got[0], want[0]) and _close(got[1], want[1])
    if weighted:
        assert _close(got[2], want[2]) and float(got[2][int(offsets[-1]):].abs().max()) == 0.0
    empty = (lens == 0).t()                                                  # (B, NF)
    assert float(got[0][empty].abs().max()) == 0.0


def test_restatement_checks_an_id_against_its_own_field():
    w = torch.arange(1, 2 * sum(SIZES) + 1, dtype=torch.float64).reshape(sum(SIZES), 2)
    offsets = torch.tensor([0, 2, 3, 5])                                     # B = 1: one bag per field
    values = torch.tensor([1, 7, 0, 3, 50])                                  # 7 == SIZES[0], 50 == SIZES[2]: outside
    gout = torch.ones(1, NF, 2, dtype=torch.float64)
    out, grad, _ = fields_bag(w, values, offsets, SIZES, "mean", None, gout)
    fo = field_starts(SIZES)
    assert torch.equal(out[0, 0], w[1] / 2) and torch.equal(out[0, 1], w[7]) and torch.equal(out[0, 2], w[8 + 3] / 2)
    assert float(grad[int(fo[1])].abs().max()) == 1.0                        # the neighbour's row 0: its own lookup only
    assert float(grad.sum()) == 2 * (0.5 + 1.0 + 0.5)


def test_batch_builders():
    values, offsets, _, _, _ = _batch(3)
    v2, o2 = cut_pow2(values, offsets)
    for j in range(NF * B):
        ln = int(o2[j + 1] - o2[j])
        assert ln & (ln - 1) == 0
    assert v2.numel() == int(o2[-1]) + 4
    g = torch.Generator().manual_seed(4)
    v3 = one_id_long_bags(g, values, offsets, SIZES)
    for j in range(NF * B):
        bag = v3[int(offsets[j]):int(offsets[j + 1])]
        assert bag.numel() <= 8 or int(bag.min()) == int(bag.max())
        assert bag.numel() == 0 or int(bag.max()) < SIZES[j // B]


# ------------------------------------------------------------------------------------------------ the C entries
@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_workspace_query(lib):
    assert lib.trs_bag_fields_workspace_bytes(39) >= 4 * 40                  # a counter + at most F*B entries
    assert lib.trs_bag_fields_workspace_bytes(0) >= 4
    assert lib.trs_bag_fields_workspace_bytes(39) == lib.trs_bag_ragged_workspace_bytes(39)


def test_argument_errors_without_gpu(lib):
    from torecsys_amd import _abi
    EINVAL, EDTYPE, ESHAPE, EWORKSPACE = -1, -2, -3, -6
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    big = 1 << 20

    def fwd(table=p, dtype=0, values=p, val_dtype=0, n=10, offsets=p, off_dtype=0, n_off=13, B=4, F=3, fo=p, mode=0,
            weights=null, out=p, argmax=null, inv_cnt=null, ws=p, ws_bytes=big):
        return lib.trs_bag_pool_fields_fwd(table, 20, 8, dtype, values, val_dtype, n, offsets, off_dtype, n_off, B, F, fo,
                                           mode, weights, out, argmax, inv_cnt, ws, ws_bytes, null, null)

    bad = [(dict(table=null), EINVAL, "NULL"), (dict(offsets=null), EINVAL, "NULL"), (dict(out=null), EINVAL, "NULL"),
           (dict(values=null), EINVAL, "NULL"), (dict(ws=null), EINVAL, "NULL"), (dict(fo=null), EINVAL, "field_offsets"),
           (dict(F=0, n_off=1), EINVAL, "F=0"), (dict(F=-2), EINVAL, "F=-2"), (dict(mode=3), EINVAL, "mode"),
           (dict(n_off=12), EINVAL, "offsets"), (dict(n_off=14), EINVAL, "offsets"), (dict(n_off=5), EINVAL, "offsets"),
           (dict(n=2 ** 31 - 1), ESHAPE, "int32"), (dict(B=(2 ** 31 - 1 + 2) // 3, n_off=2 ** 31 + 2), ESHAPE, "int32"),
           (dict(B=2 ** 62, n_off=5), ESHAPE, "int32"),
           (dict(mode=1, weights=p, inv_cnt=p), EINVAL, "weights"), (dict(mode=2, weights=p, argmax=p), EINVAL, "weights"),
           (dict(mode=2), EINVAL, "argmax"), (dict(mode=1), EINVAL, "inv_cnt"), (dict(dtype=7), EDTYPE, "dtype"),
           (dict(val_dtype=5), EDTYPE, "values dtype"), (dict(off_dtype=5), EDTYPE, "offsets dtype"),
           (dict(ws_bytes=4), EWORKSPACE, "workspace")]
    for kw, code, word in bad:
        assert fwd(**kw) == code, kw
        msg = _abi.last_error()
        assert msg.startswith("bag_pool_fields_fwd:") and word in msg, (kw, msg)
    # an empty batch touches nothing, whatever else is handed in
    assert fwd(B=0, n_off=1, table=null, offsets=null, out=null, ws=null, values=null, fo=null) == 0

    def owner(values=p, val_dtype=0, n=10, offsets=p, off_dtype=0, n_off=13, B=4, F=3, fo=p, out_row_of=p, rows=p):
        return lib.trs_bag_owner_fields(values, val_dtype, n, offsets, off_dtype, n_off, B, F, 20, fo, out_row_of, rows,
                                        null)

    bad = [(dict(values=null), EINVAL), (dict(offsets=null), EINVAL), (dict(fo=null), EINVAL),
           (dict(out_row_of=null), EINVAL), (dict(rows=null), EINVAL), (dict(F=0), EINVAL), (dict(n_off=12), EINVAL),
           (dict(B=2 ** 40), ESHAPE), (dict(val_dtype=3), EDTYPE), (dict(off_dtype=3), EDTYPE)]
    for kw, code in bad:
        assert owner(**kw) == code, kw
        assert _abi.last_error().startswith("bag_owner_fields:"), (kw, _abi.last_error())
    assert owner(n=0, values=null, offsets=null, out_row_of=null, rows=null) == 0      # no position: nothing to map


# ------------------------------------------------------------------------------------------------ Python validation
def test_python_validation_without_gpu():
    from torecsys_amd import functional as F_
    w = torch.zeros(sum(SIZES), 4)
    fo = field_starts(SIZES)
    values, off = torch.tensor([1, 0, 3]), torch.tensor([0, 1, 2, 3])
    with pytest.raises(ValueError, match="mode"):
        F_.bag_pool_fields(w, values, off, fo, "median")
    with pytest.raises(ValueError, match=r"F\*B \+ 1"):
        F_.bag_pool_fields(w, values, torch.tensor([0, 1, 2, 3, 3]), fo, "sum")
    with pytest.raises(ValueError, match=r"F\*B \+ 1"):
        F_.bag_pool_fields(w, values, torch.zeros(0, dtype=torch.int64), fo, "sum")
    with pytest.raises(ValueError, match="only supported for mode='sum'"):
        F_.bag_pool_fields(w, values, off, fo, "mean", per_sample_weights=torch.ones(3))
    with pytest.raises(ValueError, match="only supported for mode='sum'"):
        F_.bag_pool_fields(w, values, off, fo, "max", per_sample_weights=torch.ones(3))
    with pytest.raises(ValueError, match="dtype"):
        F_.bag_pool_fields(w, values, off, fo, "sum", per_sample_weights=torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\(n,\)"):
        F_.bag_pool_fields(w, values, off, fo, "sum", per_sample_weights=torch.ones(4))
    with pytest.raises(ValueError, match=r"\(n,\) or \(n, 1\)"):
        F_.bag_pool_fields(w, values.reshape(1, 3), off, fo)
    with pytest.raises(ValueError, match="field_offsets"):
        F_.bag_pool_fields(w, values, off, fo.int(), "sum")
    with pytest.raises(ValueError, match="field_offsets"):
        F_.bag_pool_fields(w, values, off, fo[:1], "sum")
    with pytest.raises(TypeError):
        F_.bag_pool_fields(w, values.float(), off, fo, "sum")
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.bag_pool_fields(w, values, off, fo, "sum")


def test_module_contract_without_gpu():
    import torecsys_amd
    from torecsys_amd.inputs import MultiIndicesEmbedding, RaggedMultiListIndicesEmbedding
    assert torecsys_amd.RaggedMultiListIndicesEmbedding is RaggedMultiListIndicesEmbedding
    m = RaggedMultiListIndicesEmbedding(4, list(SIZES))
    ref = MultiIndicesEmbedding(4, list(SIZES))
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys()) == ["embedding.weight"]
    assert tuple(m.embedding.weight.shape) == (sum(SIZES), 4) and len(m) == NF
    assert torch.equal(m.offsets, field_starts(SIZES)) and m.offsets.dtype == torch.int64
    assert torch.equal(m.offsets[:-1], ref.offsets)                          # the same rows per field
    m.load_state_dict(ref.state_dict())                                      # a MultiIndicesEmbedding checkpoint loads
    assert m.double().offsets.dtype == torch.int64                           # the buffer follows .to(), stays an index
    assert m.output_method == "avg_pooling"
    with pytest.raises(ValueError):
        RaggedMultiListIndicesEmbedding(4, list(SIZES), output_method="none")
    with pytest.raises(ValueError):
        RaggedMultiListIndicesEmbedding(4, [])
    with pytest.raises(ValueError):
        RaggedMultiListIndicesEmbedding(None, list(SIZES))
    with pytest.raises(ValueError, match="rows"):
        RaggedMultiListIndicesEmbedding(4, list(SIZES), nn_embedding=torch.nn.Parameter(torch.zeros(5, 4)))
    pre = RaggedMultiListIndicesEmbedding(None, list(SIZES), nn_embedding=torch.nn.Parameter(torch.ones(sum(SIZES), 8)))
    assert pre.embed_size == 8 and list(pre.state_dict().keys()) == ["embedding.weight"]
    # set_schema: the contract of RaggedListIndicesEmbedding
    with pytest.raises(TypeError):
        m.set_schema("tags")
    with pytest.raises(TypeError):
        m.set_schema("tags", offsets="tag_offsets", weights=3)
    m.set_schema("tags", offsets="tag_offsets")
    assert m.schema.inputs == ["tags"] and m.schema.offsets == "tag_offsets" and m.schema.weights is None
    m.set_schema(["tags"], offsets="tag_offsets", weights="tag_weights")
    assert m.schema.inputs == ["tags"] and m.schema.weights == "tag_weights"
    with pytest.raises(NotImplementedError):
        m.set_fused_optimizer(object())
    assert m.set_fused_optimizer(None) is m

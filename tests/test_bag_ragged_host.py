"""Ragged bag pooling, host side (no GPU): the fp64 restatement tests/bag_ragged_ref.py pinned to
torch.nn.functional.embedding_bag(ids, w, offsets, ...) + autograd on the CPU wherever ATen serves the case, the
lookup -> sample map pinned to torch.bucketize arithmetic, and the argument checks of the new C entries (error codes and
messages that name the entry, before any launch)."""
import ctypes

import pytest
import torch

from bag_ragged_ref import (bag_bounds, bag_owner, bags_from_lengths, boundary_lengths, embedding_bag_ref, pad_bags,
                            pow2_lengths, pow2_live, ragged_bag)

V, E, PAD = 53, 6, 0


def _batch(seed, T=16, trailing=5):
    g = torch.Generator().manual_seed(seed)
    lengths = boundary_lengths(g, T) + [0]                                   # the LAST bag is empty too
    ids, offsets = bags_from_lengths(g, lengths, V, PAD, trailing=trailing, sprinkle=0.2, all_pad=(5,))
    w = torch.randn(V, E, generator=g, dtype=torch.float64)
    gout = torch.randn(len(lengths), E, generator=g, dtype=torch.float64)
    psw = torch.rand(ids.numel(), generator=g, dtype=torch.float64) + 0.5
    return ids, offsets, w, gout, psw


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
@pytest.mark.parametrize("last", [True, False])
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_restatement_equals_embedding_bag_with_padding_idx(mode, last, idt):
    """empty first, middle (zero length; and the bag of nothing but padding) and LAST bags -- offsets[B - 1] == n without
    include_last_offset, offsets[-2] == offsets[-1] with it; ids behind the last bag with include_last_offset"""
    ids, offsets, w, gout, _ = _batch(1)
    if not last:
        ids, offsets = ids[:int(offsets[-1])], offsets[:-1]
        assert int(offsets[-1]) == ids.numel()
    else:
        assert int(offsets[-2]) == int(offsets[-1]) < ids.numel()
    lens = [e - b for b, e in bag_bounds(offsets, ids.numel(), last)]
    assert lens[0] == 0 and lens[12] == 0 and lens[-1] == 0 and lens[-2] > 0
    assert bool((ids[sum(lens[:5]):sum(lens[:6])] == PAD).all())
    # ATen takes the last offset for the number of ids (its documentation asks for that): it is handed the ids up to
    # there, the restatement all of them -- the ids behind the last bag belong to no bag
    covered = ids[:int(offsets[-1])] if last else ids
    want = embedding_bag_ref(w, covered.to(idt), offsets.to(idt), mode, PAD, None, gout, last)
    got = ragged_bag(w, ids.to(idt), offsets.to(idt), mode, PAD, True, None, gout, last)
    assert _close(got[0], want[0]) and _close(got[1], want[1])
    assert float(got[0][5].abs().max()) == 0.0 and float(got[0][0].abs().max()) == 0.0
    assert float(got[0][-1].abs().max()) == 0.0 and float(want[0][-1].abs().max()) == 0.0
    assert float(got[1][PAD].abs().max()) == 0.0


@pytest.mark.parametrize("last", [True, False])
def test_restatement_equals_embedding_bag_weighted_and_plain(last):
    ids, offsets, w, gout, psw = _batch(2)
    if not last:
        ids, offsets, psw = ids[:int(offsets[-1])], offsets[:-1], psw[:int(offsets[-1])]
    m = int(offsets[-1]) if last else ids.numel()                           # ATen: the ids that a bag holds (see above)
    want = embedding_bag_ref(w, ids[:m], offsets, "sum", PAD, psw[:m], gout, last)
    got = ragged_bag(w, ids, offsets, "sum", PAD, True, psw, gout, last)
    assert _close(got[0], want[0]) and _close(got[1], want[1]) and _close(got[2][:m], want[2])
    assert float(got[2][ids == PAD].abs().max()) == 0.0
    if last:
        assert float(got[2][m:].abs().max()) == 0.0                         # ids that no bag holds
    # nothing excluded: every position counts; only the padding row's gradient is zeroed on top of ATen's
    for mode, p in (("sum", None), ("mean", None), ("max", None), ("sum", psw)):
        want = embedding_bag_ref(w, ids[:m], offsets, mode, None, None if p is None else p[:m], gout, last)
        got = ragged_bag(w, ids, offsets, mode, None, False, p, gout, last)
        assert _close(got[0], want[0]) and _close(got[1], want[1]), mode
        assert p is None or _close(got[2][:m], want[2])


def test_restatement_max_gives_the_gradient_to_the_first_of_equal_rows():
    w = torch.tensor([[0.0, 0.0], [1.0, 5.0], [1.0, 5.0], [3.0, 2.0], [3.0, 5.0]], dtype=torch.float64)
    ids = torch.tensor([1, 2, 3, 4, 2, 1, 0, 0])
    offsets = torch.tensor([0, 4, 6])
    gout = torch.tensor([[1.0, 10.0], [100.0, 1000.0], [7.0, 7.0]], dtype=torch.float64)
    want = embedding_bag_ref(w, ids, offsets, "max", PAD, None, gout)
    got = ragged_bag(w, ids, offsets, "max", PAD, True, None, gout)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # bag 0: column 0 -> row 3 (the first 3.0), column 1 -> row 1 (the first 5.0); bag 1: row 2 comes first
    assert got[1].tolist() == [[0, 0], [0, 10], [100, 1000], [1, 0], [0, 0]]


def test_restatement_agrees_with_the_padded_restatement():
    """the same bags padded to the longest one, through the restatement of the padded op"""
    from bag_masked_ref import masked_bag
    ids, offsets, w, gout, psw = _batch(3)
    idx, wts = pad_bags(ids, offsets, PAD, True, psw)
    for mode, p, pw in (("sum", None, None), ("mean", None, None), ("max", None, None), ("sum", psw, wts)):
        a = ragged_bag(w, ids, offsets, mode, PAD, True, p, gout, True)
        b = masked_bag(w, idx, mode, pad=PAD, exclude=True, psw=pw, gout=gout)
        assert _close(a[0], b[0]) and _close(a[1], b[1]), mode


def test_restatement_extras_out_of_range_id_and_bad_offsets():
    w = torch.arange(1, 11, dtype=torch.float64).reshape(5, 2)
    ids = torch.tensor([1, 9, 2, 3, 4, 1])
    out, grad, _ = ragged_bag(w, ids, torch.tensor([0, 3]), "mean", PAD, True, None, torch.ones(2, 2, dtype=torch.float64))
    assert torch.equal(out[0], (w[1] + w[2]) / 3)                  # the id outside the table: a zero row that counts
    assert torch.equal(grad[1], torch.tensor([1 / 3 + 1 / 3] * 2, dtype=torch.float64))
    assert bag_bounds(torch.tensor([0, 3, 2, 9]), 6) == [(0, 3), (3, 3), (2, 6), (6, 6)]
    assert bag_bounds(torch.tensor([-2, 4]), 6, True) == [(0, 4)]


@pytest.mark.parametrize("last", [True, False])
def test_owner_map_is_bucketize_arithmetic(last):
    ids, offsets, _, _, _ = _batch(4)
    n = ids.numel()
    off = offsets if last else offsets[:-1]
    got = bag_owner(off, n, last)
    want = torch.full((n,), -1, dtype=torch.int64)
    for b, (beg, end) in enumerate(bag_bounds(off, n, last)):
        want[beg:end] = b
    assert torch.equal(got, want)
    if last:
        assert bool((got[int(offsets[-1]):] == -1).all())           # behind the last bag: no owner
    # repeated offsets (empty bags) resolve to the one non-empty bag
    assert bag_owner(torch.tensor([0, 0, 0, 2, 2, 5]), 6).tolist() == [2, 2, 4, 4, 4, 5]
    assert bag_owner(torch.tensor([2, 2, 4]), 6, True).tolist() == [-1, -1, 1, 1, -1, -1]


def test_exact_batch_builders():
    g = torch.Generator().manual_seed(5)
    ids, offsets = bags_from_lengths(g, boundary_lengths(g, 16), V, PAD, trailing=5, sprinkle=0.2, all_pad=(5,))
    cut = pow2_live(ids, offsets, PAD)
    ids2, off2 = pow2_lengths(ids, offsets)
    for b in range(offsets.numel() - 1):
        c = int((cut[int(offsets[b]):int(offsets[b + 1])] != PAD).sum())
        ln = int(off2[b + 1] - off2[b])
        assert c & (c - 1) == 0 and ln & (ln - 1) == 0
    assert ids2.numel() == int(off2[-1]) + 5


# ------------------------------------------------------------------------------------------------ the C entries
@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_long_len_and_workspace_queries(lib):
    T = lib.trs_bag_ragged_long_len()
    assert T >= 1
    from torecsys_amd import functional as F_
    assert F_.bag_ragged_long_len() == T
    assert lib.trs_bag_ragged_workspace_bytes(100) >= 4 * 101       # a counter + at most B entries
    assert lib.trs_bag_ragged_workspace_bytes(0) >= 4
    assert lib.trs_scatter_ragged_workspace_bytes(1000, 16) >= 8


def test_argument_errors_without_gpu(lib):
    from torecsys_amd import _abi
    EINVAL, EDTYPE, EWORKSPACE = -1, -2, -6
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    big = 1 << 20

    def fwd(table=p, dtype=0, ids=p, ids_dtype=0, n=10, offsets=p, off_dtype=0, n_off=4, B=4, mode=0, excl=-1,
            weights=null, out=p, argmax=null, inv_cnt=null, ws=p, ws_bytes=big):
        return lib.trs_bag_pool_ragged_fwd(table, 20, 8, dtype, ids, ids_dtype, n, offsets, off_dtype, n_off, B, mode,
                                           excl, weights, out, argmax, inv_cnt, ws, ws_bytes, null, null)

    bad = [(dict(table=null), EINVAL, "NULL"), (dict(offsets=null), EINVAL, "NULL"), (dict(out=null), EINVAL, "NULL"),
           (dict(ids=null), EINVAL, "NULL"), (dict(ws=null), EINVAL, "NULL"), (dict(mode=3), EINVAL, "mode"),
           (dict(n_off=6), EINVAL, "offsets"), (dict(excl=20), EINVAL, "exclude_row"),
           (dict(mode=1, weights=p, inv_cnt=p), EINVAL, "weights"), (dict(mode=2), EINVAL, "argmax"),
           (dict(mode=1), EINVAL, "inv_cnt"), (dict(dtype=7), EDTYPE, "dtype"), (dict(ids_dtype=5), EDTYPE, "ids dtype"),
           (dict(off_dtype=5), EDTYPE, "offsets dtype"), (dict(ws_bytes=4), EWORKSPACE, "workspace")]
    for kw, code, word in bad:
        assert fwd(**kw) == code, kw
        msg = _abi.last_error()
        assert msg.startswith("bag_pool_ragged_fwd:") and word in msg, (kw, msg)
    assert fwd(B=0, n_off=0, table=null, offsets=null, out=null, ws=null) == 0      # an empty batch touches nothing

    assert lib.trs_bag_owner(null, 0, 4, 4, 10, p, null) == EINVAL and _abi.last_error().startswith("bag_owner:")
    assert lib.trs_bag_owner(p, 0, 7, 4, 10, p, null) == EINVAL and _abi.last_error().startswith("bag_owner:")
    assert lib.trs_bag_owner(p, 3, 4, 4, 10, p, null) == EDTYPE and "dtype" in _abi.last_error()
    assert lib.trs_bag_owner(null, 0, 4, 4, 0, null, null) == 0

    def walk(g=p, bag_of=p, weights=null, argmax=null, dtype=0, ws_bytes=big):
        return lib.trs_scatter_rows_ragged(g, bag_of, weights, argmax, p, p, 10, 4, 20, 8, dtype, -1, p, p, ws_bytes, null)

    for kw, code in ((dict(g=null), EINVAL), (dict(bag_of=null), EINVAL), (dict(weights=p, argmax=p), EINVAL),
                     (dict(dtype=9), EDTYPE), (dict(ws_bytes=4), EWORKSPACE)):
        assert walk(**kw) == code, kw
        assert _abi.last_error().startswith("scatter_rows_ragged:"), (kw, _abi.last_error())

    def wgrad(g=p, bag_of=p, dtype=0, ids_dtype=0, excl=-1, n=10):
        return lib.trs_bag_weight_grad_ragged(g, p, 20, 8, dtype, p, ids_dtype, n, bag_of, excl, p, null)

    for kw, code in ((dict(g=null), EINVAL), (dict(bag_of=null), EINVAL), (dict(excl=-2), EINVAL), (dict(dtype=9), EDTYPE),
                     (dict(ids_dtype=9), EDTYPE)):
        assert wgrad(**kw) == code, kw
        assert _abi.last_error().startswith("bag_weight_grad_ragged:"), (kw, _abi.last_error())
    assert wgrad(n=0) == 0


def test_python_validation_without_gpu():
    from torecsys_amd import functional as F_
    from torecsys_amd.inputs import RaggedListIndicesEmbedding
    w = torch.zeros(10, 4)
    ids, off = torch.tensor([1, 2, 3]), torch.tensor([0, 2])
    with pytest.raises(ValueError, match="mode"):
        F_.bag_pool_ragged(w, ids, off, "median")
    with pytest.raises(ValueError, match="only supported for mode='sum'"):
        F_.bag_pool_ragged(w, ids, off, "mean", per_sample_weights=torch.ones(3))
    with pytest.raises(ValueError, match="dtype"):
        F_.bag_pool_ragged(w, ids, off, "sum", per_sample_weights=torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\(n,\)"):
        F_.bag_pool_ragged(w, ids, off, "sum", per_sample_weights=torch.ones(4))
    with pytest.raises(ValueError, match="needs a padding_idx"):
        F_.bag_pool_ragged(w, ids, off, "sum", exclude_padding=True)
    with pytest.raises(ValueError, match="inside the table"):
        F_.bag_pool_ragged(w, ids, off, "sum", 10, exclude_padding=True)
    with pytest.raises(ValueError, match=r"\(n,\) or \(n, 1\)"):
        F_.bag_pool_ragged(w, ids.reshape(1, 3), off)
    with pytest.raises(NotImplementedError, match="dividing"):
        F_.bag_pool_ragged(w, ids, off, "sum", opt=object())
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.bag_pool_ragged(w, ids, off, "sum")
    m = RaggedListIndicesEmbedding(embed_size=4, field_size=10)
    assert list(m.state_dict().keys()) == ["embedding.weight"] and m.padding_idx == 0 and len(m) == 4
    with pytest.raises(ValueError):
        RaggedListIndicesEmbedding(embed_size=4, field_size=10, output_method="none")
    with pytest.raises(TypeError):
        m.set_schema("tags")
    m.set_schema("tags", offsets="tag_offsets")
    assert m.schema.inputs == ["tags"] and m.schema.offsets == "tag_offsets" and m.schema.weights is None
    with pytest.raises(NotImplementedError):
        m.set_fused_optimizer(object())
    import torecsys_amd
    assert torecsys_amd.RaggedListIndicesEmbedding is RaggedListIndicesEmbedding

"""Attention pooling of ragged bags, host side (no GPU): the fp64 restatement tests/attn_ragged_ref.py pinned to a per-bag
nn.MultiheadAttention loop and to pad + key_padding_mask + masked pooling on the CPU, the module's constructor / forward
errors and state_dict keys, and the argument checks of the four new C entries (error codes and messages that name the
entry, before any launch)."""
import ctypes

import pytest
import torch

from attn_ragged_ref import mha_loop, pad_to, parity_lengths, ragged_attn_with
from bag_ragged_ref import bags_from_lengths
from list_attn_ref import ATTN_KEYS, make_attention

V, PAD = 41, 0
KEYS = ["embedding.weight"] + ATTN_KEYS


def _batch(seed, E, sprinkle):
    g = torch.Generator().manual_seed(seed)
    lengths = [0, 1, 2, 7, 3, 0, 9, 4, 5, 0]                                  # empty first, middle and last bags
    ids, offsets = bags_from_lengths(g, lengths, V, PAD, trailing=3, sprinkle=sprinkle, all_pad=(4, 7))
    w = torch.randn(V, E, generator=g, dtype=torch.float64)
    gout = torch.randn(len(lengths), 1, E, generator=g, dtype=torch.float64)
    return ids, offsets, w, gout


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("E,H", [(8, 1), (12, 3)])
def test_restatement_equals_a_per_bag_multihead_attention_loop(E, H, mode, exclude, bias):
    ids, offsets, w, gout = _batch(E + H, E, 0.25)
    attn = make_attention(E, H, bias, generator=torch.Generator().manual_seed(3)).double()
    for last, ids_, off_ in ((True, ids, offsets), (False, ids[:int(offsets[-1])], offsets[:-1])):
        for max_length in (64, 4):                                            # 4: the bags of 7, 9 and 5 are cut
            kw = dict(pad=PAD, exclude=exclude, include_last_offset=last, gout=gout)
            got = ragged_attn_with(w, ids_, off_, attn, mode, max_length, **kw)
            want_y, want = mha_loop(w, ids_, off_, attn, mode, max_length, **kw)
            assert _close(got["y"], want_y)
            for k in KEYS:
                if want.get(k) is None:
                    assert got[k] is None and not bias
                    continue
                assert _close(got[k], want[k]), (k, max_length, last)
            assert float(got["embedding.weight"][PAD].abs().max()) == 0.0
            assert float(got["y"][0].abs().max()) == 0.0 and got["cnt"][0] == 0      # an empty bag: an exact zero row
            assert any(got["over"]) == (max_length == 4)
            if exclude:
                assert float(got["y"][4].abs().max()) == 0.0 and got["cnt"][4] == 0  # nothing but padding
                assert float(got["dx"][ids_ == PAD].abs().max()) == 0.0
            if last:
                assert float(got["dx"][int(offsets[-1]):].abs().max()) == 0.0        # ids that no bag holds
            # dx is the per-position gradient: summed per row (padding row aside) it is the table gradient
            tab = torch.zeros_like(w).index_add_(0, ids_.long(), got["dx"])
            tab[PAD] = 0
            assert _close(tab, got["embedding.weight"])


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_restatement_equals_padding_with_a_key_padding_mask(mode):
    """the ATen composition the GPU tests measure bf16 against: pad, nn.MultiheadAttention(key_padding_mask), masked pool"""
    E, H = 8, 2
    ids, offsets, w, gout = _batch(9, E, 0.0)
    attn = make_attention(E, H, True, generator=torch.Generator().manual_seed(5)).double()
    got = ragged_attn_with(w, ids, offsets, attn, mode, 64, pad=PAD, include_last_offset=True, gout=gout)
    idx, mask = pad_to(ids, offsets, 9, PAD, True)
    wl = w.clone().requires_grad_()
    seq = torch.nn.functional.embedding(idx, wl).transpose(0, 1)
    live = ~mask.all(dim=1)                                                   # a fully masked sample would give NaN
    o, _ = attn(seq[:, live], seq[:, live], seq[:, live], key_padding_mask=mask[live])
    o = o.transpose(0, 1) * (~mask[live]).unsqueeze(-1)
    o = o.sum(dim=1) / ((~mask[live]).sum(dim=1, keepdim=True) if mode == "mean" else 1)
    y = torch.zeros(idx.shape[0], 1, E, dtype=torch.float64).index_add(0, live.nonzero().flatten(), o.unsqueeze(1))
    assert _close(got["y"], y.detach())
    (y * gout).sum().backward()
    wl.grad[PAD] = 0
    assert _close(got["embedding.weight"], wl.grad)
    assert _close(got["attention.in_proj_weight"], attn.in_proj_weight.grad)


def test_parity_lengths_cover_the_boundaries():
    lens = parity_lengths(torch.Generator().manual_seed(1))
    assert len(lens) == 97 and max(lens) == 64 and lens[:11] == [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64]
    assert all(a >= 32 and b <= 5 for a, b in zip(lens[11::2], lens[12::2]))


# ------------------------------------------------------------------------------------------------ the module
def test_module_constructor_forward_errors_and_state_dict_keys():
    from torecsys_amd.inputs import ListIndicesEmbedding, RaggedListIndicesEmbedding
    plain = RaggedListIndicesEmbedding(embed_size=8, field_size=10)
    assert list(plain.state_dict().keys()) == ["embedding.weight"] and plain.use_attn is False
    m = RaggedListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, max_length=20, num_heads=2)
    padded = ListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, num_heads=2)
    assert list(m.state_dict().keys()) == list(padded.state_dict().keys())
    m.load_state_dict(padded.state_dict())
    padded.load_state_dict(m.state_dict())
    assert isinstance(m.attention, torch.nn.MultiheadAttention) and m.attention.num_heads == 2 and m.max_length == 20
    nb = RaggedListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, max_length=1, bias=False)
    assert nb.attention.in_proj_bias is None
    for bad in (dict(), dict(max_length=0), dict(max_length=65)):
        with pytest.raises(ValueError, match="max_length"):
            RaggedListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, **bad)
    with pytest.raises(ValueError, match="max_pooling"):
        RaggedListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, max_length=8, output_method="max_pooling")
    with pytest.raises(NotImplementedError):
        m.set_fused_optimizer(object())
    ids, off = torch.tensor([1, 2, 3]), torch.tensor([0, 2])
    with pytest.raises(ValueError, match="per_sample_weights"):
        m(ids, off, per_sample_weights=torch.ones(3))
    drop = RaggedListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, max_length=8, dropout=0.5)
    with pytest.raises(NotImplementedError, match="dropout"):
        drop(ids, off)
    wide = RaggedListIndicesEmbedding(embed_size=256, field_size=10, use_attn=True, max_length=8)
    with pytest.raises(NotImplementedError, match="E=256"):
        wide(ids, off)
    with pytest.raises(NotImplementedError, match="float64"):
        RaggedListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, max_length=8).double()(ids, off)
    mixed = RaggedListIndicesEmbedding(embed_size=8, field_size=10, use_attn=True, max_length=8)
    mixed.attention.bfloat16()
    with pytest.raises(NotImplementedError, match="dtype"):
        mixed(ids, off)
    with pytest.raises(RuntimeError, match="no CPU path"):                    # no composition fallback behind the kernel
        m(ids, off)


def test_functional_validation_without_gpu():
    from torecsys_amd import functional as F_
    w, wqk = torch.zeros(10, 4), torch.zeros(8, 4)
    ids, off = torch.tensor([1, 2, 3]), torch.tensor([0, 2])
    with pytest.raises(ValueError, match="mode"):
        F_.attn_pool_ragged(w, ids, off, wqk, None, 1, "max", max_length=4)
    with pytest.raises(ValueError, match="max_length"):
        F_.attn_pool_ragged(w, ids, off, wqk, None, 1, "sum", max_length=65)
    with pytest.raises(TypeError):
        F_.attn_pool_ragged(w, ids, off, wqk, None, 1, "sum")                 # max_length is required
    with pytest.raises(ValueError, match="w_qk"):
        F_.attn_pool_ragged(w, ids, off, wqk[:4], None, 1, "sum", max_length=4)
    with pytest.raises(ValueError, match="needs a padding_idx"):
        F_.attn_pool_ragged(w, ids, off, wqk, None, 1, "sum", max_length=4, exclude_padding=True)
    with pytest.raises(NotImplementedError, match="H=3"):
        F_.attn_pool_ragged(w, ids, off, wqk, None, 3, "sum", max_length=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.attn_pool_ragged(w, ids, off, wqk, None, 1, "sum", max_length=4)


# ------------------------------------------------------------------------------------------------ the C entries
@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_workspace_query_is_a_pure_function(lib):
    assert lib.trs_attn_pool_ragged_bwd_workspace_bytes(7, 50, 64, 4) == 0            # pbar fits in LDS
    assert lib.trs_attn_pool_ragged_bwd_workspace_bytes(7, 64, 128, 128) == 4 * 7 * 128 * 64
    assert lib.trs_attn_pool_ragged_bwd_workspace_bytes(0, 64, 128, 128) == 0
    assert lib.trs_attn_pool_ragged_blocks(0, 50, 64, 4, 0, 0) == 0
    assert lib.trs_attn_pool_ragged_blocks(5, 50, 64, 3, 0, 0) == 0                   # E % H != 0: no path


def test_argument_errors_without_gpu(lib):
    from torecsys_amd import _abi
    EINVAL, EDTYPE, ESHAPE, EWORKSPACE = -1, -2, -3, -6
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    V_, big = 20, 2 ** 31 - 1

    def fwd(table=p, E=8, dtype=0, ids=p, ids_dtype=0, n=10, offsets=p, off_dtype=0, n_off=4, B=4, max_len=16, excl=-1,
            w_qk=p, H=2, mode=0, out=p, cnt=p):
        return lib.trs_attn_pool_ragged_fwd(table, V_, E, dtype, ids, ids_dtype, n, offsets, off_dtype, n_off, B, max_len,
                                            excl, w_qk, null, H, mode, out, cnt, null, null)

    def bwd(table=p, E=8, dtype=0, ids=p, ids_dtype=0, n=10, offsets=p, off_dtype=0, n_off=4, B=4, max_len=16, excl=-1,
            w_qk=p, H=2, mode=0, gout=p, dx=p, dw=p, db=p, blocks=2, ws=null, ws_bytes=0):
        return lib.trs_attn_pool_ragged_bwd(table, V_, E, dtype, ids, ids_dtype, n, offsets, off_dtype, n_off, B, max_len,
                                            excl, w_qk, null, H, mode, gout, dx, dw, db, blocks, ws, ws_bytes, null, null)

    shared = [(dict(table=null), EINVAL, "NULL"), (dict(offsets=null), EINVAL, "NULL"), (dict(w_qk=null), EINVAL, "NULL"),
              (dict(ids=null), EINVAL, "NULL"), (dict(n_off=6), EINVAL, "offsets"), (dict(n_off=3), EINVAL, "offsets"),
              (dict(excl=V_), EINVAL, "exclude_row"), (dict(excl=-2), EINVAL, "exclude_row"),
              (dict(max_len=0), EINVAL, "max_len"), (dict(max_len=65), EINVAL, "max_len"),
              (dict(n=big), ESHAPE, "int32"), (dict(B=big, n_off=big), ESHAPE, "int32"),
              (dict(dtype=7), EDTYPE, "dtype"), (dict(ids_dtype=5), EDTYPE, "ids dtype"),
              (dict(off_dtype=5), EDTYPE, "offsets dtype"), (dict(E=129, H=1), EDTYPE, "unsupported shape"),
              (dict(H=3), EDTYPE, "unsupported shape")]
    for name, fn, more in (("attn_pool_ragged_fwd:", fwd, [(dict(out=null), EINVAL, "NULL"), (dict(cnt=null), EINVAL, "NULL")]),
                           ("attn_pool_ragged_bwd:", bwd,
                            [(dict(gout=null), EINVAL, "NULL"), (dict(dx=null), EINVAL, "NULL"),
                             (dict(dw=null), EINVAL, "NULL"), (dict(db=null), EINVAL, "NULL"),
                             (dict(blocks=0), EINVAL, "blocks"), (dict(blocks=5), EINVAL, "blocks"),
                             (dict(E=128, H=128, max_len=64), EWORKSPACE, "workspace"),
                             (dict(E=128, H=128, max_len=64, ws=p, ws_bytes=4 * 2 * 128 * 64 - 1), EWORKSPACE, "workspace")])):
        for kw, code, word in shared + more:
            assert fn(**kw) == code, (name, kw)
            msg = _abi.last_error()
            assert msg.startswith(name) and word in msg, (kw, msg)
        # an empty batch touches nothing
        assert fn(B=0, n_off=0, table=null, offsets=null, w_qk=null, ids=null) == 0

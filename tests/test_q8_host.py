"""Q8 tables without a GPU: the numpy reference of the format, the size query, argument errors of the new entries before
any launch, and the refusals of the modules."""
import ctypes

import numpy as np
import pytest
import torch

import q8_ref

EINVAL, EDTYPE, EWORKSPACE = -1, -2, -6


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


@pytest.mark.parametrize("E", [8, 20, 64])
def test_pack_dequant_round_trip(E):
    rng = np.random.default_rng(E)
    V = 33
    codes = rng.integers(0, 256, (V, E))
    scale, bias = rng.uniform(1e-3, 2e-2, V).astype(np.float32), rng.normal(size=V).astype(np.float32)
    q = q8_ref.pack(codes, scale, bias)
    assert q.shape == (V, q8_ref.stride(E)) and q.dtype == np.uint8 and not q[:, E + 8:].any()
    s, b = q8_ref.tails(q, E)
    assert np.array_equal(s[:, 0], scale) and np.array_equal(b[:, 0], bias) and np.array_equal(q[:, :E], codes)
    assert np.array_equal(q8_ref.dequant(q, E), (codes.astype(np.float32) * scale[:, None]).astype(np.float32) + bias[:, None])


@pytest.mark.parametrize("E", [16, 20, 64])
def test_quantize_meets_the_reconstruction_bound(E):
    rng = np.random.default_rng(100 + E)
    x = (rng.normal(size=(257, E)) * rng.uniform(1e-3, 30, (257, 1))).astype(np.float32)
    x[3] = 1.25                                  # a constant row dequantizes to itself
    q = q8_ref.quantize(x)
    xq = q8_ref.dequant(q, E)
    assert np.array_equal(xq[3], x[3]) and not q[3, :E].any()
    err = np.abs(xq.astype(np.float64) - x.astype(np.float64))
    assert (err <= q8_ref.recon_bound(x, q8_ref.tails(q, E)[0])).all()


def test_row_bytes(lib):
    assert [lib.trs_q8_row_bytes(E) for E in (8, 20, 64, 128, 0)] == [16, 32, 80, 144, 0]


def test_argument_errors_before_any_launch(lib):
    from torecsys_amd import _abi
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def bag(qrows=p, mode=1, out_dtype=0, off_dtype=0, ws=p, ws_bytes=1 << 20):
        return lib.trs_bag_pool_ragged_q8_fwd(qrows, 10, 16, p, 0, 4, p, off_dtype, 3, 2, mode, -1, p, out_dtype, null, ws,
                                              ws_bytes, null, null)

    g, fm = lib.trs_gather_rows_q8, lib.trs_embed_fm_q8
    cases = [(lib.trs_q8_quantize_rows(null, 10, 16, 0, p, null), EINVAL), (lib.trs_q8_quantize_rows(p, 10, 16, 7, p, null), EDTYPE),
             (g(null, 10, 16, p, 0, null, 2, 2, p, 0, null, null), EINVAL), (g(p, 10, 16, p, 0, null, 2, 2, p, 7, null, null), EDTYPE),
             (g(p, 10, 16, p, 5, null, 2, 2, p, 0, null, null), EDTYPE),
             (fm(p, 10, 16, null, 0, null, 2, 2, p, p, null, null, null, 0, null, null), EINVAL),
             (fm(p, 10, 16, p, 0, null, 2, 2, p, p, null, p, null, 0, null, null), EINVAL),      # first_table without first
             (fm(p, 10, 16, p, 0, null, 2, 2, p, p, null, null, null, 2, null, null), EDTYPE),
             (bag(qrows=null), EINVAL), (bag(ws=null), EINVAL), (bag(mode=2), EINVAL), (bag(mode=-1), EINVAL),
             (bag(out_dtype=3), EDTYPE), (bag(off_dtype=9), EDTYPE),
             (bag(ws_bytes=lib.trs_bag_pool_ragged_q8_workspace_bytes(2) - 1), EWORKSPACE)]
    assert [rc for rc, _ in cases] == [want for _, want in cases]
    assert bag(mode=2) == EINVAL and _abi.last_error().startswith("bag_pool_ragged_q8_fwd: mode 2")
    assert lib.trs_gather_rows_q8(null, 10, 16, null, 0, null, 0, 2, null, 0, null, null) == 0      # B == 0: nothing to do


def test_module_refusals():
    from torecsys_amd import functional as F_, inputs, quant
    sizes = [3, 4]
    mods = [quant.QuantizedMultiIndicesEmbedding(16, sizes), quant.QuantizedEmbeddingFM(16, sizes),
            quant.QuantizedRaggedListIndicesEmbedding(16, 7, output_method='sum')]
    for m in mods:
        assert m.state_dict()['qweight'].dtype == torch.uint8 and m.qweight.shape == (7, 32)
        assert m.set_fused_optimizer(None) is m
        with pytest.raises(NotImplementedError):
            m.set_fused_optimizer(object())
    assert sorted(mods[0].state_dict()) == ['qweight'] and sorted(mods[1].state_dict()) == ['first', 'qweight']
    Ragged = quant.QuantizedRaggedListIndicesEmbedding
    with pytest.raises(NotImplementedError):
        Ragged(16, 7, output_method='max_pooling')
    for kw in (dict(output_method='max_pooling'), dict(output_method='sum', use_attn=True, max_length=8)):
        with pytest.raises(NotImplementedError):
            Ragged.from_float(inputs.RaggedListIndicesEmbedding(16, 7, **kw))
    with pytest.raises(TypeError):
        quant.QuantizedMultiIndicesEmbedding(16, sizes, out_dtype=torch.float16)
    for cls in (quant.QuantizedMultiIndicesEmbedding, quant.QuantizedEmbeddingFM, quant.QuantizedRaggedListIndicesEmbedding):
        with pytest.raises(TypeError):
            cls.from_float(torch.nn.Embedding(7, 16))
    q = torch.zeros(7, 32, dtype=torch.uint8)
    for bad, exc in ((q.float(), TypeError), (q[:, :16], ValueError)):
        with pytest.raises(exc):
            F_.gather_rows_q8(bad, 16, torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        F_.gather_rows_q8(q, 16, torch.zeros(2, 2, dtype=torch.int64))

"""Row-wise int8 (Q8) tables on the device (csrc/q8.hip) against the numpy float32 reference of the format (q8_ref.py):
the quantizer byte for byte, the lookup bit for bit, lookup + FM and ragged bags on exact operands (scale 1 or 0.5,
integer bias in [-128, 0], at most 5 fields / 257 ids: every fp32 sum is exact, so the result equals the float64 reference
rounded once), and the modules.  E = 16 .. 128 take the lane-group path, E = 8 and 20 the element path."""
import io

import numpy as np
import pytest
import torch

import q8_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
V = 67
SIZES = {1: [67], 5: [13, 14, 13, 14, 13]}


def _bits(t):
    return t.detach().rename(None).cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(got, want64, dtype):
    """bit-equal to the float64 reference rounded to dtype (through float32, as the kernels hold every value)"""
    want = torch.from_numpy(np.asarray(want64, np.float64).astype(np.float32)).to(dtype)
    assert got.dtype == dtype and torch.equal(_bits(got), _bits(want.reshape(got.shape)))


def _table(E, exact, seed=0):
    rng = np.random.default_rng(1000 * E + seed)
    codes = rng.integers(0, 256, (V, E))
    if exact:
        scale, bias = rng.choice([1.0, 0.5], V), rng.integers(-128, 1, V)
    else:
        scale, bias = rng.uniform(1e-3, 2e-2, V), rng.normal(size=V)
    q = q8_ref.pack(codes, scale.astype(np.float32), bias.astype(np.float32))
    return torch.from_numpy(q).to(DEV), q8_ref.dequant(q, E)


def _indices(rng, B, N, with_offsets, idt):
    """((B, N) ids on the device, offsets or None, the table rows they name)"""
    if with_offsets:
        sizes = np.array(SIZES[N])
        off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        idx = rng.integers(0, sizes, (B, N))
        return torch.from_numpy(idx).to(DEV, idt), torch.from_numpy(off).to(DEV), idx + off
    idx = rng.integers(0, V, (B, N))
    return torch.from_numpy(idx).to(DEV, idt), None, idx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [16, 64, 128, 20])
def test_quantizer_bytes(E, dtype):
    from torecsys_amd import quant
    x = torch.randn(V, E, generator=torch.Generator().manual_seed(E)) * torch.logspace(-2, 1, V).view(V, 1)
    x[5] = -0.75                                                       # a constant row
    x[6] = torch.tensor([0.0, -0.0]).repeat(E // 2)                    # +-0 only
    x[7, ::2] = torch.tensor([0.0, -0.0]).repeat(E // 4)               # +-0 among other values
    x = x.to(dtype)
    got = quant.quantize_rows(x.to(DEV)).cpu().numpy()
    want = q8_ref.quantize(x.float().numpy())
    assert np.array_equal(got[:, E:], want[:, E:])                     # scale, bias, padding
    diff = got[:, :E].astype(int) - want[:, :E].astype(int)
    for r in np.unique(np.nonzero(diff)[0]):                           # a half-way case reads x.5 here, a bug does not
        s, b = q8_ref.tails(want[r:r + 1], E)
        print(f"row {r}: codes differ at (x - bias) / scale =", ((x[r].float().numpy() - b[0]) / s[0])[diff[r] != 0])
    assert np.abs(diff).max() <= 1 and not diff.any()
    deq = quant.dequantize_rows(torch.from_numpy(got).to(DEV), E, torch.float32)
    assert torch.equal(_bits(deq), _bits(torch.from_numpy(q8_ref.dequant(got, E))))


@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [16, 32, 64, 128, 8, 20])
def test_gather(E, dtype, idt):
    from torecsys_amd import functional as F_
    q, x = _table(E, exact=False)
    rng = np.random.default_rng(E)
    F_.index_errors_seen()
    for B in (1, 67):
        for N in (1, 5):
            for with_offsets in (False, True):
                idx, off, rows = _indices(rng, B, N, with_offsets, idt)
                _same(F_.gather_rows_q8(q, E, idx, off, dtype), x[rows], dtype)
    assert not F_.index_errors_seen()
    idx, _, rows = _indices(rng, 67, 5, False, idt)
    idx[0, 0], idx[66, 4] = -1, V
    want = x[rows]
    want[0, 0], want[66, 4] = 0, 0
    _same(F_.gather_rows_q8(q, E, idx, None, dtype), want, dtype)
    assert F_.index_errors_seen()


def _fm_ref(x, rows, first=None):
    xs = x[rows].astype(np.float64)                                    # (B, N, E)
    fm = 0.5 * (xs.sum(1) ** 2 - (xs ** 2).sum(1))
    return xs, fm, None if first is None else first[rows].astype(np.float64).sum(1, keepdims=True)


@pytest.mark.parametrize("want_emb,with_first", [(True, True), (False, False)])
@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [16, 32, 64, 128, 8, 20])
def test_embed_fm_exact(E, dtype, idt, want_emb, with_first):
    from torecsys_amd import functional as F_
    q, x = _table(E, exact=True)
    rng = np.random.default_rng(E + 1)
    first = rng.integers(-8, 9, V).astype(np.float32)
    fw = torch.from_numpy(first).to(DEV, dtype).view(V, 1) if with_first else None
    for B in (1, 67):
        for N in (1, 5):
            for with_offsets in (False, True):
                idx, off, rows = _indices(rng, B, N, with_offsets, idt)
                emb, fm, f1 = F_.embed_fm_q8(q, E, idx, off, fw, want_emb, dtype)
                xs, fm_ref, f1_ref = _fm_ref(x, rows, first if with_first else None)
                _same(fm, fm_ref, dtype)
                assert (emb is None) == (not want_emb) and (f1 is None) == (not with_first)
                if want_emb:
                    _same(emb, xs, dtype)
                if with_first:
                    _same(f1, f1_ref, dtype)


@pytest.mark.parametrize("E", [64, 20])
def test_embed_fm_random_scales(E):
    """fp32 out, random scales: against the float64 reference within the error of fp32 sums of N terms, N * 2^-23 * sum
    |terms| (terms: the products x_i x_j / 2 of the square of the sum and of the sum of squares), plus half an ulp."""
    from torecsys_amd import functional as F_
    q, x = _table(E, exact=False, seed=7)
    N, (idx, off, rows) = 5, _indices(np.random.default_rng(3), 67, 5, True, torch.int64)
    _, fm, _ = F_.embed_fm_q8(q, E, idx, off, None, False, torch.float32)
    xs, fm_ref, _ = _fm_ref(x, rows)
    terms = 0.5 * (np.abs(xs).sum(1) ** 2 + (xs ** 2).sum(1))
    tol = N * 2.0 ** -23 * terms + 0.5 * np.spacing(np.abs(fm_ref).astype(np.float32)).astype(np.float64)
    err = np.abs(fm.cpu().numpy().astype(np.float64) - fm_ref)
    assert (err <= tol).all()


@pytest.mark.parametrize("variant", ["plain", "last_offset", "int32_offsets", "exclude_padding"])
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [16, 64, 20])
def test_ragged_bags_exact(E, dtype, mode, variant):
    from torecsys_amd import functional as F_
    T = F_.bag_ragged_long_len()
    lengths = [0, 1, T, T + 1, 0]              # empty, single, the longest first-tier bag, a second-tier bag, empty last
    q, x = _table(E, exact=True)
    rng = np.random.default_rng(E + 2)
    ends = np.cumsum(lengths)
    ids = rng.integers(1, V, ends[-1])
    exclude = variant == "exclude_padding"
    if exclude:
        ids[rng.random(ids.shape) < 0.2] = 0
    last = variant == "last_offset"
    offsets = np.concatenate([[0], ends]) if last else np.concatenate([[0], ends[:-1]])
    want = np.zeros((len(lengths), E))
    for b, (beg, end) in enumerate(zip(np.concatenate([[0], ends[:-1]]), ends)):
        live = ids[beg:end][ids[beg:end] != 0] if exclude else ids[beg:end]
        if len(live):
            want[b] = x[live].astype(np.float64).sum(0) / (len(live) if mode == "mean" else 1)
    F_.index_errors_seen()
    out = F_.bag_pool_ragged_q8(q, E, torch.from_numpy(ids).to(DEV),
                                torch.from_numpy(offsets).to(DEV, torch.int32 if variant == "int32_offsets" else torch.int64),
                                mode, 0, exclude_padding=exclude, include_last_offset=last, out_dtype=dtype)
    assert out.shape == (len(lengths), 1, E)
    _same(out, want, dtype)
    assert not F_.index_errors_seen()
    if variant == "plain":                     # a decreasing pair: that bag is empty and the flag is raised
        bad = torch.tensor([0, 5, 3, 9], device=DEV)
        F_.bag_pool_ragged_q8(q, E, torch.from_numpy(ids).to(DEV), bad, mode, out_dtype=dtype)
        assert F_.index_errors_seen()


def _reload(fresh, module):
    buf = io.BytesIO()
    torch.save(module.state_dict(), buf)
    buf.seek(0)
    fresh.load_state_dict(torch.load(buf))
    assert torch.equal(fresh.qweight.cpu(), module.qweight.cpu())
    return fresh.to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
def test_modules(dtype):
    from torecsys_amd import functional as F_, fused, inputs, quant
    torch.manual_seed(11)
    E, sizes = 64, SIZES[5]
    idx = torch.from_numpy(np.random.default_rng(5).integers(0, 13, (67, 5))).to(DEV)
    fl = inputs.MultiIndicesEmbedding(E, sizes).to(DEV).to(dtype)
    m = quant.QuantizedMultiIndicesEmbedding.from_float(fl)
    out = m(idx)
    assert out.names == ('B', 'N', 'E') and out.dtype == dtype and not out.requires_grad
    assert sorted(m.state_dict()) == ['qweight'] and torch.equal(m.qweight, quant.quantize_rows(fl.embedding.weight))
    assert torch.equal(_bits(out), _bits(F_.gather_rows_q8(m.qweight, E, idx, m.offsets, dtype)))
    assert torch.equal(_bits(_reload(quant.QuantizedMultiIndicesEmbedding(E, sizes, dtype), m)(idx)), _bits(out))
    fm_q = quant.QuantizedEmbeddingFM.from_float(fused.EmbeddingFM(E, sizes).to(DEV).to(dtype))
    outs = fm_q(idx)
    assert outs[0].names == ('B', 'N', 'E') and outs[1].names == ('B', 'O') and outs[2].shape == (67, 1)
    assert sorted(fm_q.state_dict()) == ['first', 'qweight']
    want = F_.embed_fm_q8(fm_q.qweight, E, idx, fm_q.offsets, fm_q.first, True, dtype)
    again = _reload(quant.QuantizedEmbeddingFM(E, sizes, out_dtype=dtype), fm_q)(idx)
    assert all(torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c)) for a, b, c in zip(outs, want, again))
    values = torch.from_numpy(np.random.default_rng(6).integers(0, 40, 300)).to(DEV)
    offsets = torch.tensor([0, 0, 7, 120, 300], device=DEV)
    for method in ("sum", "avg_pooling"):
        kw = dict(output_method=method, exclude_padding=True, include_last_offset=True)
        rg = quant.QuantizedRaggedListIndicesEmbedding.from_float(inputs.RaggedListIndicesEmbedding(E, 40, **kw).to(DEV).to(dtype))
        out = rg(values, offsets)
        assert out.names == ('B', 'N', 'E') and out.shape == (4, 1, E) and sorted(rg.state_dict()) == ['qweight']
        want = F_.bag_pool_ragged_q8(rg.qweight, E, values, offsets, rg._POOL[method], 0, exclude_padding=True,
                                     include_last_offset=True, out_dtype=dtype)
        assert torch.equal(_bits(out), _bits(want))
        fresh = quant.QuantizedRaggedListIndicesEmbedding(E, 40, out_dtype=dtype, **kw)
        assert torch.equal(_bits(_reload(fresh, rg)(values, offsets)), _bits(out))


def test_quantized_fm_against_the_float_module():
    """fm = sum_{i<j} x_i x_j.  With |x^_n - x_n| <= d_n (the reconstruction bound of row n, from the scales in qweight):
    |fm^ - fm| <= sum_{i<j} (|x_i| d_j + d_i |x_j| + d_i d_j), plus the fp32 arithmetic of the two kernels (N * 2^-23 * sum
    |terms| each) and half an ulp of each output."""
    from torecsys_amd import fused, quant
    torch.manual_seed(12)
    E, sizes, N = 64, SIZES[5], 5
    fl = fused.EmbeddingFM(E, sizes).to(DEV)
    q = quant.QuantizedEmbeddingFM.from_float(fl)
    idx_np = np.random.default_rng(8).integers(0, 13, (67, N))
    idx = torch.from_numpy(idx_np).to(DEV)
    with torch.no_grad():
        fm_fl = fl(idx)[1].rename(None).cpu().numpy().astype(np.float64)
    fm_q = q(idx)[1].rename(None).cpu().numpy().astype(np.float64)
    w = fl.emb.embedding.weight.detach().cpu().numpy()
    d = q8_ref.recon_bound(w, q8_ref.tails(q.qweight.cpu().numpy(), E)[0])          # (V, 1)
    rows = idx_np + fl.emb.offsets.cpu().numpy()
    ax, dx = np.abs(w[rows]).astype(np.float64), np.broadcast_to(d[rows], (67, N, E))
    A, D = ax.sum(1), dx.sum(1)
    bound = (A * D - (ax * dx).sum(1)) + 0.5 * (D ** 2 - (dx ** 2).sum(1))
    arith = 2 * N * 2.0 ** -23 * 0.5 * ((A + D) ** 2 + ((ax + dx) ** 2).sum(1))
    ulp = np.spacing(np.abs(fm_fl).astype(np.float32)).astype(np.float64)
    err = np.abs(fm_q - fm_fl)
    print("Q8 fm vs float fm: max err", err.max(), "max err / bound", (err / (bound + arith + ulp)).max())
    assert (err <= bound + arith + ulp).all()

"""functional.topk_scores_q8 / QuantizedEmbeddingPairScorer.topk (csrc/topk.hip, Q8 targets) against the fp64 reference of
tests/topk_ref.py over the rows c * scale + bias of tests/q8_ref.py; B = 70 leaves a ragged anchor tile.  Exact cases: codes
0..4, scale in {0.5, 1, 2}, bias and anchors integers in -2..2, so d * scale + sa * bias is exact in any order and collides
constantly.  Real-valued cases: |score - ref| <= gamma(n) * sum_e |a_e| (c_e scale + |bias|), n = E + 4 (dot: E roundings on
each of d and sa, two products, one sum, one spare) or E + 20 (cosine: the float kernel's E + 16 plus the same 4)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import q8_ref
from topk_ref import gamma, topk_ref

gpu, B = pytest.mark.gpu, 70
DTYPES = [torch.bfloat16, torch.float32]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _F():
    import torecsys_amd.functional as F_
    return F_


@lru_cache(maxsize=None)
def int_case(Vt, E, seed=0):      # anchors (B, E), Q8 rows (Vt, S) uint8, their exact dequantized rows (Vt, E)
    g = torch.Generator().manual_seed(seed * 7919 + Vt * 31 + E)
    a = torch.randint(-2, 3, (B, E), generator=g).float()
    codes = torch.randint(0, 5, (Vt, E), generator=g)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Vt,), generator=g)]
    bias = torch.randint(-2, 3, (Vt,), generator=g).float()
    q = torch.from_numpy(q8_ref.pack(codes.numpy(), scale.numpy(), bias.numpy()))
    return a, q, codes.float() * scale[:, None] + bias[:, None]


int_ref = lru_cache(maxsize=None)(lambda Vt, E, k: topk_ref(*int_case(Vt, E)[::2], k))      # computed once per case


def run(dev, a, q, E, k, dtype, **kw):
    v, i = _F().topk_scores_q8(a.to(dev, dtype), None, q.to(dev), E, k, **kw)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and not v.requires_grad
    return v.cpu(), i.cpu()


def assert_exact(got, ref):
    assert torch.equal(got[0].double(), ref[1]) and torch.equal(got[1], ref[2])


@gpu
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("Vt", [127, 129, 1000, 5003])
@pytest.mark.parametrize("E", ["vec", 32, 56, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_exact_with_ties(dev, dtype, E, Vt, k):
    E = (8 if dtype == torch.bfloat16 else 4) if E == "vec" else E
    a, q, _ = int_case(Vt, E)
    assert_exact(run(dev, a, q, E, min(k, Vt), dtype), int_ref(Vt, E, min(k, Vt)))


@gpu
@pytest.mark.parametrize("order", ["increasing", "decreasing", "random"])
def test_order_of_arrival(dev, order):
    """score(b, j) = m_b * rank(j): code columns 0, 1 carry rank // 64, rank % 64 (scale 1, bias 0) against 64 m_b, m_b"""
    Vt, k, E = 5003, 100, 32
    g = torch.Generator().manual_seed(5)
    rank = {"increasing": torch.arange(Vt), "decreasing": torch.arange(Vt - 1, -1, -1),
            "random": torch.randperm(Vt, generator=g)}[order]
    codes = torch.randint(0, 5, (Vt, E), generator=g)
    codes[:, 0], codes[:, 1] = rank // 64, rank % 64
    q = torch.from_numpy(q8_ref.pack(codes.numpy(), np.ones(Vt), np.zeros(Vt)))
    a = torch.zeros(B, E)
    a[:, 1] = torch.randint(1, 3, (B,), generator=g).float()
    a[:, 0] = 64 * a[:, 1]
    assert_exact(run(dev, a, q, E, k, torch.bfloat16), topk_ref(a, codes.float(), k))


@gpu
@pytest.mark.parametrize("E", [64, 40])
@pytest.mark.parametrize("sim", ["dot", "cosine"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_real_valued(dev, dtype, sim, E):
    Vt, k = 1000, 10
    g = torch.Generator().manual_seed(11)
    a = torch.randn(B, E, generator=g).to(dtype).float()
    qn = q8_ref.quantize(torch.randn(Vt, E, generator=g).numpy())
    scale, bias = (torch.from_numpy(t.astype(np.float64)) for t in q8_ref.tails(qn, E))
    c = torch.from_numpy(qn[:, :E].astype(np.float64))
    x = c * scale + bias      # fp64: the reference rows
    scores, ref_v, _ = topk_ref(a, x, k, sim)
    bound = gamma(E + 4 if sim == "dot" else E + 20) * (a.double().abs() @ (c * scale + bias.abs()).T)
    if sim == "cosine":
        bound = bound / (a.double().norm(dim=1)[:, None] * x.norm(dim=1)[None, :])
    v, i = run(dev, a, torch.from_numpy(qn), E, k, dtype, sim=sim)
    assert int(i.min()) >= 0 and int(i.max()) < Vt and all(len(set(row)) == k for row in i.tolist())
    err = (v.double() - scores.gather(1, i)).abs()
    print(f"max err / bound = {float((err / bound.gather(1, i)).max()):.3f}")
    assert bool((err <= bound.gather(1, i)).all()) and bool((v[:, 1:] <= v[:, :-1]).all()) \
        and bool((v[:, -1].double() >= ref_v[:, -1] - bound.amax(dim=1)).all())


@gpu
def test_addressing_exclusion_and_index_flag(dev):
    """float anchor table through int32 ids + offset, targets inside the Q8 table, top 3 excluded, sample 0 keeps k - 2"""
    F_ = _F()
    E, k, lo, hi, off, Vt = 32, 10, 150, 450, 3, 300
    _, q, x = int_case(900, E, seed=1)
    g = torch.Generator().manual_seed(3)
    table = torch.randint(-2, 3, (200, E), generator=g).float()
    idx = torch.randint(0, 190, (B,), generator=g)
    a = table[idx + off]
    ex = torch.cat([topk_ref(a, x[lo:hi], 3)[2], torch.randint(-1, Vt, (B, Vt - 3), generator=g)], dim=1)
    ex[[0, 5]] = -1
    ex[0, :Vt - (k - 2)] = torch.randperm(Vt, generator=g)[:Vt - (k - 2)]
    w, qd, exd = table.to(dev, torch.bfloat16), q.to(dev), ex.to(dev)
    F_.index_errors_seen()
    got = F_.topk_scores_q8(w, idx.to(dev, torch.int32), qd, E, k, anchor_offset=off, target_lo=lo, target_hi=hi, exclude=exd)
    got = (got[0].cpu(), got[1].cpu())
    assert_exact(got, topk_ref(a, x[lo:hi], k, exclude=ex))
    assert not F_.index_errors_seen()
    assert got[1][0, -2:].tolist() == [-1, -1] and bool(torch.isinf(got[0][0, -2:]).all()) and int(got[1][0, -3]) >= 0
    idx[5] = 200 - off      # one row past the table: a zero row, every score 0, ids 0 .. k-1 by the tie rule
    v, i = F_.topk_scores_q8(w, idx.to(dev), qd, E, k, anchor_offset=off, target_lo=lo, target_hi=hi, exclude=exd)
    assert F_.index_errors_seen() and v[5].tolist() == [0.0] * k and i[5].tolist() == list(range(k))
    assert torch.equal(v[:5].cpu(), got[0][:5]) and torch.equal(i[6:].cpu(), got[1][6:])


@gpu
@pytest.mark.parametrize("shared", [False, True])
def test_module(dev, shared):
    from torecsys_amd.fused import EmbeddingPairScorer
    from torecsys_amd.quant import QuantizedEmbeddingPairScorer
    F_ = _F()
    torch.manual_seed(2)
    sizes = (400, None) if shared else (100, 300)
    m = EmbeddingPairScorer(32, *sizes, similarity="cosine", target_offset=100 if shared else 0).to(dev)
    qm = QuantizedEmbeddingPairScorer.from_float(m)
    assert sorted(qm.state_dict()) == (["qweight"] if shared else ["anchor_qweight", "qweight"])
    idx = torch.randint(0, 100, (B,), device=dev)
    ex = torch.randint(-1, 300, (B, 4), device=dev)
    v, i = qm.topk(idx, 7, exclude=ex)
    anchors = F_.gather_rows_q8(qm.qweight if shared else qm.anchor_qweight, 32, idx.view(-1, 1)).view(B, 32)
    rv, ri = F_.topk_scores_q8(anchors, None, qm.qweight, 32, 7, target_lo=100 if shared else 0, sim="cosine", exclude=ex)
    assert torch.equal(v, rv) and torch.equal(i, ri) and tuple(v.shape) == (B, 7) and int(i.max()) < 300
    again = QuantizedEmbeddingPairScorer(32, *sizes, "cosine", target_offset=100 if shared else 0).to(dev)
    again.load_state_dict(qm.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(again.topk(idx, 7, exclude=ex), (v, i)))
    with pytest.raises(NotImplementedError):
        qm.set_fused_optimizer(object())


@pytest.mark.parametrize("case,exc", [("dtype", TypeError), ("stride", ValueError), ("k0", ValueError), ("k129", ValueError),
                                      ("k>Vt", ValueError), ("width", NotImplementedError)])
def test_argument_errors_before_any_launch(case, exc):      # CPU tensors: every check comes before the device is looked at
    E = 6 if case == "width" else 32
    a, q = torch.zeros(4, E), torch.zeros(200, q8_ref.stride(E), dtype=torch.uint8)
    k = {"k0": 0, "k129": 129, "k>Vt": 101}.get(case, 5)
    if case == "dtype":
        q = q.to(torch.int8)
    if case == "stride":
        q = torch.zeros(200, 64, dtype=torch.uint8)
    with pytest.raises(exc, match="topk_scores_q8"):
        _F().topk_scores_q8(a, None, q, E, k, target_hi=100 if case == "k>Vt" else None)

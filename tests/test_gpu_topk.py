"""functional.topk_scores / EmbeddingPairScorer.topk (csrc/topk.hip) against the fp64 reference of tests/topk_ref.py.

Exact cases: tables drawn from {-2 .. 2} are exact in bf16 and every partial sum is an integer far below 2^24, so the
scores are exact in any order, collide constantly, and the tie rule (smaller id first) decides most slots: values and ids
must EQUAL the reference.  B = 70 leaves a ragged anchor tile; Vt = 127 / 129 / 1 000 / 5 003 are below one 128-row tile,
one past it, and several tiles over 1, 3 and 19 target ranges whose last tile is partial.  (k = 128 with Vt = 127 asks for
more than there is, which the interface refuses; that one combination runs with k = 127.)

Real-valued cases: the kernel multiplies table-dtype operands exactly and accumulates in fp32, so a score is off by at most
gamma_n * sum_e |a_e t_e|, gamma_n = n 2^-24 / (1 - n 2^-24): n = E roundings for the inner product (E - 1 additions, and
one spare); cosine divides that sum by the two norms, and n = E + 16 covers the two norm sums (E roundings each on a sum of
squares, i.e. E / 2 relative on the root, against E for the dot: together below E + 8 in first order after the square
roots) and the reciprocals and scalings (8 more).  Ids may differ from the reference on near-ties, so the assertions are:
every returned value is its id's reference score within the bound, values do not increase, ids are distinct and in range,
and the last value reaches the reference's k-th within the row's largest bound."""
from functools import lru_cache

import pytest
import torch

from topk_ref import gamma, topk_ref

gpu = pytest.mark.gpu
B = 70
DTYPES = [torch.bfloat16, torch.float32]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _F():
    from torecsys_amd import functional as F_
    return F_


@lru_cache(maxsize=None)
def int_tables(Vt, E, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + Vt * 31 + E)
    return (torch.randint(-2, 3, (B, E), generator=g).float(), torch.randint(-2, 3, (Vt, E), generator=g).float())


@lru_cache(maxsize=None)
def int_ref(Vt, E, k):
    return topk_ref(*int_tables(Vt, E), k)


def run(dev, a, t, k, dtype, **kw):
    v, i = _F().topk_scores(a.to(dev, dtype), None, t.to(dev, dtype), k, **kw)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and not v.requires_grad
    return v.cpu(), i.cpu()


def assert_exact(got, ref):
    assert torch.equal(got[0].double(), ref[1]) and torch.equal(got[1], ref[2])


@gpu
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("Vt", [127, 129, 1000, 5003])
@pytest.mark.parametrize("E", [32, 64, "vec"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_exact_with_ties(dev, dtype, E, Vt, k):
    E = (8 if dtype == torch.bfloat16 else 4) if E == "vec" else E
    k = min(k, Vt)
    assert_exact(run(dev, *int_tables(Vt, E), k, dtype), int_ref(Vt, E, k))


@gpu
@pytest.mark.parametrize("order", ["increasing", "decreasing", "random"])
def test_order_of_arrival(dev, order):
    """score(b, j) = m_b * rank(j), m_b in {1, 2}: columns 0 and 1 carry rank // 64 and rank % 64 against 64 m_b and m_b"""
    Vt, k, E = 5003, 100, 32
    g = torch.Generator().manual_seed(5)
    rank = {"increasing": torch.arange(Vt), "decreasing": torch.arange(Vt - 1, -1, -1),
            "random": torch.randperm(Vt, generator=g)}[order]
    t = torch.randint(-2, 3, (Vt, E), generator=g).float()
    t[:, 0], t[:, 1] = rank // 64, rank % 64
    a = torch.zeros(B, E)
    a[:, 1] = torch.randint(1, 3, (B,), generator=g).float()
    a[:, 0] = 64 * a[:, 1]
    assert_exact(run(dev, a, t, k, torch.bfloat16), topk_ref(a, t, k))


@gpu
@pytest.mark.parametrize("E", [64, 40])
@pytest.mark.parametrize("sim", ["dot", "cosine"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_real_valued(dev, dtype, sim, E):
    Vt, k = 1000, 10
    g = torch.Generator().manual_seed(11)
    a = torch.randn(B, E, generator=g).to(dtype).float()
    t = torch.randn(Vt, E, generator=g).to(dtype).float()
    scores, ref_v, _ = topk_ref(a, t, k, sim)
    bound = gamma(E if sim == "dot" else E + 16) * (a.double().abs() @ t.double().abs().T)
    if sim == "cosine":
        bound = bound / (a.double().norm(dim=1)[:, None] * t.double().norm(dim=1)[None, :])
    v, i = run(dev, a, t, k, dtype, sim=sim)
    assert int(i.min()) >= 0 and int(i.max()) < Vt
    assert all(len(set(row)) == k for row in i.tolist())
    err = (v.double() - scores.gather(1, i)).abs()
    print(f"max err / bound = {float((err / bound.gather(1, i)).max()):.3f}")
    assert bool((err <= bound.gather(1, i)).all())
    assert bool((v[:, 1:] <= v[:, :-1]).all())
    assert bool((v[:, -1].double() >= ref_v[:, -1] - bound.amax(dim=1)).all())


@gpu
@pytest.mark.parametrize("X,idt", [(1, torch.int32), (300, torch.int64)])
def test_exclusion(dev, X, idt):
    Vt, E, k = 300, 32, 10
    a, t = int_tables(Vt, E, seed=1)
    g = torch.Generator().manual_seed(X)
    top3 = topk_ref(a, t, 3)[2]
    ex = torch.cat([top3, torch.randint(0, Vt, (B, 40), generator=g), torch.full((B, X), -1)], dim=1)[:, :X].contiguous()
    if X >= Vt - (k - 2):      # sample 0 keeps k - 2 targets: the last two slots are padding
        ex[0] = -1
        ex[0, :Vt - (k - 2)] = torch.randperm(Vt, generator=g)[:Vt - (k - 2)]
    got = run(dev, a, t, k, torch.bfloat16, exclude=ex.to(dev, idt))
    ref = topk_ref(a, t, k, exclude=ex)
    assert_exact(got, ref)
    if X >= Vt - (k - 2):
        assert got[1][0, -2:].tolist() == [-1, -1] and bool(torch.isinf(got[0][0, -2:]).all()) and int(got[1][0, -3]) >= 0


@gpu
def test_addressing_and_index_flag(dev):
    """a shared table: anchors through int32 ids and an offset, targets strictly inside it; one anchor id out of range"""
    F_ = _F()
    E, k, lo, hi, off = 32, 10, 150, 850, 3
    g = torch.Generator().manual_seed(3)
    table = torch.randint(-2, 3, (900, E), generator=g).float()
    idx = torch.randint(0, 140, (B,), generator=g)
    w = table.to(dev, torch.bfloat16)
    F_.index_errors_seen()
    got = F_.topk_scores(w, idx.to(dev, torch.int32), None, k, anchor_offset=off, target_lo=lo, target_hi=hi)
    assert_exact((got[0].cpu(), got[1].cpu()), topk_ref(table[idx + off], table[lo:hi], k))
    assert not F_.index_errors_seen()
    q = table[idx + off].to(dev, torch.bfloat16)      # the same anchors as a (B, E) query matrix
    again = F_.topk_scores(q, None, w, k, target_lo=lo, target_hi=hi)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    idx[5] = 900 - off      # one row past the table: a zero row, every score 0, ids 0 .. k-1 by the tie rule
    v, i = F_.topk_scores(w, idx.to(dev), None, k, anchor_offset=off, target_lo=lo, target_hi=hi)
    assert F_.index_errors_seen()
    assert v[5].tolist() == [0.0] * k and i[5].tolist() == list(range(k))
    assert torch.equal(v[:5], got[0][:5]) and torch.equal(i[6:], got[1][6:])


@gpu
@pytest.mark.parametrize("shared", [False, True])
def test_module_equals_functional(dev, shared):
    from torecsys_amd.fused import EmbeddingPairScorer
    F_ = _F()
    torch.manual_seed(2)
    m = EmbeddingPairScorer(32, 100 if not shared else 400, None if shared else 300, similarity="cosine",
                            target_offset=100 if shared else 0).to(dev)
    idx = torch.randint(0, 100, (B,), device=dev)
    ex = torch.randint(-1, 300, (B, 4), device=dev)
    v, i = m.topk(idx, 7, exclude=ex)
    tw = None if shared else m.target.weight
    rv, ri = F_.topk_scores(m.anchor.weight, idx, tw, 7, target_lo=100 if shared else 0, sim="cosine", exclude=ex)
    assert torch.equal(v, rv) and torch.equal(i, ri) and tuple(v.shape) == (B, 7) and int(i.max()) < 300


@pytest.mark.parametrize("case,exc", [("k0", ValueError), ("k129", ValueError), ("k>Vt", ValueError), ("mixed", TypeError),
                                      ("width", NotImplementedError)])
def test_argument_errors_before_any_launch(case, exc):
    """CPU tensors: every check below comes before the device is looked at"""
    a, t = torch.zeros(4, 32), torch.zeros(200, 32)
    k = {"k0": 0, "k129": 129, "k>Vt": 101}.get(case, 5)
    if case == "mixed":
        t = t.bfloat16()
    if case == "width":
        a, t = torch.zeros(4, 6), torch.zeros(200, 6)
    with pytest.raises(exc, match="topk_scores"):
        _F().topk_scores(a, None, t, k, target_hi=100 if case == "k>Vt" else None)

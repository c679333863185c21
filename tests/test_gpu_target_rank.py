"""functional.target_ranks / EmbeddingPairScorer.rank (csrc/target_rank.hip) against the int64 / fp64 count of
tests/target_rank_ref.py.

Exact cases: tables drawn from {-2 .. 2} are exact in bf16 and fp32 and every partial sum is an integer far below 2^24, so
scores are exact in any order and collide constantly: ranks and label scores must EQUAL the reference.  B = 70 leaves a
ragged anchor tile; Vt = 127 / 129 / 1 000 / 5 003 are below one target tile, past it, and several tiles over 1, 3 and 19
target ranges with a partial last tile.  Real-valued cases use the bound of tests/test_gpu_topk.py: a score is off by at
most gamma(n) |a|.|t| (over the norms for cosine), n = E for the inner product, E + 16 for cosine."""
from functools import lru_cache

import pytest
import torch

from target_rank_ref import target_rank_ref
from topk_ref import gamma

gpu = pytest.mark.gpu
B = 70
DTYPES = [torch.bfloat16, torch.float32]
dtype_sim = [pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"]), pytest.mark.parametrize("sim", ["dot", "cosine"])]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _F():
    from torecsys_amd import functional as F_
    return F_


@lru_cache(maxsize=None)
def int_case(Vt, E, P, seed=0):
    """integer tables as test_gpu_topk.int_tables builds them, labels (B, P) with one padding label per fifth sample"""
    g = torch.Generator().manual_seed(seed * 7919 + Vt * 31 + E)
    a, t = torch.randint(-2, 3, (B, E), generator=g).float(), torch.randint(-2, 3, (Vt, E), generator=g).float()
    y = torch.randint(0, Vt, (B, P), generator=g)
    y[::5, P - 1] = -1
    return a, t, y


@lru_cache(maxsize=None)
def real_case(dtype, E, Vt=1000, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, E, generator=g).to(dtype).float(), torch.randn(Vt, E, generator=g).to(dtype).float()


def run(dev, a, t, y, dtype, exclude=None, **kw):
    ex = None if exclude is None else exclude.to(dev)
    r, s = _F().target_ranks(a.to(dev, dtype), None, t.to(dev, dtype), y.to(dev), exclude=ex, **kw)
    assert r.dtype == torch.int64 and s.dtype == torch.float32 and tuple(r.shape) == tuple(s.shape) == (B, y.shape[1])
    return r.cpu(), s.cpu()


def assert_exact(got, ref):
    assert torch.equal(got[0], ref[1]) and torch.equal(got[1].double(), ref[2])


@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("Vt", [127, 129, 1000, 5003])
@pytest.mark.parametrize("E", [32, 64, "vec"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_exact_with_ties(dev, dtype, E, Vt, P):
    E = (8 if dtype == torch.bfloat16 else 4) if E == "vec" else E      # one 16-byte vector: not a whole 64-byte k-step
    a, t, y = int_case(Vt, E, P)
    got = run(dev, a, t, y, dtype)
    assert_exact(got, target_rank_ref(a, t, y))
    assert got[0][0, P - 1] == -1 and got[1][0, P - 1] == float("-inf")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_widest_rows_and_most_labels(dev, dtype):
    """E = 256 takes the small arrangements (rows of 512 and 1 024 bytes), P = 16 the thresholds kept in LDS"""
    a, t, y = int_case(300, 256, 16)
    assert_exact(run(dev, a, t, y, dtype), target_rank_ref(a, t, y))


@gpu
@dtype_sim[0]
@dtype_sim[1]
def test_same_bits_in_both_kernels(dev, dtype, sim):
    """Sample b's label row is 2 a_b -- its best target by far -- and stands at five ids in all, the label the (b % 5)-th
    of them: the rank is exactly b % 5 only if the label's score from the list kernel and the copies' scores from the
    streaming kernel are the same bits."""
    a, t = real_case(dtype, 64)
    t = t.clone()
    spots = torch.randperm(1000, generator=torch.Generator().manual_seed(4))[:5 * B].reshape(B, 5).sort(dim=1)[0]
    t[spots.reshape(-1)] = (2 * a).repeat_interleave(5, dim=0)
    want = torch.arange(B) % 5
    y = spots.gather(1, want[:, None])
    # the construction, in fp64: nothing but the copies is near the label (fp64 sums of fp32 products are rounded too, in
    # an order that depends on the column, so the reference cannot decide among the copies themselves)
    assert bool((target_rank_ref(a, t, y, sim)[1] <= 4).all())
    assert torch.equal(run(dev, a, t, y, dtype, sim=sim)[0], want[:, None])


@gpu
@dtype_sim[0]
@dtype_sim[1]
@pytest.mark.parametrize("excl", [False, True])
def test_agrees_with_topk_scores(dev, dtype, sim, excl):
    F_ = _F()
    a, t = (x.to(dev, dtype) for x in real_case(dtype, 64))
    ex = F_.topk_scores(a, None, t, 4, sim=sim)[1] if excl else None      # the four best are taken out
    v, i = F_.topk_scores(a, None, t, 128, sim=sim, exclude=ex)
    far = torch.tensor([min(set(range(200)) - set(row)) for row in (i if ex is None else torch.cat([i, ex], 1)).tolist()])
    y = torch.stack([i[:, 5], i[:, 100], far.to(dev), i[:, 0]], dim=1)
    r, s = F_.target_ranks(a, None, t, y, sim=sim, exclude=ex)
    assert r[:, [0, 1, 3]].tolist() == [[5, 100, 0]] * B and bool((r[:, 2] >= 128).all())
    assert torch.equal(s[:, [0, 1, 3]], v[:, [5, 100, 0]])


@gpu
@dtype_sim[0]
@dtype_sim[1]
@pytest.mark.parametrize("E", [64, 40])
def test_real_valued(dev, dtype, sim, E):
    a, t = real_case(dtype, E)
    y = torch.randint(0, 1000, (B, 3), generator=torch.Generator().manual_seed(E))
    scores = target_rank_ref(a, t, y, sim)[0]
    bound = gamma(E if sim == "dot" else E + 16) * (a.double().abs() @ t.double().abs().T)
    if sim == "cosine":
        bound = bound / (a.double().norm(dim=1)[:, None] * t.double().norm(dim=1)[None, :])
    sl, bl = scores.gather(1, y)[:, :, None], bound.gather(1, y)[:, :, None]
    other = torch.arange(1000)[None, None, :] != y[:, :, None]
    lo = ((scores[:, None, :] > sl + bound[:, None, :] + bl) & other).sum(dim=2)
    hi = ((scores[:, None, :] >= sl - bound[:, None, :] - bl) & other).sum(dim=2)
    print(f"widest interval {int((hi - lo).max())}, of width 0: {float((hi == lo).double().mean()):.3f}")
    assert float((hi == lo).double().mean()) >= 0.9      # the inputs: the condition below is not vacuous
    r, s = run(dev, a, t, y, dtype, sim=sim)
    assert bool(((lo <= r) & (r <= hi)).all())
    assert bool(((s.double() - sl[:, :, 0]).abs() <= bl[:, :, 0]).all())


@gpu
@pytest.mark.parametrize("X,idt", [(1, torch.int32), (300, torch.int64), (300, torch.int32), (1, torch.int64)])
def test_exclusion(dev, X, idt):
    """the list: the other label, the label itself, duplicates of random ids, padding, ids past the range"""
    Vt = 300
    a, t, y = int_case(Vt, 32, 2, seed=1)
    g = torch.Generator().manual_seed(X)
    rnd = torch.randint(0, Vt, (B, 120), generator=g)
    ex = torch.cat([y[:, 1:], y[:, :1], rnd, rnd[:, :60], torch.full((B, 60), -1), torch.randint(Vt, Vt + 50, (B, 58), generator=g)], 1)
    ex = ex[:, torch.randperm(300, generator=g)] if X == 300 else ex[:, :X]
    ref = target_rank_ref(a, t, y, exclude=ex)
    assert X == 1 or not torch.equal(ref[1], target_rank_ref(a, t, y)[1])
    assert_exact(run(dev, a, t, y, torch.bfloat16, exclude=ex.to(idt).contiguous()), ref)


@gpu
def test_addressing_and_index_flag(dev):
    """a shared table: anchors through int32 ids and an offset, targets strictly inside it (700 rows: two target ranges
    for 70 anchors); then one anchor id and one label out of range"""
    F_ = _F()
    E, lo, hi, off = 32, 150, 850, 3
    g = torch.Generator().manual_seed(3)
    table = torch.randint(-2, 3, (900, E), generator=g).float()
    idx = torch.randint(0, 140, (B,), generator=g)
    y = torch.randint(0, hi - lo, (B, 2), generator=g)
    w = table.to(dev, torch.bfloat16)
    ref = target_rank_ref(table[idx + off], table[lo:hi], y)
    F_.index_errors_seen()
    got = F_.target_ranks(w, idx.to(dev, torch.int32), None, y.to(dev, torch.int32), anchor_offset=off, target_lo=lo, target_hi=hi)
    assert_exact((got[0].cpu(), got[1].cpu()), ref)
    assert not F_.index_errors_seen()
    again = F_.target_ranks(table[idx + off].to(dev, torch.bfloat16), None, w, y.to(dev), target_lo=lo, target_hi=hi)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    idx[5] = 900 - off      # one row past the table: a zero row, every score 0, the rank of a label is its id
    r, s = F_.target_ranks(w, idx.to(dev), None, y.to(dev), anchor_offset=off, target_lo=lo, target_hi=hi)
    assert F_.index_errors_seen()
    assert torch.equal(r[5].cpu(), y[5]) and s[5].tolist() == [0.0, 0.0] and torch.equal(r[6:], got[0][6:])
    y[7, 1] = hi - lo       # one label past the range
    r, s = F_.target_ranks(w, idx.to(dev), None, y[:, 1].to(dev), anchor_offset=off, target_lo=lo, target_hi=hi)
    assert F_.index_errors_seen() and tuple(r.shape) == (B, 1)
    assert int(r[7, 0]) == -1 and float(s[7, 0]) == float("-inf") and torch.equal(r[8:, 0], got[0][8:, 1])


@gpu
@pytest.mark.parametrize("shared", [False, True])
def test_module_equals_functional(dev, shared):
    from torecsys_amd.fused import EmbeddingPairScorer
    torch.manual_seed(2)
    m = EmbeddingPairScorer(32, 100 if not shared else 400, None if shared else 300, similarity="cosine",
                            target_offset=100 if shared else 0).to(dev)
    idx, y = torch.randint(0, 100, (B,), device=dev), torch.randint(-1, 300, (B, 5), device=dev)
    ex = torch.randint(-1, 300, (B, 4), device=dev)
    r, s = m.rank(idx, y, exclude=ex)
    tw = None if shared else m.target.weight
    rr, rs = _F().target_ranks(m.anchor.weight, idx, tw, y, target_lo=100 if shared else 0, sim="cosine", exclude=ex)
    assert torch.equal(r, rr) and torch.equal(s, rs) and tuple(r.shape) == (B, 5) and int(r.max()) < 300
    i = m.topk(idx, 128, exclude=ex)[1]      # a label in its own exclusion row is ranked, and never returned
    listed = (y[:, :, None] == ex[:, None, :]).any(dim=2)
    assert bool(((r < 0) | (r >= 128) | listed | (i.gather(1, r.clamp(0, 127)) == y)).all())


@pytest.mark.parametrize("case,exc", [("P0", ValueError), ("P17", ValueError), ("mixed", TypeError), ("strided", ValueError),
                                      ("range", ValueError), ("exclude", ValueError), ("X", NotImplementedError)])
def test_argument_errors_before_any_launch(case, exc):
    """CPU tensors: every check below comes before the device is looked at"""
    a, t = torch.zeros(4, 32), torch.zeros(200, 32)
    y = torch.zeros(4, {"P0": 0, "P17": 17}.get(case, 2), dtype=torch.int64)
    if case == "mixed":
        t = t.bfloat16()
    if case == "strided":
        t = torch.zeros(200, 64)[:, :32]
    ex = {"exclude": torch.zeros(3, 2, dtype=torch.int64), "X": torch.zeros(4, 1025, dtype=torch.int64)}.get(case)
    with pytest.raises(exc, match="target_ranks"):
        _F().target_ranks(a, None, t, y, target_hi=201 if case == "range" else None, exclude=ex)

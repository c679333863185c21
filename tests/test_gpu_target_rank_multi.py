"""functional.target_ranks(..., interests=G) (csrc/target_rank.hip, the multi-interest kernels) against the count of
tests/topk_multi_ref.py over score[u, j] = max over the user's G anchors.  Integer tables as tests/test_gpu_topk_multi.py:
ranks and label scores must EQUAL the reference.  P = 1 and 4 keep the thresholds in registers, P = 5 in LDS; every
fifth user's last label is padding."""
import pytest
import torch

from topk_multi_ref import U, dev, dtypes, int_tables, multi_rank_ref, same      # noqa: F401 (dev: a fixture)

gpu = pytest.mark.gpu


def ranks(dev, a, idx, t, y, G, dtype, flag=False, exclude=None, **kw):
    """the call on ``dev``; the index flag must read ``flag`` behind it"""
    from torecsys_amd import functional as F_
    F_.index_errors_seen()
    r, s = F_.target_ranks(a.to(dev, dtype), idx, t if t is None else t.to(dev, dtype), y.to(dev), interests=G,
                           exclude=None if exclude is None else exclude.to(dev), **kw)
    assert r.dtype == torch.int64 and s.dtype == torch.float32 and F_.index_errors_seen() == flag
    return r.cpu(), s.cpu().double()


def labels(Vt, P, seed):
    y = torch.randint(0, Vt, (U, P), generator=torch.Generator().manual_seed(seed))
    y[::5, P - 1] = -1
    return y


@gpu
@pytest.mark.parametrize("P", [1, 4, 5])
@pytest.mark.parametrize("Vt", [129, 5003])
@pytest.mark.parametrize("E", [32, "vec"])
@pytest.mark.parametrize("G", [2, 3, 4, 8, 16])
@dtypes
def test_exact_with_ties(dev, dtype, G, E, Vt, P):
    a, t = int_tables(G, Vt, (8 if dtype == torch.bfloat16 else 4) if E == "vec" else E)
    y = labels(Vt, P, G)
    got = ranks(dev, a, None, t, y, G, dtype)
    assert same(got, multi_rank_ref(a, t, G, y)) and got[0][0, P - 1] == -1 and got[1][0, P - 1] == float("-inf")


@gpu
def test_exclusion_per_user(dev):
    """the list, shuffled: the other label, the label itself, random ids and 60 of them again, padding, ids past the range"""
    a, t = int_tables(3, 300, 32, seed=1)
    y, g = labels(300, 2, 1), torch.Generator().manual_seed(1)
    rnd = torch.randint(0, 300, (U, 120), generator=g)
    ex = torch.cat([y[:, 1:], y[:, :1], rnd, rnd[:, :60], torch.full((U, 60), -1), torch.randint(300, 350, (U, 58), generator=g)], 1)
    ex = ex[:, torch.randperm(300, generator=g)].contiguous()
    ref = multi_rank_ref(a, t, 3, y, exclude=ex)
    assert not torch.equal(ref[0], multi_rank_ref(a, t, 3, y)[0]) and same(ranks(dev, a, None, t, y, 3, torch.bfloat16, exclude=ex), ref)


@gpu
@pytest.mark.parametrize("G", [3, 8])
@pytest.mark.parametrize("sim", ["dot", "cosine"])
@dtypes
def test_same_bits(dev, dtype, sim, G):
    """identical rows per user: today's ranks and scores on the U distinct rows; and for labels taken from a k = 128
    multi-interest top-k result, their column and their value bits"""
    from torecsys_amd import functional as F_
    g = torch.Generator().manual_seed(7)
    a, t, q = torch.randn(U, 64, generator=g), torch.randn(1000, 64, generator=g), torch.randn(U * G, 64, generator=g)
    y = torch.randint(0, 1000, (U, 2), generator=g)
    assert same(ranks(dev, a.repeat_interleave(G, dim=0), None, t, y, G, dtype, sim=sim), ranks(dev, a, None, t, y, 1, dtype, sim=sim))
    v, i = F_.topk_scores(q.to(dev, dtype), None, t.to(dev, dtype), 128, sim=sim, interests=G)
    cols = [0, 5, 100, 127]
    r, s = ranks(dev, q, None, t, i[:, cols], G, dtype, sim=sim)
    assert r.tolist() == [cols] * U and torch.equal(s, v[:, cols].cpu().double())


@gpu
@pytest.mark.parametrize("bad", [False, True])
def test_addressing_and_index_flag(dev, bad):
    """a shared table: anchors through int32 ids and an offset, targets strictly inside it; ``bad``: one interest of user 5
    is a row past the table -- a zero row in that slot of its max, the flag raised, every other user as the reference"""
    G, lo, hi, off = 3, 150, 850, 3
    g = torch.Generator().manual_seed(3)
    table, idx = torch.randint(-2, 3, (900, 32), generator=g).float(), torch.randint(0, 140, (U * G,), generator=g)
    y, rows = torch.randint(0, hi - lo, (U, 2), generator=g), table[idx + off]
    if bad:
        idx[5 * G + 1], rows[5 * G + 1] = 900 - off, 0
    got = ranks(dev, table, idx.to(dev, torch.int32), None, y.int(), G, torch.bfloat16, flag=bad, anchor_offset=off, target_lo=lo, target_hi=hi)
    assert same(got, multi_rank_ref(rows, table[lo:hi], G, y))


@pytest.mark.parametrize("case", ["rows", "G0", "G17", "labels", "exclude"])
def test_argument_errors_before_any_launch(case):
    """CPU tensors: every check below comes before the device is looked at"""
    from torecsys_amd import functional as F_
    y = torch.zeros(12 if case == "labels" else 3, 2, dtype=torch.int64)
    ex = torch.zeros(12, 2, dtype=torch.int64) if case == "exclude" else None
    with pytest.raises(ValueError, match="target_ranks"):
        F_.target_ranks(torch.zeros(14 if case == "rows" else 12, 32), None, torch.zeros(200, 32), y, exclude=ex,
                        interests={"G0": 0, "G17": 17}.get(case, 4))

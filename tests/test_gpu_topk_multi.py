"""functional.topk_scores(..., interests=G) (csrc/topk.hip, the multi-interest kernels) against tests/topk_multi_ref.py:
score[u, j] = max over the user's G anchors.  Integer tables: values and ids must EQUAL the reference.  G = 3 is padded to
4 rows on chip; Vt = 129 is one past a tile, 5 003 several ranges with a partial last tile; k = 128 takes the per-user
sizing of the candidate buffers.  Real values: test_gpu_topk.test_real_valued's assertions with the max of the G bounds."""
import pytest
import torch

from topk_multi_ref import U, dev, dtypes, int_tables, multi_scores, multi_topk_ref, same      # noqa: F401 (dev: a fixture)

gpu = pytest.mark.gpu


def topk(dev, a, idx, t, G, k, dtype, flag=False, **kw):
    """the call on ``dev``; the index flag must read ``flag`` behind it"""
    from torecsys_amd import functional as F_
    F_.index_errors_seen()
    v, i = F_.topk_scores(a.to(dev, dtype), idx, t if t is None else t.to(dev, dtype), k, interests=G, **kw)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and F_.index_errors_seen() == flag
    return v.cpu().double(), i.cpu()


@gpu
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("Vt", [129, 5003])
@pytest.mark.parametrize("E", [32, "vec"])
@pytest.mark.parametrize("G", [2, 3, 4, 8, 16])
@dtypes
def test_exact_with_ties(dev, dtype, G, E, Vt, k):
    a, t = int_tables(G, Vt, (8 if dtype == torch.bfloat16 else 4) if E == "vec" else E)
    assert same(topk(dev, a, None, t, G, k, dtype), multi_topk_ref(a, t, G, k))


@gpu
@pytest.mark.parametrize("X,idt", [(1, torch.int32), (300, torch.int64)])
def test_exclusion_per_user(dev, X, idt):
    """(U, X) lists that hold the reference's top 3"""
    a, t = int_tables(3, 300, 32, seed=1)
    rnd = torch.randint(0, 300, (U, 40), generator=torch.Generator().manual_seed(X))
    ex = torch.cat([multi_topk_ref(a, t, 3, 3)[1], rnd, torch.full((U, X), -1)], dim=1)[:, :X].contiguous()
    assert same(topk(dev, a, None, t, 3, 10, torch.bfloat16, exclude=ex.to(dev, idt)), multi_topk_ref(a, t, 3, 10, exclude=ex))


@gpu
@pytest.mark.parametrize("E", [64, 40])
@pytest.mark.parametrize("sim", ["dot", "cosine"])
@dtypes
def test_real_valued(dev, dtype, sim, E):
    G, Vt, k = 4, 1000, 10
    g = torch.Generator().manual_seed(11)
    a, t = torch.randn(U * G, E, generator=g).to(dtype).float(), torch.randn(Vt, E, generator=g).to(dtype).float()
    scores, bound = multi_scores(a, t, G, sim)
    v, i = topk(dev, a, None, t, G, k, dtype, sim=sim)
    assert int(i.min()) >= 0 and int(i.max()) < Vt and all(len(set(row)) == k for row in i.tolist())
    assert bool(((v - scores.gather(1, i)).abs() <= bound.gather(1, i)).all())
    assert bool((v[:, 1:] <= v[:, :-1]).all())
    assert bool((v[:, -1] >= multi_topk_ref(a, t, G, k, sim)[0][:, -1] - bound.amax(dim=1)).all())


@gpu
@pytest.mark.parametrize("G", [3, 8])
@pytest.mark.parametrize("sim", ["dot", "cosine"])
@dtypes
def test_same_bits_as_single_interest(dev, dtype, sim, G):
    """every user's G rows identical: exactly what today's call returns on the U distinct rows"""
    g = torch.Generator().manual_seed(7)
    a, t = torch.randn(U, 64, generator=g), torch.randn(1000, 64, generator=g)
    assert same(topk(dev, a.repeat_interleave(G, dim=0), None, t, G, 100, dtype, sim=sim), topk(dev, a, None, t, 1, 100, dtype, sim=sim))


@gpu
@pytest.mark.parametrize("bad", [False, True])
def test_addressing_and_index_flag(dev, bad):
    """a shared table: anchors through int32 ids and an offset, targets strictly inside it; ``bad``: one interest of user 5
    is a row past the table -- a zero row in that slot of its max, the flag raised, every other user as the reference"""
    G, k, lo, hi, off = 3, 10, 150, 850, 3
    g = torch.Generator().manual_seed(3)
    table, idx = torch.randint(-2, 3, (900, 32), generator=g).float(), torch.randint(0, 140, (U * G,), generator=g)
    rows = table[idx + off]
    if bad:
        idx[5 * G + 1], rows[5 * G + 1] = 900 - off, 0
    got = topk(dev, table, idx.to(dev, torch.int32), None, G, k, torch.bfloat16, flag=bad, anchor_offset=off, target_lo=lo, target_hi=hi)
    assert same(got, multi_topk_ref(rows, table[lo:hi], G, k))


@pytest.mark.parametrize("case", ["rows", "G0", "G17", "exclude"])
def test_argument_errors_before_any_launch(case):
    """CPU tensors: every check below comes before the device is looked at"""
    from torecsys_amd import functional as F_
    ex = torch.zeros(12, 2, dtype=torch.int64) if case == "exclude" else None
    with pytest.raises(ValueError, match="topk_scores"):
        F_.topk_scores(torch.zeros(14 if case == "rows" else 12, 32), None, torch.zeros(200, 32), 5, exclude=ex,
                       interests={"G0": 0, "G17": 17}.get(case, 4))

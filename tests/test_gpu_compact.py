"""GPU: device-side row compaction (functional.compact_rows / trs_compact_rows), the replacement of
torch.unique(return_inverse=True) on the owner side of a large row-sharded table.  Integer results: every property is
checked exactly, the distinct count against torch.unique run eagerly here."""
import pytest
import torch

from conftest import rel_err
from torecsys_amd import functional as F_
from torecsys_amd.functional import compact_rows          # (absent before this feature: the module fails at collection)
from torecsys_amd.functional import compact_rows_dense

pytestmark = pytest.mark.gpu

V_BIG = 125_000_000          # rows of one BASELINE configs[4] shard
KS = [1, 63, 64, 65, 4096, 4097, 100_003]
PATTERNS = ["one_hot_row", "arange", "times_4096", "times_T", "uniform", "zipf", "padded", "past_the_table"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def slots_of(K):
    T = 2
    while T < 2 * K:
        T *= 2
    return T


def zipf_ids(K, V, g, s=1.05):
    """Zipf(s) ranks over V rows by inverting the continuous CDF (rank 1 = the hottest row)"""
    u = torch.rand(K, generator=g, dtype=torch.float64)
    a = 1.0 - s
    r = ((V ** a - 1.0) * u + 1.0) ** (1.0 / a)
    return (r.long() - 1).clamp_(0, V - 1)


def make_ids(pattern, K, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + K)
    T = slots_of(K)
    if pattern == "one_hot_row":
        ids = torch.full((K,), 77_777_777, dtype=torch.int64)
    elif pattern == "arange":
        ids = torch.arange(K)
    elif pattern == "times_4096":                  # the same low 12 bits; wrapped into int32 (the low bits stay equal)
        ids = (torch.arange(K) * 4096) & 0x7fffffff
    elif pattern == "times_T":
        ids = (torch.arange(K) * T) & 0x7fffffff
    elif pattern == "uniform":
        ids = torch.randint(0, V_BIG, (K,), generator=g)
    elif pattern == "zipf":
        ids = zipf_ids(K, V_BIG, g)
    elif pattern == "padded":                      # 30 % padding slots of a fixed-capacity exchange
        ids = torch.randint(0, V_BIG, (K,), generator=g)
        ids[torch.rand(K, generator=g) < 0.3] = -1
        if K == 1:
            ids[0] = -1
    elif pattern == "past_the_table":              # a few ids >= V, the largest int32 ones among them
        ids = torch.randint(0, V_BIG, (K,), generator=g)
        n = max(1, K // 50)
        where = torch.randperm(K, generator=g)[:n]
        ids[where] = torch.tensor([2 ** 31 - 5, V_BIG, V_BIG + 12345, 2 ** 31 - 1])[torch.arange(n) % 4]
    else:
        raise ValueError(pattern)
    return ids.to(torch.int32)


def check_compaction(ids, row_map, inv):
    K = ids.numel()
    T = slots_of(K)
    assert row_map.dtype == torch.int32 and inv.dtype == torch.int32
    assert row_map.shape == (T + 1,) and inv.shape == (K,)
    rm, iv = row_map.long(), inv.long()
    pos = ids >= 0
    assert bool(((iv >= 0) & (iv <= T)).all())
    # every id >= 0 sits in a slot < T that holds exactly that id
    assert bool((iv[pos] < T).all())
    assert torch.equal(rm[iv[pos]], ids[pos].long())
    # every id < 0 maps to the reserved slot, whose key is -1
    assert bool((iv[~pos] == T).all())
    assert int(rm[T]) == -1
    # as many occupied slots as distinct ids (with the line above: one slot per id, distinct ids in distinct slots)
    assert int((rm[:T] >= 0).sum()) == torch.unique(ids[pos]).numel()
    # slots nobody points at are empty
    hit = torch.zeros(T + 1, dtype=torch.bool, device=ids.device)
    hit[iv] = True
    assert bool((rm[~hit] == -1).all())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("K", KS)
def test_compact_rows_properties(dev, K, pattern):
    ids = make_ids(pattern, K).to(dev)
    row_map, inv = compact_rows(ids)
    check_compaction(ids, row_map, inv)


def check_dense(ids, dense_map, inv):
    """the densely numbered form: the same properties over K + 1 rows, and the occupied rows are exactly [0, U)"""
    K = ids.numel()
    assert dense_map.dtype == torch.int32 and inv.dtype == torch.int32
    assert dense_map.shape == (K + 1,) and inv.shape == (K,)
    dm, iv = dense_map.long(), inv.long()
    pos = ids >= 0
    U = torch.unique(ids[pos]).numel()
    assert bool(((iv >= 0) & (iv <= K)).all())
    assert bool((iv[pos] < U).all())
    assert torch.equal(dm[iv[pos]], ids[pos].long())
    assert bool((iv[~pos] == K).all())
    assert bool((dm[:U] >= 0).all()) and bool((dm[U:] == -1).all())
    assert torch.unique(dm[:U]).numel() == U          # distinct ids in distinct rows


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("K", KS)
def test_compact_rows_dense_properties(dev, K, pattern):
    ids = make_ids(pattern, K).to(dev)
    check_dense(ids, *compact_rows_dense(ids))


@pytest.mark.parametrize("pattern", ["uniform", "zipf"])
def test_compact_rows_dense_many_workgroups(dev, pattern):
    ids = make_ids(pattern, 1_048_576).to(dev)
    check_dense(ids, *compact_rows_dense(ids))
    ids2 = make_ids("padded", 1_048_576, seed=3).to(dev)          # again, through recycled allocations
    check_dense(ids2, *compact_rows_dense(ids2))


@pytest.mark.parametrize("pattern", ["uniform", "zipf"])
def test_compact_rows_many_workgroups(dev, pattern):
    """K = 2^20: 4096 workgroups race for the slots (T = 2^21 exactly: load 0.5)"""
    ids = make_ids(pattern, 1_048_576).to(dev)
    row_map, inv = compact_rows(ids)
    check_compaction(ids, row_map, inv)


def test_compact_rows_reuses_its_buffers(dev):
    """two calls into the SAME outputs with different ids: the second must not see the keys of the first (the clear is
    part of the entry)"""
    K = 4097
    a, b = make_ids("uniform", K, seed=1).to(dev), make_ids("padded", K, seed=2).to(dev)
    out = compact_rows(a)
    check_compaction(a, *out)
    out2 = compact_rows(b, out=out)
    assert out2[0].data_ptr() == out[0].data_ptr() and out2[1].data_ptr() == out[1].data_ptr()
    check_compaction(b, *out2)


def test_compact_rows_argument_errors(dev):
    with pytest.raises(TypeError):
        compact_rows(torch.zeros(4, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError):
        compact_rows(torch.zeros(4, dtype=torch.int32))          # CPU tensor: no fallback
    with pytest.raises(ValueError):
        compact_rows(torch.zeros(4, dtype=torch.int32, device=dev),
                     out=(torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)))


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("E", [1, 64])
def test_compacted_update_equals_index_add(dev, E, dense):
    """compact_rows (or its densely numbered form, which the sharded owner uses) -> row_buckets over the compact rows ->
    scatter_rows_update_mapped (SGD, fp32) == index_add_ of
    -lr * g on a copy of the table; repeats (30 000 ids over 5000 rows, a hot row), padding and ids past the table, which
    update nothing.  1e-5: the project's fp32 bound for re-ordered sums."""
    from torecsys_amd.optim import FusedSparseSGD
    g = torch.Generator().manual_seed(5)
    K, V, lr = 30_000, 5000, 0.05
    ids = torch.randint(0, V, (K,), generator=g)
    ids[torch.rand(K, generator=g) < 0.1] = 17                       # a hot row: the long-row kernels
    ids[torch.rand(K, generator=g) < 0.2] = -1
    ids[torch.randperm(K, generator=g)[:5]] = torch.tensor([V, V + 1, 2 ** 31 - 5, V + 99, V])
    ids = ids.to(torch.int32).to(dev)
    W = torch.randn(V, E, generator=g).to(dev)
    G = torch.randn(K, E, generator=g).to(dev)
    ok = (ids >= 0) & (ids < V)
    ref = W.clone().index_add_(0, ids[ok].long(), -lr * G[ok])
    row_map, inv = compact_rows_dense(ids) if dense else compact_rows(ids)
    rb = F_.row_buckets(inv.view(-1, 1), None, row_map.numel())
    table = W.clone()
    F_.scatter_rows_update_mapped(rb, table, FusedSparseSGD(lr), G, row_map)
    err = rel_err(table, ref)
    print(f"compacted SGD update E={E} dense={dense}: rel_err {err:.3e}")
    assert err <= 1e-5
    assert not torch.equal(table, W)

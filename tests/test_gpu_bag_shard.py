"""GPU: the sharded bag-pooling kernels (csrc/bag_shard.hip) with one process playing every owner, and
dist.RowShardedListIndicesEmbedding on an nccl group of one rank, against functional.bag_pool / ListIndicesEmbedding on the
whole table.  Integer-valued operands make fp32 sums exact in any order, so those comparisons are bit equalities."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bag_shard_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _ops():
    from torecsys_amd.dist import HipOps
    return HipOps()


def _int_table(V, E, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, (V, E), generator=g).to(dtype).to(DEV)


def _route_and_pool(table, idx, world, mean, check_route=True):
    """route -> every owner's bag_pool_segments on its slice of the table -> stack -> combine"""
    from torecsys_amd.dist import shard_ranges
    ops = _ops()
    V = table.shape[0]
    B, L = idx.shape
    per, ranges = shard_ranges(V, world)
    counts, seg_start, send_ids = ops.bag_route(idx, V, per, world)
    seg = seg_start.cpu()
    if check_route:
        rc, rs, ri, _ = R.route(idx.cpu(), V, per, world)
        assert torch.equal(counts.cpu(), rc) and torch.equal(seg, rs)
        assert torch.equal(send_ids.cpu()[: ri.numel()], ri)
    parts = []
    for w, (lo, hi) in enumerate(ranges):
        a, b = int(seg[w * B]), int(seg[(w + 1) * B])
        shard = table[lo:hi] if hi > lo else table[:1]            # an empty shard still has a (never read) row
        parts.append(ops.bag_pool_segments(shard, hi - lo, send_ids[a:b], seg_start[w * B: (w + 1) * B + 1] - a))
    return ops.bag_combine(torch.stack(parts), R.scale_of(L, mean), table.dtype)


def _patterned_ids(B, L, V, world, idt, seed):
    from torecsys_amd.dist import shard_ranges
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, V, (B, L), generator=g)
    per, ranges = shard_ranges(V, world)
    lo, hi = [r for r in ranges if r[1] > r[0]][-1]
    idx[0] = torch.randint(lo, hi, (L,), generator=g)            # every id of sample 0 on the last owner that has rows
    if L >= 3:
        idx[B - 1, :3] = int(idx[B - 1, 0])                      # one row three times in one sample
    return idx.to(idt).to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_kernels_bit_equal_bag_pool(world, dtype):
    """B x L x E x index dtype, sum and mean: outputs bit-equal to functional.bag_pool on the full table, counts and
    send_ids equal to the reference.  V = 5 keeps whole samples on one owner, so L = 300 gives segments longer than 256;
    E = 1 and 48 take the element path, 16 / 64 / 128 the lane-group path."""
    from torecsys_amd import functional as F_
    F_.index_errors_seen()
    for V in (5, 37):
        for E in (1, 16, 48, 64, 128):
            table = _int_table(V, E, dtype, 7 * E + V)
            for B in (1, 5, 257):
                for L in (1, 3, 64, 65, 300):
                    if V == 37 and (B, L) not in ((5, 65), (257, 3), (1, 300)):
                        continue
                    if B == 257 and L in (64, 300) and E != 64:      # the two largest shapes at one width only (every width keeps
                        # B = 257 at L = 65 and L = 300 at B = 5): keeps the test quick
                        continue
                    idt = torch.int32 if (B + L + E) % 2 else torch.int64
                    idx = _patterned_ids(B, L, V, world, idt, B * 1000 + L)
                    for mean in (False, True):
                        got = _route_and_pool(table, idx, world, mean, check_route=not mean)
                        want = F_.bag_pool(table, idx, "mean" if mean else "sum").squeeze(1)
                        assert torch.equal(got, want), (V, E, B, L, idt, mean)
    assert not F_.index_errors_seen()


@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_empty_shard_and_long_segments(idt):
    """V = 2 over 3 ranks: the last shard has no rows; every sample's 300 lookups fall on two owners (segments > 256)"""
    from torecsys_amd import functional as F_
    table = _int_table(2, 64, torch.float32, 1)
    idx = _patterned_ids(5, 300, 2, 3, idt, 2)
    for mean in (False, True):
        assert torch.equal(_route_and_pool(table, idx, 3, mean), F_.bag_pool(table, idx, "mean" if mean else "sum").squeeze(1))


@pytest.mark.parametrize("E", [16, 48])
def test_out_of_range_ids_are_zero_rows_and_flagged(E):
    from torecsys_amd import functional as F_
    V, B, L = 37, 5, 65
    table = _int_table(V, E, torch.float32, 3)
    idx = _patterned_ids(B, L, V, 3, torch.int64, 4)
    idx[1, 2], idx[2, 64], idx[4, 0] = V, -1, 10 ** 12
    F_.index_errors_seen()
    got = _route_and_pool(table, idx, 3, False)
    assert F_.index_errors_seen(), "the route must raise the index flag"
    assert torch.equal(got, F_.bag_pool(table, idx, "sum").squeeze(1))
    F_.index_errors_seen()
    # a local id outside the shard's valid rows on the owner: zero row and the flag
    ops = _ops()
    ids = torch.tensor([1, 9, 2], dtype=torch.int32, device=DEV)
    seg = torch.tensor([0, 3], dtype=torch.int32, device=DEV)
    out = ops.bag_pool_segments(table, 9, ids, seg)
    assert F_.index_errors_seen()
    assert torch.equal(out[0], table[1] + table[2])


def _ulp_bf16(x):
    """one bf16 unit in the last place at |x| (8 significant bits)"""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_random_rows_against_float64(dtype, mean):
    """B = 257, L = 65, E = 64, W = 3, rows uniform in [0.5, 1.5): no cancellation, so the bounds measure the sum itself.
    fp32: 1e-5 relative (the project's bound for interaction sums) of the float64 sum; bf16: one bf16 ulp of the float64
    sum rounded to bf16 -- only the order of the fp32 sum differs before the single rounding.  functional.bag_pool is held
    to the same bounds on the same inputs."""
    from torecsys_amd import functional as F_
    B, L, E, V, world = 257, 65, 64, 1000, 3
    g = torch.Generator().manual_seed(5)
    table = (torch.rand(V, E, generator=g) + 0.5).to(dtype)
    idx = torch.randint(0, V, (B, L), generator=g)
    ref = table.double()[idx].sum(1) * (float(R.scale_of(L, True)) if mean else 1.0)
    table, idx = table.to(DEV), idx.to(DEV)
    got = _route_and_pool(table, idx, world, mean).cpu()
    base = F_.bag_pool(table, idx, "mean" if mean else "sum").squeeze(1).cpu()
    for name, x in (("bag_pool", base), ("sharded", got)):
        if dtype == torch.float32:
            err = rel_err(x, ref)
            print(f"{name} fp32 mean={mean}: rel_err {err:.3e}")
            assert err <= 1e-5, name
        else:
            want = ref.to(torch.bfloat16)
            ulps = float(((x.double() - want.double()).abs() / _ulp_bf16(want)).max())
            print(f"{name} bf16 mean={mean}: {ulps:.2f} ulp")
            assert ulps <= 1.0, name


@pytest.mark.parametrize("E", [64, 48])
def test_backward_kernels_as_rank_1_of_3(E):
    """bag_expand_grad + shard_grad_dense on the segments rank 1 receives from three senders == rows [lo, hi) of the
    unsharded bag_pool gradient (integer g, fp32: equal); the padding row is zero; ids_bwd is -1 exactly at its lookups"""
    from torecsys_amd import functional as F_
    from torecsys_amd.dist import segment_starts, shard_ranges
    ops = _ops()
    V, B, L, world, me = 37, 33, 65, 3, 1
    per, ranges = shard_ranges(V, world)
    lo, hi = ranges[me]
    pad = lo + 1
    gen = torch.Generator().manual_seed(9)
    table = _int_table(V, E, torch.float32, 8).requires_grad_()
    idxs = [_patterned_ids(B, L, V, world, torch.int64, 20 + p) for p in range(world)]
    gs = [torch.randint(-4, 5, (B, E), generator=gen).float().to(DEV) for _ in range(world)]
    recv_counts, recv_ids = [], []
    for idx in idxs:
        counts, seg_start, send_ids = ops.bag_route(idx, V, per, world)
        a, b = int(seg_start[me * B]), int(seg_start[(me + 1) * B])
        recv_counts.append(counts[me])
        recv_ids.append(send_ids[a:b])
    ids = torch.cat(recv_ids)
    rseg = segment_starts(torch.stack(recv_counts))
    g_all = torch.cat(gs)
    rows, ids_bwd = ops.bag_expand_grad(g_all, ids, rseg, hi - lo, pad - lo)
    want_rows, want_ids = R.expand_grad(g_all.cpu(), ids.cpu(), rseg.cpu(), hi - lo, pad - lo)
    assert torch.equal(rows.cpu(), want_rows) and torch.equal(ids_bwd.cpu(), want_ids)
    assert torch.equal(ids_bwd == -1, ids == pad - lo) and bool((ids == pad - lo).any())
    gw = ops.shard_grad_dense(table.detach()[lo:hi], ids_bwd, rows, padded=True)
    loss = sum((F_.bag_pool(table, idx, "sum", pad).squeeze(1) * g).sum() for idx, g in zip(idxs, gs))
    loss.backward()
    assert torch.equal(gw, table.grad[lo:hi])
    assert not gw[pad - lo].any()


# ---- the module on an nccl group of one rank -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pg():
    assert torch.cuda.is_available()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    yield
    dist.destroy_process_group()


def _pair(method, dtype, W, **kw):
    from torecsys_amd.dist import RowShardedListIndicesEmbedding
    from torecsys_amd.inputs import ListIndicesEmbedding
    V, E = W.shape
    a = ListIndicesEmbedding(E, V, padding_idx=0, output_method=method).to(DEV).to(dtype)
    a.embedding.weight.data.copy_(W)
    b = RowShardedListIndicesEmbedding(E, V, padding_idx=0, output_method=method, dtype=dtype, device=DEV, **kw)
    b.load_full_weight(W.to(DEV).to(dtype))
    return a, b


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("method", ["sum", "avg_pooling", "mean"])
def test_module_world1_equals_unsharded_on_integers(pg, method, dtype):
    """forward bit-equal in both dtypes, fp32 dense gradient bit-equal.  L = 16: the mean's gradient terms g / 16 are exact,
    so their sums do not depend on the order the two backward paths add them in."""
    V, E, B, L = 1000, 64, 300, 16
    g = torch.Generator().manual_seed(12)
    W = torch.randint(-4, 5, (V, E), generator=g).float()
    idx = torch.randint(0, V, (B, L), generator=g)
    idx[::3, 5:] = 0                                              # padded tails
    idx = idx.to(DEV)
    go = torch.randint(-4, 5, (B, 1, E), generator=g).to(dtype).to(DEV)
    res = []
    for m in _pair(method, dtype, W):
        out = m(idx)
        assert out.names == ("B", "N", "E") and out.shape == (B, 1, E) and out.dtype == dtype
        (out.rename(None) * go).sum().backward()
        res.append((out.rename(None).detach(), m.embedding.weight.grad))
    assert torch.equal(res[0][0], res[1][0])
    if dtype == torch.float32:
        assert torch.equal(res[0][1], res[1][1])
    else:
        assert rel_err(res[1][1].float(), res[0][1].float()) <= 1e-2
    assert not res[1][1][0].any()                                 # the padding row


def test_module_world1_random_bf16_gradient(pg):
    V, E, B, L = 1000, 64, 300, 50
    g = torch.Generator().manual_seed(13)
    W = torch.randn(V, E, generator=g)
    idx = torch.randint(0, V, (B, L), generator=g).to(DEV)
    go = torch.randn(B, 1, E, generator=g).to(torch.bfloat16).to(DEV)
    res = []
    for m in _pair("avg_pooling", torch.bfloat16, W):
        out = m(idx)
        (out.rename(None).float() * go.float()).sum().backward()
        res.append((out.rename(None).detach().float(), m.embedding.weight.grad.float()))
    assert rel_err(res[1][0], res[0][0]) <= 1e-2
    assert rel_err(res[1][1], res[0][1]) <= 1e-2                  # the bound of test_sharded_equals_unsharded (bf16, dense)


def test_module_world1_sparse_gradient(pg):
    V, E, B, L = 500, 16, 100, 7
    g = torch.Generator().manual_seed(14)
    W = torch.randint(-4, 5, (V, E), generator=g).float()
    idx = torch.randint(0, V, (B, L), generator=g).to(torch.int32).to(DEV)
    go = torch.randint(-4, 5, (B, 1, E), generator=g).float().to(DEV)
    a, b = _pair("sum", torch.float32, W, dense_grad_max_rows=0)
    for m in (a, b):
        (m(idx).rename(None) * go).sum().backward()
    gw = b.embedding.weight.grad
    assert gw.is_sparse
    assert torch.equal(gw.to_dense(), a.embedding.weight.grad)


@pytest.mark.parametrize("big_shard", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "adagrad"])
def test_module_world1_fused_optimizer(pg, kind, big_shard):
    """one step of the fused optimizer on the owner == the same optimizer on the unsharded module (tolerance of
    test_sharded_fused_optimizer_matches_unsharded); ``big_shard``: the compact-row path of a shard above the dense limit"""
    from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseSGD
    V, E, B, L = 800, 64, 200, 20
    g = torch.Generator().manual_seed(15)
    W = torch.randn(V, E, generator=g)
    idx = torch.randint(0, V, (B, L), generator=g).to(DEV)
    go = torch.randn(B, 1, E, generator=g).to(DEV)
    a, b = _pair("avg_pooling", torch.float32, W, dense_grad_max_rows=0 if big_shard else 10 ** 9)
    for m in (a, b):
        m.set_fused_optimizer(FusedSparseSGD(0.05) if kind == "sgd" else FusedSparseAdagrad(0.05))
        (m(idx).rename(None) * go).sum().backward()
        assert m.embedding.weight.grad is None
    assert rel_err(b.full_weight(), a.embedding.weight.detach()) <= 1e-5
    assert not torch.equal(b.full_weight().cpu(), W)


def test_module_world1_state_dict_round_trip(pg):
    from torecsys_amd.inputs import ListIndicesEmbedding
    W = torch.randn(50, 16, generator=torch.Generator().manual_seed(16))
    _, b = _pair("sum", torch.float32, W)
    assert list(b.state_dict().keys()) == ["embedding.weight"]
    fresh = ListIndicesEmbedding(16, 50, padding_idx=0, output_method="sum").to(DEV)
    fresh.load_state_dict(b.full_state_dict())
    assert torch.equal(fresh.embedding.weight.detach().cpu(), W)
    assert (b.length, b.field_size, b.embed_size, b.padding_idx) == (16, 50, 16, 0)


def test_refusals(pg):
    from torecsys_amd.dist import RowShardedListIndicesEmbedding
    for kw in (dict(output_method="max_pooling"), dict(output_method="none"), dict(use_attn=True)):
        with pytest.raises(NotImplementedError):
            RowShardedListIndicesEmbedding(16, 50, device=DEV, **kw)

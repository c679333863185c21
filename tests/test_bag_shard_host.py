"""Host side of the sharded bag pooling (dist.RowShardedListIndicesEmbedding, csrc/bag_shard.hip): the C entries exist and
refuse bad arguments before any launch, the torch reference of the route agrees with a brute-force loop, and the module's
choreography (count / id / partial exchanges, gradient all-gather, owner-side reduction) runs on gloo at world 2 and 3 with
the device ops replaced by tests/bag_shard_ref.CpuOps.  Values are integers in [-4, 4], so every comparison is an equality."""
import ctypes
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bag_shard_ref as R  # noqa: E402

ENTRIES = ["trs_bag_route_count", "trs_bag_route_place", "trs_bag_pool_segments", "trs_bag_combine", "trs_bag_expand_grad"]
OK, EINVAL, EDTYPE, ESHAPE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import _abi, build
    build.build()
    return _abi.load()


def test_abi_symbols_exist(lib):
    from torecsys_amd import _abi
    for n in ENTRIES:
        assert hasattr(lib, n) and n in _abi.SIGNATURES


def test_error_codes_before_any_launch(lib):
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)

    def count(idx=p, dt=0, B=4, L=3, V=10, per=5, world=2, counts=p):
        return lib.trs_bag_route_count(idx, dt, B, L, V, per, world, counts, null, null)

    def place(idx=p, dt=0, B=4, L=3, V=10, per=5, world=2, seg=p, ids=p, n=12):
        return lib.trs_bag_route_place(idx, dt, B, L, V, per, world, seg, ids, n, null)

    for f in (count, place):
        assert f(B=0, idx=null) == OK                       # empty batch: nothing touched, pointers may be NULL
        assert f(idx=null) == EINVAL
        assert f(dt=7) == EDTYPE
        assert f(world=0) == ESHAPE and f(world=65, per=1) == ESHAPE
        assert f(L=0) == ESHAPE and f(L=65536) == ESHAPE
        assert f(B=1 << 20, L=4096) == ESHAPE               # B*L = 2^32
        assert f(per=4) == EINVAL                           # 2 ranks x 4 rows do not cover 10
    assert count(counts=null) == EINVAL
    assert place(seg=null) == EINVAL and place(ids=null) == EINVAL
    assert place(n=0, ids=null) == OK

    def pool(shard=p, E=4, dt=0, ids=p, n=5, seg=p, S=3, out=p):
        return lib.trs_bag_pool_segments(shard, 10, E, dt, ids, n, seg, S, out, null, null)

    assert pool(S=0, shard=null, seg=null, out=null) == OK
    assert pool(shard=null) == EINVAL and pool(seg=null) == EINVAL and pool(out=null) == EINVAL and pool(ids=null) == EINVAL
    assert pool(dt=5) == EDTYPE
    assert pool(n=1 << 31) == ESHAPE

    def comb(parts=p, P=2, B=3, E=4, dt=1, out=p):
        return lib.trs_bag_combine(parts, P, B, E, 1.0, dt, out, null)

    assert comb(B=0, parts=null, out=null) == OK
    assert comb(parts=null) == EINVAL and comb(out=null) == EINVAL and comb(P=0) == EINVAL
    assert comb(dt=2) == EDTYPE

    def expand(g=p, dt=0, E=4, ids=p, n=5, seg=p, S=3, rows=p, idb=p):
        return lib.trs_bag_expand_grad(g, dt, E, ids, n, seg, S, 10, -1, rows, idb, null)

    assert expand(S=0, g=null) == OK and expand(n=0, ids=null) == OK
    for k in ("g", "ids", "seg", "rows", "idb"):
        assert expand(**{k: null}) == EINVAL, k
    assert expand(dt=9) == EDTYPE


def test_hip_ops_refuse_cpu_tensors():
    from torecsys_amd.dist import HipOps
    ops = HipOps()
    idx = torch.zeros(2, 3, dtype=torch.long)
    seg = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bag_route(idx, 10, 5, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bag_pool_segments(torch.zeros(5, 4), 5, torch.zeros(0, dtype=torch.int32), seg)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bag_combine(torch.zeros(1, 2, 4), 1.0, torch.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bag_expand_grad(torch.zeros(2, 4), torch.zeros(1, dtype=torch.int32), seg, 5, -1)


@pytest.mark.parametrize("world,V,B,L", [(1, 10, 5, 7), (2, 10, 5, 7), (3, 10, 5, 7), (3, 2, 4, 3), (8, 1000, 9, 70)])
def test_reference_route_agrees_with_brute_force(world, V, B, L):
    from torecsys_amd.dist import shard_ranges
    g = torch.Generator().manual_seed(world * 100 + L)
    idx = torch.randint(0, V, (B, L), generator=g)
    idx[0, 0], idx[B - 1, L - 1] = V, -1                  # not sent
    per, _ = shard_ranges(V, world)
    counts, seg_start, send_ids, bad = R.route(idx, V, per, world)
    want_ids, want_counts = [], torch.zeros(world, B, dtype=torch.int32)
    for w in range(world):
        for b in range(B):
            for l in range(L):
                r = int(idx[b, l])
                if 0 <= r < V and r // per == w:
                    want_ids.append(r - w * per)
                    want_counts[w, b] += 1
    assert bad and torch.equal(counts, want_counts)
    assert send_ids.tolist() == want_ids and int(seg_start[-1]) == len(want_ids) == B * L - 2
    assert torch.equal(seg_start[1:].long(), want_counts.reshape(-1).long().cumsum(0))


def test_refusals():
    """max is not linear and 'none' / attention need the rows: refused at construction, before any process group is asked"""
    from torecsys_amd.dist import RowShardedListIndicesEmbedding
    with pytest.raises(NotImplementedError, match="not linear"):
        RowShardedListIndicesEmbedding(4, 10, output_method="max_pooling")
    with pytest.raises(NotImplementedError, match="rows|row"):
        RowShardedListIndicesEmbedding(4, 10, output_method="none")
    with pytest.raises(NotImplementedError, match="attention"):
        RowShardedListIndicesEmbedding(4, 10, use_attn=True)


# ---- gloo -----------------------------------------------------------------------------------------------------------
B_, L_, E_, V_ = 5, 7, 4, 10


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batches(world, case):
    """one (B, L) id batch and one integer (B, E) output gradient per rank"""
    from torecsys_amd.dist import shard_ranges
    g = torch.Generator().manual_seed(11)
    per, ranges = shard_ranges(V_, world)
    hi_all = ranges[-2][1] if case == "idle_owner" else V_        # idle_owner: nobody looks up a row of the last rank
    idx = [torch.randint(0, hi_all, (B_, L_), generator=g) for _ in range(world)]
    for t in idx:
        t[0] = torch.randint(0, per, (L_,), generator=g)        # every id of sample 0 on owner 0: the others send zero rows
        t[1, :3] = 0                                            # the padding row, three times in one sample
    if case == "bad_ids":
        idx[0][2, 1] = V_ + 3
        idx[world - 1][3, 0] = -2
    gout = [torch.randint(-4, 5, (B_, E_), generator=g).float() for _ in range(world)]
    W = torch.randint(-4, 5, (V_, E_), generator=g).float()
    return W, idx, gout


def _reference(W, idx, gout, method, padding_idx):
    """single process: F.embedding on the whole table + sum / mean; the gradient as the sum over every rank's lookups in
    (rank, sample, list position) order -- the order the owners receive them in, so that the mean's non-integer terms
    add up to the same bits"""
    mean = method != "sum"
    c = torch.tensor(R.scale_of(L_, mean), dtype=torch.float32)
    outs, ids, rows = [], [], []
    for t, go in zip(idx, gout):
        ok = (t >= 0) & (t < V_)
        e = F.embedding(t.clamp(0, V_ - 1), W) * ok.unsqueeze(-1)
        outs.append(e.sum(1) * c)
        gl = (go * (1.0 / L_) if mean else go).unsqueeze(1).expand(B_, L_, E_)
        keep = ok & (t != (-1 if padding_idx is None else padding_idx))
        ids.append(t[keep])
        rows.append(gl[keep])
    grad = torch.zeros_like(W).index_add_(0, torch.cat(ids), torch.cat(rows))
    return outs, grad


def _worker(rank, world, port, method, padding_idx, sparse, case, optimizer, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torecsys_amd import dist as D
        from torecsys_amd import functional as F_
        W, idx, gout = _batches(world, case)
        m = D.RowShardedListIndicesEmbedding(E_, V_, padding_idx=padding_idx, output_method=method, ops=R.CpuOps(),
                                             dense_grad_max_rows=0 if sparse else 10 ** 9)
        assert list(m.state_dict().keys()) == ["embedding.weight"]
        per, ranges = D.shard_ranges(V_, world)
        assert m.row_range == ranges[rank] and m.rows_per_rank == per and m.length == E_ and m.field_size == V_
        assert m.padding_idx == padding_idx and m.embed_size == E_
        m.load_full_weight(W)
        assert torch.equal(m.full_weight(), W) and torch.equal(m.full_state_dict()["embedding.weight"], W)
        opt = None
        if optimizer is not None:
            from torecsys_amd.optim import FusedSparseSGD
            opt = FusedSparseSGD(0.5)
            m.set_fused_optimizer(opt)
        if case == "unequal":
            try:
                m(idx[rank][: B_ - rank])
                raise AssertionError("unequal local batch sizes must be refused")
            except RuntimeError as e:
                assert "same local batch size" in str(e)
            ret[rank] = "ok"
            return
        F_.index_errors_seen()
        for k in D.bag_wire_bytes:
            D.bag_wire_bytes[k] = 0
        out = m(idx[rank])
        assert out.names == ("B", "N", "E") and out.shape == (B_, 1, E_)
        ref_out, ref_grad = _reference(W, idx, gout, method, padding_idx)
        assert torch.equal(out.rename(None).squeeze(1), ref_out[rank]), "forward must be equal, not close"
        (out.rename(None).squeeze(1) * gout[rank]).sum().backward()
        # the flag is local to the rank that saw the id: the sender of a bad id raises it
        saw = F_.index_errors_seen()
        if case == "bad_ids":
            assert saw == (rank in (0, world - 1)), (rank, saw)
        else:
            assert not saw
        lo, hi = m.row_range
        gw = m.embedding.weight.grad
        if opt is not None:
            assert gw is None
            assert torch.equal(m.embedding.weight.data[: hi - lo], (W - 0.5 * ref_grad)[lo:hi])
        else:
            if sparse:
                assert gw.is_sparse
                gw = gw.to_dense()
            assert torch.equal(gw[: hi - lo], ref_grad[lo:hi]), "dense gradient must be equal, not close"
            if padding_idx is not None and lo <= padding_idx < hi:
                assert not gw[padding_idx - lo].any()
        # wire bytes of the step: what this rank sent to the others
        counts, _, _, _ = R.route(idx[rank], V_, per, world)
        n_other = int(counts.sum()) - int(counts[rank].sum())
        assert D.bag_wire_bytes == {"counts": (world - 1) * B_ * 4, "ids": n_other * 4, "partials": (world - 1) * B_ * E_ * 4,
                                    "g": (world - 1) * B_ * E_ * 4, "steps": 1}, D.bag_wire_bytes
        if case == "idle_owner" and rank == world - 1:
            assert not gw.any()
        ret[rank] = "ok"
    except Exception:  # noqa: BLE001
        import traceback
        ret[rank] = "FAIL: " + traceback.format_exc()
    finally:
        dist.destroy_process_group()


def _run(world, method, padding_idx, sparse=False, case="plain", optimizer=None):
    assert dist.is_gloo_available()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), method, padding_idx, sparse, case, optimizer, ret), nprocs=world, join=True)
    for r in range(world):
        assert ret.get(r) == "ok", ret.get(r)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("method,padding_idx", [("sum", 0), ("avg_pooling", None), ("mean", 0)])
def test_sharded_bag_gloo(world, method, padding_idx):
    """world 3 has a short last shard (rows 8, 9) and V not divisible by W; sample 0 lies on one owner"""
    _run(world, method, padding_idx)


@pytest.mark.parametrize("world,padding_idx", [(2, None), (3, 0)])
def test_sharded_bag_sparse_gradient_gloo(world, padding_idx):
    _run(world, "sum", padding_idx, sparse=True)


@pytest.mark.parametrize("sparse", [False, True])
def test_sharded_bag_rank_without_lookups_gloo(sparse):
    """no batch looks up rows 8, 9: rank 2 of 3 receives no ids at all, pools zero rows and ends with a zero gradient"""
    _run(3, "sum", 0, sparse=sparse, case="idle_owner")


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_bag_bad_ids_gloo(world):
    """an id >= V and a negative id: zero contribution, no gradient, the index flag raised on the rank that sent them"""
    _run(world, "avg_pooling", 0, case="bad_ids")


def test_sharded_bag_fused_optimizer_gloo():
    _run(3, "sum", 0, optimizer="sgd")


def test_sharded_bag_unequal_batch_is_refused_gloo():
    _run(2, "sum", 0, case="unequal")


def test_wire_bytes_world3():
    """the counters of a world-3 step equal the formulas (asserted inside every gloo worker; this case names it)"""
    _run(3, "mean", None)

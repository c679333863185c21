"""Plain torch restatement of the sharded bag-pooling data path (csrc/bag_shard.hip; dist.RowShardedListIndicesEmbedding):
route, per-owner segment pooling, combine, gradient expansion.  The reference of tests/test_gpu_bag_shard.py and, as
``CpuOps``, the stand-in for the HIP ops in the gloo runs of tests/test_bag_shard_host.py (tests only: the product default
is the HIP ops, which refuse CPU tensors).  The (counts, send_ids) layout is fully determined by the ids, so tests compare
it for equality."""
import torch


def route(idx, num_rows, rows_per_rank, world):
    """(B, L) global ids -> counts (W, B) int32, seg_start (W*B + 1) int32, send_ids (n) int32 -- LOCAL ids grouped by owner,
    then sample, then list order -- and whether an id outside [0, num_rows) was seen (such ids are not sent)."""
    B, L = idx.shape
    g = idx.reshape(-1).long().cpu()
    b = torch.arange(B).repeat_interleave(L)
    ok = (g >= 0) & (g < num_rows)
    owner = torch.div(g, rows_per_rank, rounding_mode="floor")
    key = (owner * B + b)[ok]
    order = torch.argsort(key, stable=True)              # stable: list order inside a segment
    send_ids = (g - owner * rows_per_rank)[ok][order].to(torch.int32)
    counts = torch.bincount(key, minlength=world * B)[: world * B].to(torch.int32).view(world, B)
    return counts, seg_starts(counts), send_ids, bool((~ok).any())


def seg_starts(counts):
    out = torch.zeros(counts.numel() + 1, dtype=torch.int32)
    out[1:] = torch.cumsum(counts.reshape(-1).long(), 0).to(torch.int32)
    return out


def pool_segments(shard, n_valid, ids, seg_start):
    """(S, E) fp32: rows ids[seg_start[s] : seg_start[s+1]] summed in list order in fp32; ids outside [0, n_valid) are zero
    rows.  -> (out, whether such an id was seen)"""
    S = seg_start.numel() - 1
    E = shard.shape[1]
    out = torch.zeros(S, E, dtype=torch.float32)
    bad = False
    sh = shard.detach().float().cpu()
    for s in range(S):
        for q in range(int(seg_start[s]), int(seg_start[s + 1])):
            r = int(ids[q])
            if 0 <= r < n_valid:
                out[s] = out[s] + sh[r]
            else:
                bad = True
    return out, bad


def combine(parts, scale, dtype):
    """(P, B, E) fp32 -> (B, E): summed over P in order, times the fp32 ``scale``, one rounding"""
    acc = torch.zeros_like(parts[0])
    for p in range(parts.shape[0]):
        acc = acc + parts[p]
    return (acc * torch.tensor(scale, dtype=torch.float32)).to(dtype)


def expand_grad(g_all, ids, seg_start, n_valid, pad_local_row):
    """-> grad_rows (n, E), ids_bwd (n) int32: -1 and a zero row for the padding row, ids outside the shard and the slots
    behind the last segment"""
    n = ids.numel()
    S, E = g_all.shape
    rows = torch.zeros(n, E, dtype=g_all.dtype)
    ids_bwd = torch.full((n,), -1, dtype=torch.int32)
    for s in range(S):
        for q in range(int(seg_start[s]), int(seg_start[s + 1])):
            r = int(ids[q])
            if 0 <= r < n_valid and r != pad_local_row:
                rows[q] = g_all[s]
                ids_bwd[q] = r
    return rows, ids_bwd


def scale_of(L, mean):
    """1.f / (float)L in fp32 arithmetic"""
    return float(torch.ones((), dtype=torch.float32) / torch.tensor(float(L), dtype=torch.float32)) if mean else 1.0


def sharded_pool(table, idx, world, mean, dtype=None):
    """the whole forward with one process playing every owner: (B, E) of ``dtype`` (default: the table's)"""
    from torecsys_amd.dist import shard_ranges
    V = table.shape[0]
    per, ranges = shard_ranges(V, world)
    counts, seg_start, send_ids, _ = route(idx, V, per, world)
    B = idx.shape[0]
    parts = []
    for w, (lo, hi) in enumerate(ranges):
        sl = slice(int(seg_start[w * B]), int(seg_start[(w + 1) * B]))
        seg = seg_start[w * B: (w + 1) * B + 1] - seg_start[w * B]
        shard = table[lo:hi] if hi > lo else table[:1]
        parts.append(pool_segments(shard, hi - lo, send_ids[sl], seg)[0])
    return combine(torch.stack(parts), scale_of(idx.shape[1], mean), dtype or table.dtype)


class CpuOps:
    """torch-CPU statement of the HipOps entries RowShardedListIndicesEmbedding and its owner-side reduction use"""

    @staticmethod
    def _flag(bad):
        if bad:
            from torecsys_amd import functional as F_
            F_._ErrFlag(torch.device("cpu")).t.fill_(1)

    def bag_route(self, idx, num_rows, rows_per_rank, world):
        counts, seg_start, send_ids, bad = route(idx, num_rows, rows_per_rank, world)
        self._flag(bad)
        return counts, seg_start, send_ids

    def bag_pool_segments(self, weight, n_valid, ids, seg_start):
        out, bad = pool_segments(weight, min(n_valid, weight.shape[0]), ids, seg_start)
        self._flag(bad)
        return out

    def bag_combine(self, parts, scale, dtype):
        return combine(parts, scale, dtype)

    def bag_expand_grad(self, g_all, ids, seg_start, n_valid, pad_local_row):
        return expand_grad(g_all, ids, seg_start, n_valid, pad_local_row)

    def shard_grad_dense(self, weight, ids, grad_rows, padded=False):
        keep = ids >= 0
        g = torch.zeros_like(weight)
        g.index_add_(0, ids[keep].long(), grad_rows[keep])
        return g

    def shard_update(self, weight, ids, grad_rows, opt, dense_index, padded=False):
        keep = ids >= 0
        ids, grad_rows = ids[keep], grad_rows[keep]
        with torch.no_grad():
            g = torch.zeros_like(weight, dtype=torch.float32)
            g.index_add_(0, ids.long(), grad_rows.float())
            touched = torch.zeros(weight.shape[0], dtype=torch.bool)
            touched[ids.long()] = True
            w = weight.data
            if opt.kind == 1:
                w[touched] -= (opt.lr * g[touched]).to(w.dtype)
            elif opt.kind == 2:
                st = opt.state_for(w)
                st[touched] += g[touched] ** 2
                w[touched] -= (opt.lr * g[touched] / (st[touched].sqrt() + opt.eps)).to(w.dtype)
            else:
                raise NotImplementedError

"""Retrieval metrics over the ``ranks (B, P)`` tensor of ``functional.target_ranks`` / ``EmbeddingPairScorer.rank``: plain
torch, any device, no kernel.  ``ranks[b, p]`` is the 0-based position of sample b's p-th held-out target among all
targets, -1 where there is none (padding): such entries are ignored, and a sample without any held-out target is left
out of the mean (no sample at all: nan).  Gains are binary.  Each function returns an fp64 scalar tensor."""
import torch


def _per_sample(ranks: torch.Tensor):
    r = ranks.reshape(ranks.shape[0], -1) if ranks.dim() != 2 else ranks
    live = r >= 0
    return r, live, live.any(dim=1)


def hit_rate_at_k(ranks: torch.Tensor, k: int) -> torch.Tensor:
    """share of the samples with at least one held-out target among their first k"""
    r, live, has = _per_sample(ranks)
    return (live & (r < k)).any(dim=1)[has].double().mean()


def ndcg_at_k(ranks: torch.Tensor, k: int) -> torch.Tensor:
    """DCG@k = sum over the held-out targets in the first k of 1 / log2(rank + 2), over the DCG of the ideal order (the n
    held-out targets of the sample at positions 0 .. min(n, k) - 1)"""
    r, live, has = _per_sample(ranks)
    dcg = torch.where(live & (r < k), 1.0 / torch.log2(r.clamp_min(0).double() + 2.0), 0.0).sum(dim=1)
    ideal = torch.cumsum(1.0 / torch.log2(torch.arange(r.shape[1], device=r.device).double() + 2.0), 0)
    n = live.sum(dim=1).clamp(1, max(1, min(int(k), r.shape[1])))
    return (dcg / ideal[n - 1])[has].mean()


def mean_reciprocal_rank(ranks: torch.Tensor) -> torch.Tensor:
    """mean of 1 / (1 + the best rank among the sample's held-out targets)"""
    r, live, has = _per_sample(ranks)
    best = torch.where(live, r, torch.iinfo(torch.int64).max).amin(dim=1)
    return (1.0 / (best[has].double() + 1.0)).mean()


def mean_average_precision_at_k(ranks: torch.Tensor, k: int) -> torch.Tensor:
    """AP@k = sum over the held-out targets in the first k of precision at their position, over min(n, k); precision at
    position r is the number of the sample's held-out targets at positions <= r over r + 1"""
    r, live, has = _per_sample(ranks)
    hit = live & (r < k)
    upto = (live[:, None, :] & (r[:, None, :] <= r[:, :, None])).sum(dim=2)      # held-out targets at or before each one
    ap = torch.where(hit, upto.double() / (r.clamp_min(0).double() + 1.0), 0.0).sum(dim=1)
    return (ap / live.sum(dim=1).clamp(1, max(1, int(k))))[has].mean()

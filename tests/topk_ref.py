"""fp64 reference of functional.topk_scores: all scores, a stable sort by (-score, id), exclusion, padding slots."""
import torch

COS_EPS = 1e-8


def topk_ref(anchors, targets, k, sim="dot", exclude=None):
    """``anchors`` (B, E) and ``targets`` (Vt, E): CPU tensors that already hold the table dtype's values.  Returns
    (scores (B, Vt) fp64, values (B, k) fp64, ids (B, k) int64); an excluded target sorts behind every other one and its
    slot reads -inf / -1."""
    a, t = anchors.double(), targets.double()
    scores = a @ t.T
    if sim == "cosine":
        scores = scores / (a.norm(dim=1).clamp_min(COS_EPS)[:, None] * t.norm(dim=1).clamp_min(COS_EPS)[None, :])
    key = -scores
    if exclude is not None:
        for b, row in enumerate(exclude.tolist()):
            key[b, [j for j in row if j >= 0]] = float("inf")
    key, ids = torch.sort(key, dim=1, stable=True)      # ties: the smaller id first
    key, ids = key[:, :k], ids[:, :k].clone()
    ids[key == float("inf")] = -1
    return scores, -key, ids


def gamma(n):
    """n roundings of relative size 2^-24: (1 + 2^-24)^n - 1 <= n 2^-24 / (1 - n 2^-24)"""
    return n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)

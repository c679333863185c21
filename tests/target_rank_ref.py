"""fp64 / int64 reference of functional.target_ranks: all scores, then a plain count per label."""
import torch

from topk_ref import topk_ref


def target_rank_ref(anchors, targets, labels, sim="dot", exclude=None):
    """``anchors`` (B, E), ``targets`` (Vt, E): CPU tensors that already hold the table dtype's values; ``labels`` (B, P),
    ``exclude`` (B, X) or None.  Returns (scores (B, Vt) fp64, ranks (B, P) int64, label_scores (B, P) fp64): the number
    of targets in front of the label by (score descending, id ascending), the excluded set dropped once, the label itself
    never dropped; -1 / -inf for a label outside [0, Vt)."""
    scores = topk_ref(anchors, targets, 1, sim)[0]
    Vt, ids = targets.shape[0], torch.arange(targets.shape[0])
    ranks = torch.full(labels.shape, -1, dtype=torch.int64)
    ls = torch.full(labels.shape, float("-inf"), dtype=torch.float64)
    for b, row in enumerate(labels.tolist()):
        drop = sorted({j for j in exclude[b].tolist() if 0 <= j < Vt}) if exclude is not None else []
        for p, l in enumerate(row):
            if 0 <= l < Vt:
                s = scores[b]
                front = (s > s[l]) | ((s == s[l]) & (ids < l))
                front[[j for j in drop if j != l]] = False
                ranks[b, p], ls[b, p] = int(front.sum()), s[l]
    return scores, ranks, ls

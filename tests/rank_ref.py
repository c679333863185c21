"""Plain torch composition of the pair scores and the ranking losses, for sizes tests/golden/rank.npz does not hold
(pinned to that fixture by tests/test_rank_host.py).  Runs anywhere torch runs; any float dtype."""
import torch
import torch.nn.functional as F

RANK_SHAPES = [(5, 3, 8), (4, 1, 10), (6, 5, 64), (3, 4, 16)]      # (B, K, E) of the fixture
# fixture name -> (kind, index into the fixture's margins, masked rule: 'sample' = apply_mask, 'drop' = TripletLoss)
LOSS_CASES = {"bpr": ("bpr", None, "sample"), "hinge": ("hinge", 0, "sample"), "adaptive": ("adaptive_hinge", 1, "sample"),
              "triplet": ("hinge", 2, "drop"), "triplet0": ("bpr", None, "drop"), "pointwise": ("pointwise", None, "sample")}


def shape_tag(shape):
    return "_".join(str(v) for v in shape)


def loss_cases():
    """(fixture name, reduction) of every stored loss"""
    return [(n, r) for n in ("bpr", "hinge", "adaptive", "triplet", "triplet0") for r in ("sum", "mean")] + \
        [("pointwise", "mean")]


def pair_scores_ref(aw, a_idx, tw, t_idx, a_off=0, t_off=0, sim="dot", valid=True):
    """(B, 1 + K) scores; ids outside their table read as zero rows when ``valid`` is False"""
    def rows(w, idx):
        if valid:
            return w[idx]
        ok = (idx >= 0) & (idx < w.shape[0])
        return w[idx.clamp(0, w.shape[0] - 1)] * ok.unsqueeze(-1).to(w.dtype)
    a = rows(aw, a_idx.long().reshape(-1, 1) + a_off)          # (B, 1, E)
    t = rows(tw, t_idx.long() + t_off)                         # (B, 1 + K, E)
    if sim == "dot":
        return (a * t).sum(dim=2)
    return F.cosine_similarity(a, t, dim=2)


def rank_terms(pos, neg, kind, margin=1.0):
    """the per-element terms: (B, K), or (B, 1) for the adaptive hinge"""
    p = pos.reshape(-1, 1)
    if kind == "pointwise":
        return (1.0 - torch.sigmoid(p)) + torch.sigmoid(neg)
    if kind == "bpr":
        return F.softplus(-(p - neg))
    if kind == "hinge":
        return torch.clamp(margin - p + neg, min=0.0)
    if kind == "adaptive_hinge":
        # the FIRST of equal maxima takes the gradient (what the fixture pins), whatever K and the device
        first = (neg == neg.max(dim=1, keepdim=True)[0]).to(torch.uint8).argmax(dim=1, keepdim=True)
        return torch.clamp(margin - p + neg.gather(1, first), min=0.0)
    raise ValueError(kind)


def rank_loss_ref(pos, neg, kind, margin=1.0, mask=None, reduction="sum"):
    """'sum' | 'mean' over the kept terms, 'sample': kept terms over the number of kept samples (apply_mask)"""
    terms = rank_terms(pos, neg, kind, margin)
    if mask is not None:
        terms = terms[mask]
    if reduction == "sum":
        return terms.sum()
    if reduction == "mean":
        return terms.mean()
    if reduction == "sample":
        return terms.sum() / (mask.sum() if mask is not None else terms.shape[0])
    raise ValueError(reduction)


def fixture_reduction(name, red, masked):
    """the ``rank_loss`` reduction that a fixture case stands for"""
    if masked and LOSS_CASES[name][2] == "sample":
        return "sample"
    return red

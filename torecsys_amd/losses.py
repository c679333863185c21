"""Ranking losses of the embedding models (same class names, constructor and forward signatures as
``torecsys.losses.ltr``), each one call into the ranking-loss kernel of libtrs_hip.so (functional.rank_loss).

Reference: losses/ltr/functional.py, pairwise_ranking_loss.py, pointwise_ranking_loss.py.  ``forward(pos_out, neg_out,
mask=None)`` takes positive scores (B, 1) and negative scores (B, K) in fp32 or bf16 and returns an fp32 scalar;
``neg_out=None`` reads ``pos_out`` as the (B, 1 + K) score matrix of ``functional.pair_scores`` in place.

With a mask the reference's classes return ``loss[mask].sum() / mask.sum()`` -- the kept terms over the number of kept
SAMPLES, whatever ``reduction`` says (the reduction of a scalar is the scalar) -- and so do these; ``TripletLoss`` instead
drops the masked samples and then takes its sum or mean.  ``AdaptiveHingeLoss`` computes the documented per-sample
formula max(0, margin - p + max_k n); the reference's function broadcasts it into a (B, B, 1) cross-sample matrix
(SURVEY.md section 9).  ``BayesianPersonalizedRankingLoss`` is evaluated as softplus(-(p - n)), finite where the
reference's ``sigmoid().log()`` overflows.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import functional as F_


def get_reduction(method) -> str:
    """'sum' | 'mean' | torch.sum | torch.mean -> 'sum' | 'mean'; anything else raises (the reference's get_reduction
    takes any callable or torch attribute name: the kernel divides, it does not call)."""
    if isinstance(method, str):
        if method in ('sum', 'mean'):
            return method
        raise AssertionError(f"{method} not found.")
    if method is torch.sum:
        return 'sum'
    if method is torch.mean:
        return 'mean'
    if callable(method):
        raise NotImplementedError("torecsys_amd.losses: reduction must be 'sum', 'mean', torch.sum or torch.mean")
    raise TypeError(f"{type(method).__name__} not allowed.")


class RankingLoss(nn.Module):
    def __init__(self):
        super().__init__()


class PairwiseRankingLoss(RankingLoss):
    pass


class PointwiseRankingLoss(RankingLoss):
    pass


def _masked(reduction: str, mask) -> str:
    return reduction if mask is None else 'sample'


class BayesianPersonalizedRankingLoss(PairwiseRankingLoss):
    """-log sigmoid(p - n).  pairwise_ranking_loss.py BayesianPersonalizedRankingLoss."""

    def __init__(self, reduction='sum'):
        super().__init__()
        self.reduction = get_reduction(reduction)

    def forward(self, pos_out: torch.Tensor, neg_out: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None):
        return F_.rank_loss(pos_out, neg_out, 'bpr', 0.0, mask, _masked(self.reduction, mask))


class HingeLoss(PairwiseRankingLoss):
    """max(0, margin - p + n).  pairwise_ranking_loss.py HingeLoss."""

    def __init__(self, margin: float = 1.0, reduction=torch.sum):
        super().__init__()
        self.margin = margin
        self.reduction = get_reduction(reduction)

    def forward(self, pos_outputs: torch.Tensor, neg_outputs: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None):
        return F_.rank_loss(pos_outputs, neg_outputs, 'hinge', self.margin, mask, _masked(self.reduction, mask))


class AdaptiveHingeLoss(PairwiseRankingLoss):
    """max(0, margin - p + max_k n), one term per sample.  pairwise_ranking_loss.py AdaptiveHingeLoss as documented."""

    def __init__(self, margin: Optional[float] = 1.0, reduction=torch.sum):
        super().__init__()
        self.margin = margin
        self.reduction = get_reduction(reduction)

    def forward(self, pos_outputs: torch.Tensor, neg_outputs: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None):
        return F_.rank_loss(pos_outputs, neg_outputs, 'adaptive_hinge', self.margin, mask,
                            _masked(self.reduction, mask))


class TripletLoss(PairwiseRankingLoss):
    """``nn.MarginRankingLoss(margin, reduction)`` on (p, n, 1), or with a zero / None margin ``nn.SoftMarginLoss`` on
    p - n; a mask drops its samples before the sum / mean.  pairwise_ranking_loss.py TripletLoss."""

    def __init__(self, margin: Optional[float] = 1.0, reduction: Optional[str] = 'sum'):
        super().__init__()
        if reduction not in ('sum', 'mean'):
            raise ValueError(f"torecsys_amd.losses.TripletLoss: reduction 'sum' or 'mean', got {reduction!r}")
        self.margin = margin
        self.reduction = reduction

    def forward(self, pos_out: torch.Tensor, neg_out: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None):
        if self.margin:
            return F_.rank_loss(pos_out, neg_out, 'hinge', self.margin, mask, self.reduction)
        return F_.rank_loss(pos_out, neg_out, 'bpr', 0.0, mask, self.reduction)


class PointwiseLogisticLoss(PointwiseRankingLoss):
    """(1 - sigmoid(p)) + sigmoid(n), mean.  pointwise_ranking_loss.py PointwiseLogisticLoss."""

    def __init__(self):
        super().__init__()

    @staticmethod
    def forward(pos_out: torch.Tensor, neg_out: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None):
        return F_.rank_loss(pos_out, neg_out, 'pointwise', 0.0, mask, _masked('mean', mask))

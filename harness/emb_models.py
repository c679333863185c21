"""Test harness (NOT product code): the two embedding models of the reference, restated on ids over the drop-in layers
and ``fused.EmbeddingPairScorer`` for the GPU box, where the reference package is absent.

  MatrixFactorizationModel   (B, 2, E) rows -> (B, 1) = GMF layer                      models/emb/matrix_factorization.py
  StarSpaceModel             context / target rows (B (1+K), 1, E) -> (B (1+K), 1)      models/emb/starspace.py
                             positives first per sample: row b (1+K) the positive, the K behind it the negatives

Both also score ids directly (``score_ids``): the path a training step takes, where neither block exists.
``in_batch_negatives`` reproduces the draw of the reference's ``UniformBatchMiner`` (miners/uniform_batch_miner.py:17-44)
as a (B, 1 + K) id matrix.  Outputs are un-named tensors, pinned to the reference by ``tests/golden/rank.npz``.
"""
from __future__ import annotations

from functools import partial
from typing import Any, Optional

import torch
import torch.nn as nn

from torecsys_amd.fused import EmbeddingPairScorer
from torecsys_amd.layers import GeneralizedMatrixFactorizationLayer, StarSpaceLayer, inner_product_similarity


def _plain(t: torch.Tensor) -> torch.Tensor:
    return t.rename(None) if t.has_names() else t


def in_batch_negatives(target_idx: torch.Tensor, K: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """(B,) target ids -> (B, 1 + K): column 0 the sample's own target, columns 1 .. K the targets of K other samples
    of the batch drawn as the reference's miner draws them: ``randint(0, B, (K * B,))`` on the host generator, negative
    ``b * K + k`` belonging to anchor ``b`` (the miner repeats every anchor K times in a row).  On ``target_idx``'s
    device."""
    t = _plain(target_idx).reshape(-1)
    B = t.shape[0]
    rand_idx = torch.randint(0, B, (K * B,), generator=generator)
    neg = t[rand_idx.to(t.device)].view(B, K)
    return torch.cat([t.unsqueeze(1), neg], dim=1)


class MatrixFactorizationModel(nn.Module):
    def __init__(self):
        super().__init__()
        self.mf = GeneralizedMatrixFactorizationLayer()

    def forward(self, emb_inputs: torch.Tensor) -> torch.Tensor:
        return _plain(self.mf(emb_inputs))

    @staticmethod
    def score_ids(scorer: EmbeddingPairScorer, anchor_idx: torch.Tensor, target_idx: torch.Tensor) -> torch.Tensor:
        """(B,) user ids and (B,) item ids -> (B, 1)"""
        return scorer(anchor_idx, _plain(target_idx).reshape(-1, 1))


class StarSpaceModel(nn.Module):
    def __init__(self, embed_size: int, num_neg: int, similarity: Any = partial(inner_product_similarity, dim=2)):
        super().__init__()
        self.embed_size = embed_size
        self.num_neg = num_neg
        self.starspace = StarSpaceLayer(similarity)

    def forward(self, context_inputs: torch.Tensor, target_inputs: torch.Tensor) -> torch.Tensor:
        c, t = _plain(context_inputs), _plain(target_inputs)
        n = c.shape[0]
        pair = torch.cat([c.reshape(n, 1, self.embed_size), t.reshape(n, 1, self.embed_size)], dim=1)
        return _plain(self.starspace(pair)).reshape(n, 1)

    @staticmethod
    def score_ids(scorer: EmbeddingPairScorer, anchor_idx: torch.Tensor, target_idx: torch.Tensor) -> torch.Tensor:
        """(B,) context ids and (B, 1 + K) target ids -> (B (1+K), 1), the reference's output order"""
        return scorer(anchor_idx, target_idx).reshape(-1, 1)

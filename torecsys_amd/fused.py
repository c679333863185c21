"""Fused modules: same parameters / state_dict keys as the reference's module pairs, one kernel instead of two.

``FusedFieldAwareFM`` = ``MultiIndicesFieldAwareEmbedding`` (multi_indices_field_aware_emb.py:24-111) followed by
``FieldAwareFactorizationMachineLayer`` (field_aware_factorization_machine.py:50-94): the reference materialises a
(B, N*N, E) tensor between the two (12.8 GB at B=65 536, N=39, E=64, bf16); here the pair products are gathered
straight from the N tables.  ``EmbeddingFM`` = ``MultiIndicesEmbedding`` + ``FactorizationMachineLayer``
(+ the first-order ``MultiIndicesEmbedding(embed_size=1)`` sum) in one pass over the rows.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch
import torch.nn as nn

from . import functional as F_
from .inputs import BaseInput, MultiIndicesEmbedding, field_offsets

# TRS_SELF_ATTN: 1 / 0 send every dtype residual_self_attention covers through functional.self_attn_residual / keep the
# nn.MultiheadAttention composition (the A/B baseline).  Unset (None): per dtype by what was measured at B = 65 536, L = 30,
# E = 64, H = 4 (profiles/self_attn_kernels.md) -- bf16 (MFMA path) on: 3.3x forward, 2.0x forward + backward; fp32 (vector
# path) off: 0.86x / 0.73x of the composition
_env = os.environ.get("TRS_SELF_ATTN")
SELF_ATTN = None if _env is None else _env not in ("", "0")


def self_attn_enabled(dtype: torch.dtype) -> bool:
    return dtype == torch.bfloat16 if SELF_ATTN is None else SELF_ATTN


def residual_self_attention(mha: nn.MultiheadAttention, x: torch.Tensor) -> torch.Tensor:
    """``x + mha(x, x, x)`` over the list dimension of an un-named batch-first (B, L, E) block: the attention half of an
    encoder layer of ``PersonalizedReRankingModel`` (models/ltr/personalized_reranking.py:126-146).  One HIP pass per
    direction (``functional.self_attn_residual``, csrc/self_attn.hip) for a HIP tensor in fp32 / bf16, an ``mha`` with one
    embedding size, no ``bias_k`` / ``add_zero_attn``, attention dropout 0 or eval mode, a shape ``self_attn_path`` takes
    and the switch ``TRS_SELF_ATTN`` (default: on for bf16, off for fp32, where the kernel was measured slower than the
    composition); every other case runs the reference's composition on the transposed block."""
    if (x.is_cuda and self_attn_enabled(x.dtype) and x.dim() == 3 and x.dtype in (torch.float32, torch.bfloat16)
            and mha._qkv_same_embed_dim and mha.bias_k is None and mha.bias_v is None and not mha.add_zero_attn
            and not getattr(mha, "batch_first", False) and (mha.dropout == 0 or not mha.training)
            and x.shape[2] == mha.embed_dim and mha.in_proj_weight.dtype == x.dtype
            and F_.self_attn_path(x.shape[1], x.shape[2], mha.num_heads, x.dtype) != 0):
        return F_.self_attn_residual(x, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias,
                                     mha.num_heads)
    xt = x.transpose(0, 1)
    return x + mha(xt, xt, xt)[0].transpose(0, 1)


class FusedFieldAwareFM(BaseInput):
    """(B,N) indices -> (B, N(N-1)/2, E) named ('B','N','E'); parameters ``embeddings.{i}.weight``."""

    def __init__(self, embed_size: int, field_sizes: List[int], device: str = 'cpu', dropout_p: float = 0.0):
        super().__init__()
        self.num_fields = len(field_sizes)
        self.embeddings = nn.ModuleList([nn.Embedding(sum(field_sizes), embed_size) for _ in range(self.num_fields)])
        for embedding in self.embeddings:
            nn.init.xavier_uniform_(embedding.weight.data)
        self.register_buffer('offsets', field_offsets(field_sizes), persistent=False)
        self.dropout = nn.Dropout(dropout_p)
        self.length = embed_size
        self.to(device)

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        idx = inputs.rename(None) if inputs.has_names() else inputs
        out = F_.ffm_fused([e.weight for e in self.embeddings], idx, self.offsets)
        out = self.dropout(out)
        out.names = ('B', 'N', 'E',)
        return out


class EmbeddingFM(nn.Module):
    """One kernel for ``emb = MultiIndicesEmbedding(E)(idx)``, ``FMLayer()(emb)`` and (optionally)
    ``MultiIndicesEmbedding(1)(idx).sum('N')``.  Holds the two input modules so their parameters keep the
    reference names (``emb.embedding.weight``, ``feat.embedding.weight``)."""

    def __init__(self, embed_size: int, field_sizes: List[int], first_order: bool = True, want_block: bool = True):
        super().__init__()
        self.emb = MultiIndicesEmbedding(embed_size=embed_size, field_sizes=field_sizes)
        self.feat = MultiIndicesEmbedding(embed_size=1, field_sizes=field_sizes) if first_order else None
        self.want_block = want_block

    def forward(self, inputs: torch.Tensor):
        idx = inputs.rename(None) if inputs.has_names() else inputs
        fw = None if self.feat is None else self.feat.embedding.weight
        emb, fm, first = F_.embed_fm(self.emb.embedding.weight, idx, self.emb.offsets, fw, self.want_block)
        if emb is not None:
            emb.names = ('B', 'N', 'E',)
        fm.names = ('B', 'O',)
        return emb, fm, first


class EmbeddingPairScorer(nn.Module):
    """ids -> (B, 1 + K) similarity scores of the embedding models (MatrixFactorizationModel, StarSpaceModel) in one kernel
    per direction (functional.pair_scores): ``forward(anchor_idx (B,), target_idx (B, 1 + K))``, column 0 of the target
    ids the positive, the others sampled negatives; K = 0 is the plain GMF score.  Replaces the reference's miner
    (anchor id repeated K times) + input layer ((B (1+K), 2, E) gather) + model (slice and multiply).
    Tables: ``anchor_size`` / ``target_size`` rows in two ``nn.Embedding``s (``anchor.weight``, ``target.weight``);
    ``target_size=None``: one shared table, ``target_offset`` then places the targets' rows behind the anchors' (as the
    field offsets of ``MultiIndicesEmbedding`` do); ``anchor=`` / ``target=`` borrow existing ``nn.Embedding``s.
    ``similarity``: 'dot' | 'cosine'.  ``set_fused_optimizer(opt)``: the backward applies the fused sparse SGD / Adagrad /
    Adam step to the looked-up rows instead of returning a dense gradient."""

    def __init__(self, embed_size: int, anchor_size: Optional[int] = None, target_size: Optional[int] = None,
                 similarity: str = 'dot', anchor_offset: int = 0, target_offset: int = 0, out_dtype=None,
                 anchor: Optional[nn.Embedding] = None, target: Optional[nn.Embedding] = None):
        super().__init__()
        if similarity not in F_.PAIR_SIMS:
            raise ValueError(f"similarity must be one of {sorted(F_.PAIR_SIMS)}, got {similarity!r}")
        if anchor is None:
            if anchor_size is None:
                raise ValueError("EmbeddingPairScorer: anchor_size or an anchor nn.Embedding is needed")
            anchor = nn.Embedding(anchor_size, embed_size)
            nn.init.xavier_uniform_(anchor.weight.data)
        if target is None and target_size is not None:
            target = nn.Embedding(target_size, embed_size)
            nn.init.xavier_uniform_(target.weight.data)
        if anchor.weight.shape[1] != embed_size or (target is not None and target.weight.shape[1] != embed_size):
            raise ValueError("EmbeddingPairScorer: the tables' rows must have embed_size columns")
        self.anchor = anchor
        self.target = None if target is anchor else target
        self.similarity = similarity
        self.anchor_offset, self.target_offset = int(anchor_offset), int(target_offset)
        self.out_dtype = out_dtype
        self._fused_opt = None

    def set_fused_optimizer(self, opt) -> None:
        self._fused_opt = opt

    def forward(self, anchor_idx: torch.Tensor, target_idx: torch.Tensor) -> torch.Tensor:
        tw = None if self.target is None else self.target.weight
        return F_.pair_scores(self.anchor.weight, anchor_idx, tw, target_idx, self.anchor_offset, self.target_offset,
                              self.similarity, self.out_dtype, self._fused_opt)


class BCEWithLogitsLoss(nn.Module):
    """``nn.BCEWithLogitsLoss()`` (mean reduction, no weights) on the HIP device: ``loss(logits, labels)`` with logits in
    fp32 or bf16 -- no ``.float()`` cast needed in front -- and 0/1 (or soft) labels in fp32 / bf16; an fp32 scalar.
    Forward two launches, backward one (functional.bce_with_logits) instead of ATen's ~16.  The loss SURVEY.md 8d defines
    the fwd+bwd metric on; configurations this module does not cover raise at construction."""

    def __init__(self, weight=None, size_average=None, reduce=None, reduction: str = 'mean', pos_weight=None):
        super().__init__()
        if weight is not None or pos_weight is not None or reduction != 'mean' or size_average is not None \
                or reduce is not None:
            raise NotImplementedError("torecsys_amd.fused.BCEWithLogitsLoss covers reduction='mean' without weights; use "
                                      "torch.nn.BCEWithLogitsLoss for anything else")

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return F_.bce_with_logits(input, target)

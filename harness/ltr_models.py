"""Test harness (NOT product code): the learning-to-rank model of the reference restated over the drop-in layers for the
GPU box, where the reference package is absent.

  PersonalizedReRankingModel   (B, L, embed_size) un-named -> (B, L) named ('B', 'O'), rows sum to 1
                               models/ltr/personalized_reranking.py

Same constructor signature, module tree and ``state_dict`` keys as the reference.  The attention and its residual add of
every encoder layer run through ``fused.residual_self_attention``; the BatchNorm1d(L) pairs, the feed-forward and the
output head are the model's own torch modules.  Deviations: ``dropout=None`` (the reference's default, which raises
``TypeError`` inside ``nn.MultiheadAttention``) is read as 0.0; ``use_bias=False`` (which raises at construction in the
reference: ``None`` in a ``ModuleDict``) is refused with a ``ValueError``.  Pinned to the reference by
``tests/golden/prm.npz``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from torecsys_amd.fused import residual_self_attention
from torecsys_amd.layers import PositionEmbeddingLayer


class PersonalizedReRankingModel(nn.Module):
    def __init__(self, embed_size: int, max_num_position: int, encoding_size: int, num_heads: int, num_layers: int,
                 use_bias: Optional[bool] = True, dropout: Optional[float] = None, **kwargs):
        super().__init__()
        if not use_bias:
            raise ValueError("PersonalizedReRankingModel: use_bias=False cannot be constructed in the reference either")
        dropout = 0.0 if dropout is None else dropout
        self.layers = nn.ModuleDict()
        self.layers['InputLayer'] = nn.ModuleDict()
        self.layers['InputLayer']['PositionEmbedding'] = PositionEmbeddingLayer(max_num_position=max_num_position)
        self.layers['InputLayer']['FeedForward'] = nn.Linear(embed_size, encoding_size)
        self.layers['EncodingLayer'] = nn.ModuleDict()
        for i in range(num_layers):
            layer = nn.ModuleDict()
            layer['MultiHeadAttention'] = nn.MultiheadAttention(encoding_size, num_heads, dropout)
            layer['AttentionBatchNorm'] = nn.BatchNorm1d(max_num_position)
            feedforward = nn.Sequential()
            feedforward.add_module('FeedForward', nn.Linear(encoding_size, encoding_size))
            feedforward.add_module('Activation', kwargs.get('fnn_activation') or nn.ReLU())
            if kwargs.get('fnn_dropout_p'):
                feedforward.add_module('Dropout', nn.Dropout(kwargs.get('fnn_dropout_p')))
            layer['FeedForward'] = feedforward
            layer['FNNBatchNorm'] = nn.BatchNorm1d(max_num_position)
            self.layers['EncodingLayer'][f'Transformer_{i}'] = layer
        self.layers['OutputLayer'] = nn.ModuleDict()
        self.layers['OutputLayer']['FeedForward'] = nn.Linear(encoding_size, 1)
        self.layers['OutputLayer']['Softmax'] = nn.Softmax(dim=1)

    def forward(self, feat_inputs: torch.Tensor) -> torch.Tensor:
        output = self.layers['InputLayer']['PositionEmbedding'](feat_inputs)
        output = self.layers['InputLayer']['FeedForward'](output)
        for i in range(len(self.layers['EncodingLayer'])):
            layer = self.layers['EncodingLayer'][f'Transformer_{i}']
            output = layer['AttentionBatchNorm'](residual_self_attention(layer['MultiHeadAttention'], output))
            output = layer['FNNBatchNorm'](layer['FeedForward'](output) + output)
        output = self.layers['OutputLayer']['FeedForward'](output)            # (B, L, 1)
        output = self.layers['OutputLayer']['Softmax'](output.flatten(1))
        output.names = ('B', 'O',)
        return output

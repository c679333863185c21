"""Test harness (NOT product code): the two models built on the mixture-of-experts layer, restated over the drop-in
layers for the GPU box, where the reference package is absent (a torecsys user keeps ``torecsys.models.ctr`` and calls
``torecsys_amd.patch``).  Constructor keywords and attribute names (``moe_layer``, ``towers.Tower_{i}``, ``module.{i}``)
are the reference's, so a reference ``state_dict`` loads by name; the forwards run on plain (un-named) tensors:

  MMoE     logit = sum_t Tower_t(moe(emb)[:, t:t+1])                                 models/ctr/multigate_moe.py
  DeepMoE  x <- moe_l(x) as (B, 1, K_l) for each layer l;  logit = sum_k x[b, 0, k]   models/ctr/deep_moe.py

Outputs are (B, 1) un-named tensors, pinned to the reference by ``tests/golden/moe.npz``.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from torecsys_amd.layers import DNNLayer, MOELayer


def _plain(t: torch.Tensor) -> torch.Tensor:
    return t.rename(None) if t.has_names() else t


class MultiGateMixtureOfExpertsModel(nn.Module):
    def __init__(self, embed_size: int, num_fields: int, num_tasks: int, num_experts: int, expert_output_size: int,
                 expert_layer_sizes: List[int], deep_layer_sizes: List[int],
                 expert_dropout_p: Optional[List[float]] = None, deep_dropout_p: Optional[List[float]] = None,
                 expert_activation: Optional[nn.Module] = nn.ReLU(), deep_activation: Optional[nn.Module] = nn.ReLU()):
        super().__init__()
        self.num_tasks = num_tasks
        self.moe_layer = MOELayer(inputs_size=embed_size * num_fields, output_size=num_experts * expert_output_size,
                                  num_gates=num_tasks, num_experts=num_experts, expert_func=DNNLayer,
                                  expert_inputs_size=embed_size * num_fields, expert_output_size=expert_output_size,
                                  expert_layer_sizes=expert_layer_sizes, expert_dropout_p=expert_dropout_p,
                                  expert_activation=expert_activation)
        self.towers = nn.ModuleDict()
        for i in range(num_tasks):
            self.towers[f'Tower_{i}'] = DNNLayer(inputs_size=expert_output_size * num_experts, output_size=1,
                                                 layer_sizes=deep_layer_sizes, dropout_p=deep_dropout_p,
                                                 activation=deep_activation)

    def forward(self, emb_inputs: torch.Tensor) -> torch.Tensor:
        gated = _plain(self.moe_layer(emb_inputs))                     # (B, num_tasks, K)
        chunks = torch.chunk(gated, self.num_tasks, dim=1)             # (B, 1, K) views, as the reference hands them over
        outs = [_plain(tower(chunks[i])) for i, tower in enumerate(self.towers.values())]      # (B, 1, 1) each
        return torch.cat(outs, dim=1).sum(dim=1)


class DeepMixtureOfExpertsModel(nn.Module):
    def __init__(self, embed_size: int, num_fields: int, num_experts: int, moe_layer_sizes: List[int],
                 deep_layer_sizes: List[int], deep_dropout_p: Optional[List[float]] = None,
                 deep_activation: Optional[nn.Module] = nn.ReLU()):
        super().__init__()
        sizes = [embed_size * num_fields] + list(moe_layer_sizes)
        self.module = nn.ModuleList()
        for i, (inp, out) in enumerate(zip(sizes[:-1], sizes[1:])):
            inp = num_experts * inp if i != 0 else inp
            self.module.append(MOELayer(inputs_size=inp, output_size=num_experts * out, num_experts=num_experts,
                                        expert_func=DNNLayer, expert_inputs_size=inp, expert_output_size=out,
                                        expert_layer_sizes=deep_layer_sizes, expert_dropout_p=deep_dropout_p,
                                        expert_activation=deep_activation))

    def forward(self, emb_inputs: torch.Tensor) -> torch.Tensor:
        x = _plain(emb_inputs)
        for moe in self.module:
            x = _plain(moe(x))                                         # (B, 1, num_experts * out)
        return x.sum(dim=2)

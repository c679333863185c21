"""Drop-in index -> embedding input modules (same class names, constructor / forward signatures,
output names and ``state_dict`` keys as ``torecsys.inputs.base``), running on libtrs_hip.so.

Reference: torecsys/inputs/base/{__init__,single_index_emb,multi_indices_emb,
multi_indices_field_aware_emb}.py and torecsys/inputs/inputs.py.  Class ``__name__``s are kept
identical because ``Inputs.forward`` dispatches on them (inputs.py:70,84).
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import Dict, List, Optional, Union

import torch
import torch.nn as nn

from . import functional as F_


def _strip(t: torch.Tensor) -> torch.Tensor:
    return t.rename(None) if t.has_names() else t


def _check_embedding_kwargs(kwargs: dict):
    # nn.Embedding options the HIP path does not implement are rejected instead of silently ignored
    if kwargs.get("max_norm") is not None:
        raise NotImplementedError("torecsys_amd: nn.Embedding(max_norm=...) is not supported")
    if kwargs.get("scale_grad_by_freq"):
        raise NotImplementedError("torecsys_amd: nn.Embedding(scale_grad_by_freq=True) is not supported")
    if kwargs.get("sparse"):
        raise NotImplementedError("torecsys_amd: nn.Embedding(sparse=True) is not supported (dense gradient only)")


def field_offsets(field_sizes: List[int]) -> torch.Tensor:
    """(N,) int64 row offsets ``(0, *cumsum(field_sizes)[:-1])`` -- multi_indices_emb.py:54.
    Computed in int64 (the reference goes through float32 and is exact only below 2**24 rows)."""
    sizes = torch.as_tensor(list(field_sizes), dtype=torch.int64)
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)[:-1]])


# What ``MultiIndicesEmbedding(fuse_fm=None)`` resolves to at construction.  ``torecsys_amd.patch(torecsys)`` switches it
# on, so that models built from the reference's own classes run the fused lookup + FM kernel without naming it.
DEFAULT_FUSE_FM = False


class BaseInput(nn.Module):
    """inputs/base/__init__.py:11-45."""

    def __init__(self):
        super().__init__()
        self.schema = None
        self.fused_optimizer = None

    def set_fused_optimizer(self, opt):
        """Apply ``opt`` (torecsys_amd.optim.FusedSparse{SGD,Adagrad,RowWiseAdagrad,Adam}) to this module's table rows inside
        the backward pass: no dense gradient is produced, ``weight.grad`` stays None.  Returns self."""
        self.fused_optimizer = opt
        return self

    def __len__(self) -> int:
        return self.length

    def set_schema(self, inputs: Union[str, List[str]], **kwargs):
        if isinstance(inputs, str):
            inputs = [inputs]
        schema = namedtuple('Schema', ['inputs'])
        self.schema = schema(inputs=inputs)


class SingleIndexEmbedding(BaseInput):
    """single_index_emb.py:14-59: (B,1)|(B,N) any-int indices -> (B,N,E) named ('B','N','E')."""

    def __init__(self, embed_size: int, field_size: int, padding_idx: Optional[int] = None,
                 nn_embedding: Optional[nn.Parameter] = None, **kwargs):
        super().__init__()
        _check_embedding_kwargs(kwargs)
        if nn_embedding is not None:
            embed_size = nn_embedding.size('E') if nn_embedding.has_names() else nn_embedding.size(-1)
            self.embedding = nn.Embedding.from_pretrained(_strip(nn_embedding))
        else:
            self.embedding = nn.Embedding(field_size, embed_size, padding_idx=padding_idx, **kwargs)
        self.length = embed_size

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        out = F_.gather_rows(self.embedding.weight, inputs, None, self.embedding.padding_idx, self.fused_optimizer)
        out.names = ('B', 'N', 'E',)
        return out


class MultiIndicesEmbedding(BaseInput):
    """multi_indices_emb.py:18-112: one ``sum(field_sizes) x E`` table, per-field offsets,
    (B,N) -> (B,N,E) (or (B,1,N*E) when ``flatten``).

    ``offsets`` is a non-persistent buffer (same ``state_dict`` as the reference -- only
    ``embedding.weight`` -- but it follows ``.to()``).  With ``fuse_fm=True`` (``None`` = the package
    default ``DEFAULT_FUSE_FM``, which ``torecsys_amd.patch()`` turns on) the lookup
    kernel also produces the FM second-order term of the same rows and leaves it on the returned tensor
    for ``FactorizationMachineLayer`` to pick up (one pass over the rows instead of two); ``fuse_ipn=True`` does the
    same for ``InnerProductNetworkLayer`` (bf16 tables the matrix-core pair kernel covers; plain lookup otherwise)."""

    def __init__(self, embed_size: Optional[int] = None, field_sizes: Optional[List[int]] = None,
                 nn_embedding: Optional[nn.Parameter] = None, device: str = 'cpu',
                 flatten: Optional[bool] = False, fuse_fm: Optional[bool] = None, fuse_ipn: bool = False, **kwargs):
        super().__init__()
        _check_embedding_kwargs(kwargs)
        if nn_embedding is not None:
            self.embedding = nn.Embedding.from_pretrained(_strip(nn_embedding))
        elif field_sizes is not None and embed_size is not None:
            self.embedding = nn.Embedding(sum(field_sizes), embed_size, **kwargs)
        else:
            raise ValueError('missing required arguments')
        if field_sizes is None:
            raise ValueError('missing required arguments')
        self.register_buffer('offsets', field_offsets(field_sizes), persistent=False)
        self.flatten = flatten
        # the package default never overrides an explicit request for the fused inner-product lookup, and skips one-wide
        # tables (the first-order ``feat_inputs`` of the CTR models: nobody consumes an FM term of theirs)
        self.fuse_fm = ((DEFAULT_FUSE_FM and not fuse_ipn and self.embedding.embedding_dim > 1) if fuse_fm is None
                        else bool(fuse_fm))
        self.fuse_ipn = fuse_ipn
        self.field_size = self.embedding.num_embeddings
        self.embed_size = self.embedding.embedding_dim
        self.padding_idx = self.embedding.padding_idx
        self.length = self.embed_size * len(field_sizes) if self.flatten else self.embed_size
        self.to(device)

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        idx = _strip(inputs)
        if idx.dim() != 2 or idx.shape[1] != self.offsets.numel():
            raise ValueError(f'inputs must be (B, {self.offsets.numel()}), got {tuple(idx.shape)}')
        if self.fuse_fm and not self.flatten:
            out, fm, _ = F_.embed_fm(self.embedding.weight, idx, self.offsets, opt=self.fused_optimizer,
                                     padding_idx=self.padding_idx)
            out._trs_fused_fm = (fm, out._version)
        elif (self.fuse_ipn and not self.flatten and self.padding_idx is None
              and F_.embed_ipn_supported(self.embedding.weight, idx.shape[1])):
            out, ipn = F_.embed_ipn(self.embedding.weight, idx, self.offsets, opt=self.fused_optimizer)
            out._trs_fused_ipn = (ipn, out._version)
        else:
            out = F_.gather_rows(self.embedding.weight, idx, self.offsets, self.padding_idx, self.fused_optimizer)
        if self.flatten:
            out = out.reshape(out.shape[0], 1, -1)
        out.names = ('B', 'N', 'E',)
        return out


class MultiIndicesFieldAwareEmbedding(BaseInput):
    """multi_indices_field_aware_emb.py:24-111: N tables (xavier-uniform), (B,N) -> (B,N*N,E);
    row i*N+j = table i looked up with field j's index."""

    def __init__(self, embed_size: int, field_sizes: List[int], device: str = 'cpu',
                 flatten: Optional[bool] = False):
        super().__init__()
        self.num_fields = len(field_sizes)
        self.embeddings = nn.ModuleList([
            nn.Embedding(sum(field_sizes), embed_size) for _ in range(self.num_fields)
        ])
        for embedding in self.embeddings:
            nn.init.xavier_uniform_(embedding.weight.data)
        self.register_buffer('offsets', field_offsets(field_sizes), persistent=False)
        self.flatten = flatten
        self.length = embed_size
        self.to(device)

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        idx = _strip(inputs)
        if idx.dim() != 2 or idx.shape[1] != self.num_fields:
            raise ValueError(f'inputs must be (B, {self.num_fields}), got {tuple(idx.shape)}')
        out = F_.fa_gather_rows([e.weight for e in self.embeddings], idx, self.offsets)
        if self.flatten:
            out = out.reshape(out.shape[0], 1, -1)
        out.names = ('B', 'N', 'E',)
        return out


# TRS_ATTN_POOL=0: ListIndicesEmbedding(use_attn=True) keeps the gather + nn.MultiheadAttention + pooling composition
# (the A/B baseline of functional.attn_pool_layer)
ATTN_POOL = os.environ.get("TRS_ATTN_POOL", "1") not in ("", "0")


def _no_attention(query, key, value):
    return query, None


class ListIndicesEmbedding(BaseInput):
    """list_indices_emb.py:12-161: a padded (B,L) list of ids -> one table -> one pooled row per sample, (B,1,E) named
    ('B','N','E') (``output_method='none'``: the plain (B,L,E) lookup).  Same constructor, defaults (``padding_idx=0``),
    attributes and ``state_dict`` keys as the reference.

    ``avg_pooling`` / ``max_pooling`` run as one HIP pass over the looked-up rows (``functional.bag_pool``): the
    (B,L,E) block of the reference is never formed, forward or backward.  By default every list position counts, padding
    included (the padding row is read like any other row, as the reference does).

    ``exclude_padding=True`` (not in the reference; needs a ``padding_idx``) pools like ``nn.EmbeddingBag(padding_idx=)``:
    positions that hold the padding id are not read and take no part -- the mean is over the live positions of the
    sample, the maximum cannot be the padding row's, a list of nothing but padding gives a zero row.
    ``forward(inputs, per_sample_weights)`` with ``output_method='sum'`` weights every id of the list (a (B,L) tensor of the
    table's dtype, which may require grad); ``set_schema(inputs, weights='column')`` lets ``Inputs`` hand that column
    over.  Neither option changes names, shape or ``state_dict`` keys; neither is served together with ``use_attn=True``
    (NotImplementedError) or ``output_method='none'`` (ValueError).

    Deliberate difference: ``output_method='mean'`` and ``'sum'`` RAISE in the reference (it strips the tensor names and
    then reduces over ``dim='N'``); here they do what its docstring promises -- ``mean`` equals ``avg_pooling``, ``sum``
    is the unscaled sum, both (B,1,E).

    ``use_attn=True`` with ``avg_pooling`` / ``mean`` / ``sum``: self-attention over the bag followed by the pooling runs
    as one HIP pass per direction (``functional.attn_pool_layer``, csrc/attn_pool.hip): the pooling collapses the value
    and output projections onto one row per sample and head, so neither the (B,L,E) block nor Q, K, V or the scores are
    formed in the forward.  Same parameters and ``state_dict`` keys as the reference (the module's own
    ``nn.MultiheadAttention`` holds them).  Served for 1 <= L <= 64, E <= 128, fp32 / bf16, no ``add_bias_kv`` /
    ``add_zero_attn``, attention dropout 0 or eval mode, and the switch ``TRS_ATTN_POOL`` not ``0``; every other case --
    ``max_pooling`` and ``none`` with attention among them -- runs as the HIP gather to (B,L,E), ``nn.MultiheadAttention``
    (ATen) on (L,B,E) and the pooling in ATen.  ``show_attention`` (a plotting helper) is not provided."""

    _POOL = {'avg_pooling': 'mean', 'max_pooling': 'max', 'mean': 'mean', 'sum': 'sum'}

    def _attn_pool_mode(self, idx: torch.Tensor) -> Optional[str]:
        """the pooling mode when this call takes the fused attention-pooling kernel, None when it keeps the composition"""
        pool = self._POOL.get(self.output_method)
        if not ATTN_POOL or not self.use_attn or pool not in ('mean', 'sum') or idx.shape[1] < 1:
            return None
        a = self.attention
        if (a.bias_k is not None or a.bias_v is not None or a.add_zero_attn or not a._qkv_same_embed_dim
                or (a.dropout > 0.0 and self.training)):
            return None
        w = self.embedding.weight
        if not w.is_cuda or a.in_proj_weight.dtype != w.dtype:
            return None
        return pool if F_.attn_pool_path(idx.shape[1], self.embed_size, a.num_heads, w.dtype) != 0 else None

    def __init__(self, embed_size: Optional[int] = None, field_size: Optional[int] = None,
                 padding_idx: Optional[int] = 0, nn_embedding: Optional[nn.Parameter] = None,
                 use_attn: Optional[bool] = False, output_method: Optional[str] = 'avg_pooling',
                 exclude_padding: bool = False, **kwargs):
        super().__init__()
        if nn_embedding is not None:
            self.embedding = nn.Embedding.from_pretrained(_strip(nn_embedding))
        elif field_size is not None and embed_size is not None:
            self.embedding = nn.Embedding(field_size, embed_size, padding_idx=padding_idx)
        else:
            raise ValueError('missing required arguments')
        self.field_size = self.embedding.num_embeddings
        self.embed_size = self.embedding.embedding_dim
        self.padding_idx = self.embedding.padding_idx
        self.length = self.embed_size
        self.use_attn = use_attn
        if self.use_attn:
            self.attn_args = {
                'embed_dim': self.embed_size,
                'num_heads': kwargs.get('num_heads', 1),
                'dropout': kwargs.get('dropout', 0.0),
                'bias': kwargs.get('bias', True),
                'add_bias_kv': kwargs.get('add_bias_kv', False),
                'add_zero_attn': kwargs.get('add_zero_attn', False)
            }
            self.attention = nn.MultiheadAttention(**self.attn_args)
        else:
            self.attention = _no_attention
        if output_method not in ('avg_pooling', 'max_pooling', 'mean', 'none', 'sum'):
            raise ValueError('output_method only allows ["avg_pooling", "max_pooling", "mean", "none", "sum"].')
        self.output_method = output_method
        self.exclude_padding = bool(exclude_padding)
        if self.exclude_padding:
            if self.padding_idx is None:
                raise ValueError('exclude_padding=True needs a padding_idx (nn_embedding= tables have none)')
            self._check_masked_options('exclude_padding=True')

    def _check_masked_options(self, what: str):
        if self.use_attn:
            raise NotImplementedError(f'torecsys_amd: {what} with use_attn=True is not implemented (the attention '
                                      f'kernels take no key-padding mask)')
        if self.output_method == 'none':
            raise ValueError(f"{what} needs a pooling output_method, not 'none'")

    def set_schema(self, inputs: Union[str, List[str]], **kwargs):
        """``weights='column'``: ``Inputs.forward`` hands that column to ``forward`` as ``per_sample_weights``."""
        weights = kwargs.get('weights', None)
        if weights is None:
            return super().set_schema(inputs)
        if not isinstance(weights, str):
            raise TypeError(f'weights must be a column name, got {type(weights).__name__}')
        schema = namedtuple('Schema', ['inputs', 'weights'])
        self.schema = schema(inputs=[inputs] if isinstance(inputs, str) else inputs, weights=weights)

    def set_fused_optimizer(self, opt):
        if opt is not None and self.output_method == 'max_pooling' and not self.use_attn:
            raise NotImplementedError('torecsys_amd: max_pooling with a fused sparse optimizer is not implemented')
        if opt is not None and getattr(self.schema, 'weights', None) is not None:
            raise NotImplementedError('torecsys_amd: per_sample_weights with a fused sparse optimizer is not implemented')
        return super().set_fused_optimizer(opt)

    def forward(self, inputs: torch.Tensor, per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        idx = _strip(inputs)
        if idx.dim() != 2:
            raise ValueError(f'inputs must be (B, L), got {tuple(idx.shape)}')
        w = self.embedding.weight
        if self.exclude_padding or per_sample_weights is not None:
            if per_sample_weights is not None:
                self._check_masked_options('per_sample_weights')
            out = F_.bag_pool(w, idx, self._POOL[self.output_method], self.padding_idx, self.fused_optimizer,
                              exclude_padding=self.exclude_padding, per_sample_weights=per_sample_weights)
            return out.refine_names('B', 'N', 'E')
        mode = self._attn_pool_mode(idx)
        if mode is not None:
            a = self.attention
            out = F_.attn_pool_layer(w, idx, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
                                     a.num_heads, mode, self.padding_idx, self.fused_optimizer)
        elif self.use_attn or self.output_method == 'none':
            out = F_.gather_rows(w, idx, None, self.padding_idx, self.fused_optimizer)      # (B,L,E)
            if self.use_attn:
                seq = out.transpose(0, 1)                                                   # (L,B,E)
                seq, _ = self.attention(seq, seq, seq)
                out = seq.transpose(0, 1)
                pool = self._POOL.get(self.output_method)
                if pool == 'max':
                    out = out.max(dim=1, keepdim=True)[0]
                elif pool == 'mean':
                    out = out.mean(dim=1, keepdim=True)
                elif pool == 'sum':
                    out = out.sum(dim=1, keepdim=True)
        else:
            out = F_.bag_pool(w, idx, self._POOL[self.output_method], self.padding_idx, self.fused_optimizer)
        return out.refine_names('B', 'N', 'E')

    def show_attention(self, inputs: torch.Tensor, save_dir: Optional[str] = None):
        raise NotImplementedError('torecsys_amd: show_attention (a plotting helper) is not provided')


class RaggedListIndicesEmbedding(BaseInput):
    """``ListIndicesEmbedding`` for bags that arrive the way ``nn.EmbeddingBag`` takes them (not in the reference): one
    flat vector of ids (n,) and ``offsets`` that say where each sample's bag begins, instead of a (B,L) list padded to the
    longest bag.  ``forward(values, offsets, per_sample_weights=None)`` -> (B,1,E) named ('B','N','E'), one HIP pass
    (``functional.bag_pool_ragged``): bags of any length, empty ones (a zero row) included; no bag length is read on the
    host.  With ``include_last_offset=True`` the last offset closes the last bag and B = len(offsets) - 1.

    ``output_method``: 'avg_pooling' / 'mean' (over the bag's own length), 'max_pooling', 'sum' (the only one that takes
    ``per_sample_weights`` (n,)).  ``exclude_padding=True`` leaves the ids equal to ``padding_idx`` out, as
    ``nn.EmbeddingBag(padding_idx=)`` does.  The table is ``embedding.weight``, so a ``ListIndicesEmbedding`` checkpoint
    loads.  Not offered: ``output_method='none'``, a fused sparse optimizer (NotImplementedError).
    ``set_schema(inputs, offsets='column', weights=None)`` names the columns ``Inputs`` hands over.

    ``use_attn=True`` (with ``max_length``, and ``num_heads`` / ``dropout`` / ``bias`` for the module's own
    ``nn.MultiheadAttention``): self-attention over the bag's OWN ids followed by the mean / sum over them, one HIP pass
    per direction (``functional.attn_pool_ragged_layer``, csrc/attn_pool.hip).  No padding exists, so nothing but the
    bag's ids takes part in the softmax -- with ``exclude_padding=True`` the ids equal to ``padding_idx`` are removed
    first -- and the work is proportional to the bags' own lengths.  ``max_length`` (1..64) sizes the kernels' working set
    and caps a bag: the first ``max_length`` live ids are taken and a longer bag raises the index flag
    (``functional.index_errors_seen()``); an empty bag is a zero row.  Parameters and ``state_dict`` keys are those of
    ``ListIndicesEmbedding(use_attn=True)``, so checkpoints load either way.  There is no composition fallback: E > 128,
    another dtype than fp32 / bf16, attention parameters of another dtype than the table, or attention dropout in
    training mode raise NotImplementedError; ``max_pooling`` and ``per_sample_weights`` with attention raise
    ValueError."""

    _POOL = ListIndicesEmbedding._POOL

    def __init__(self, embed_size: Optional[int] = None, field_size: Optional[int] = None,
                 padding_idx: Optional[int] = 0, nn_embedding: Optional[nn.Parameter] = None,
                 output_method: Optional[str] = 'avg_pooling', exclude_padding: bool = False,
                 include_last_offset: bool = False, use_attn: bool = False, max_length: Optional[int] = None,
                 num_heads: int = 1, dropout: float = 0.0, bias: bool = True):
        super().__init__()
        if nn_embedding is not None:
            self.embedding = nn.Embedding.from_pretrained(_strip(nn_embedding))
        elif field_size is not None and embed_size is not None:
            self.embedding = nn.Embedding(field_size, embed_size, padding_idx=padding_idx)
        else:
            raise ValueError('missing required arguments')
        self.field_size = self.embedding.num_embeddings
        self.embed_size = self.embedding.embedding_dim
        self.padding_idx = self.embedding.padding_idx
        self.length = self.embed_size
        if output_method not in self._POOL:
            raise ValueError(f'output_method only allows {sorted(self._POOL)}.')
        self.output_method = output_method
        self.use_attn = bool(use_attn)
        self.max_length = None
        if self.use_attn:
            if max_length is None or not 1 <= int(max_length) <= 64:
                raise ValueError(f'use_attn=True needs max_length in [1, 64], got {max_length!r}')
            if self._POOL[output_method] == 'max':
                raise ValueError("use_attn=True pools with 'avg_pooling' / 'mean' / 'sum', not 'max_pooling'")
            self.max_length = int(max_length)
            self.attention = nn.MultiheadAttention(embed_dim=self.embed_size, num_heads=num_heads, dropout=dropout,
                                                   bias=bias)
        self.exclude_padding = bool(exclude_padding)
        if self.exclude_padding and self.padding_idx is None:
            raise ValueError('exclude_padding=True needs a padding_idx (nn_embedding= tables have none)')
        self.include_last_offset = bool(include_last_offset)

    def set_schema(self, inputs: Union[str, List[str]], **kwargs):
        """``offsets='column'`` (required) and ``weights='column'``: ``Inputs.forward`` hands those columns to
        ``forward`` as ``offsets`` and ``per_sample_weights``."""
        offsets, weights = kwargs.get('offsets', None), kwargs.get('weights', None)
        if not isinstance(offsets, str):
            raise TypeError(f'offsets must be a column name, got {type(offsets).__name__}')
        if weights is not None and not isinstance(weights, str):
            raise TypeError(f'weights must be a column name, got {type(weights).__name__}')
        schema = namedtuple('Schema', ['inputs', 'offsets', 'weights'])
        self.schema = schema(inputs=[inputs] if isinstance(inputs, str) else inputs, offsets=offsets, weights=weights)

    def set_fused_optimizer(self, opt):
        if opt is not None:
            raise NotImplementedError('torecsys_amd: ragged bags with a fused sparse optimizer are not implemented (the '
                                      'fused-update walks find the sample of a lookup by dividing its position by the '
                                      'list length)')
        return super().set_fused_optimizer(opt)

    def forward(self, values: torch.Tensor, offsets: torch.Tensor,
                per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.use_attn:
            return self._forward_attn(values, offsets, per_sample_weights)
        out = F_.bag_pool_ragged(self.embedding.weight, _strip(values), _strip(offsets), self._POOL[self.output_method],
                                 self.padding_idx, exclude_padding=self.exclude_padding,
                                 per_sample_weights=per_sample_weights, include_last_offset=self.include_last_offset,
                                 opt=self.fused_optimizer)
        return out.refine_names('B', 'N', 'E')

    def _forward_attn(self, values, offsets, per_sample_weights):
        if per_sample_weights is not None:
            raise ValueError('per_sample_weights is not served with use_attn=True')
        a, w = self.attention, self.embedding.weight
        if a.dropout > 0.0 and self.training:
            raise NotImplementedError('torecsys_amd: attention dropout in training mode is not implemented for ragged '
                                      'bags (use dropout=0.0 or eval mode)')
        if a.in_proj_weight.dtype != w.dtype:
            raise NotImplementedError(f'torecsys_amd: the attention parameters ({a.in_proj_weight.dtype}) must have the '
                                      f"table's dtype ({w.dtype})")
        if F_.attn_pool_path(self.max_length, self.embed_size, a.num_heads, w.dtype) == 0:
            raise NotImplementedError(f'torecsys_amd: attention pooling of ragged bags does not cover E={self.embed_size}, '
                                      f'H={a.num_heads}, {w.dtype} (E <= 128, fp32 / bf16)')
        out = F_.attn_pool_ragged_layer(w, _strip(values), _strip(offsets), a.in_proj_weight, a.in_proj_bias,
                                        a.out_proj.weight, a.out_proj.bias, a.num_heads, self._POOL[self.output_method],
                                        self.padding_idx, max_length=self.max_length,
                                        exclude_padding=self.exclude_padding,
                                        include_last_offset=self.include_last_offset)
        return out.refine_names('B', 'N', 'E')


class RaggedMultiListIndicesEmbedding(BaseInput):
    """F multi-valued fields (tags, categories, recent items, ..) that share one ``sum(field_sizes) x E`` table, pooled to
    the (B,F,E) block named ('B','N','E') in ONE HIP pass (``functional.bag_pool_fields``, csrc/bag_fields.hip) -- what
    ``MultiIndicesEmbedding`` is to ``SingleIndexEmbedding``, for ``RaggedListIndicesEmbedding`` (not in the reference).
    The input is the "keyed jagged" layout of feature pipelines: ``forward(values, offsets, per_sample_weights=None)`` with
    ``values`` (n,) RAW per-field ids and ``offsets`` (F*B + 1,) FIELD-MAJOR -- bag f*B + b is
    values[offsets[f*B+b]:offsets[f*B+b+1]], the last entry closes the last bag.  out[b,f] pools field f's bag of sample
    b over the rows ``values + field offset``; bags of any length, empty ones (a zero row) included; no bag length is read
    on the host.  An id outside its own field reads as a zero row and raises the index flag
    (``functional.index_errors_seen()``): it never reads a neighbouring field's row.

    ``output_method``: 'avg_pooling' / 'mean' (over the bag's own length), 'max_pooling', 'sum' (the only one that takes
    ``per_sample_weights`` (n,)).  ``embedding.weight`` is the only ``state_dict`` key; ``offsets`` -- the (F+1,) prefix
    sum of the field sizes -- is a non-persistent buffer that follows ``.to()``, as in ``MultiIndicesEmbedding``.
    ``len(module)`` is F.  Not offered: a padding id, attention, ``output_method='none'``, a fused sparse optimizer
    (NotImplementedError).  ``set_schema(inputs, offsets='column', weights=None)`` names the columns ``Inputs`` hands
    over."""

    _POOL = ListIndicesEmbedding._POOL

    def __init__(self, embed_size: Optional[int] = None, field_sizes: Optional[List[int]] = None,
                 nn_embedding: Optional[nn.Parameter] = None, output_method: Optional[str] = 'avg_pooling'):
        super().__init__()
        if field_sizes is None or len(field_sizes) < 1 or any(int(s) < 1 for s in field_sizes):
            raise ValueError('field_sizes must name at least one field, each of at least one row')
        if nn_embedding is not None:
            self.embedding = nn.Embedding.from_pretrained(_strip(nn_embedding))
            if self.embedding.num_embeddings != sum(field_sizes):
                raise ValueError(f'nn_embedding has {self.embedding.num_embeddings} rows, field_sizes sum to '
                                 f'{sum(field_sizes)}')
        elif embed_size is not None:
            self.embedding = nn.Embedding(sum(field_sizes), embed_size)
        else:
            raise ValueError('missing required arguments')
        sizes = torch.as_tensor([int(s) for s in field_sizes], dtype=torch.int64)
        self.register_buffer('offsets', torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)]),
                             persistent=False)
        self.field_sizes = [int(s) for s in field_sizes]
        self.num_fields = len(self.field_sizes)
        self.field_size = self.embedding.num_embeddings
        self.embed_size = self.embedding.embedding_dim
        self.length = self.num_fields
        if output_method not in self._POOL:
            raise ValueError(f'output_method only allows {sorted(self._POOL)}.')
        self.output_method = output_method

    set_schema = RaggedListIndicesEmbedding.set_schema

    def set_fused_optimizer(self, opt):
        if opt is not None:
            raise NotImplementedError('torecsys_amd: ragged bags with a fused sparse optimizer are not implemented (the '
                                      'fused-update walks find the sample of a lookup by dividing its position by the '
                                      'list length)')
        return super().set_fused_optimizer(opt)

    def forward(self, values: torch.Tensor, offsets: torch.Tensor,
                per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = F_.bag_pool_fields(self.embedding.weight, _strip(values), _strip(offsets), self.offsets,
                                 self._POOL[self.output_method], per_sample_weights=per_sample_weights)
        return out.refine_names('B', 'N', 'E')


# TRS_SEQ_RNN=0: SequenceIndicesEmbedding runs the composition (HIP row gather, the module's own nn.LSTM / nn.GRU / nn.RNN
# on a packed sequence, ATen pooling) instead of the fused kernels, which are the default on the strength of the timing in
# profiles/seq_rnn_kernels.md (forward + backward 4.4x to 5.5x faster at the workload shape)
SEQ_RNN_FUSED = os.environ.get("TRS_SEQ_RNN", "1") not in ("", "0")


class SequenceIndicesEmbedding(BaseInput):
    """sequence_indices_emb.py:11-171: an ordered, padded (B, L) list of ids and its (B,) lengths -> embedding rows ->
    one-layer LSTM / GRU / RNN over the first ``lengths[b]`` steps -> pooling, named ('B','N','E').  Constructor
    signature, attributes (``length``, ``embedding``, ``rnn_layers``, ``output_method``) and ``state_dict`` keys
    (``embedding.weight``, ``rnn_layers.{weight,bias}_{ih,hh}_l0``) are the reference's: the module holds a real
    ``nn.LSTM`` / ``nn.GRU`` / ``nn.RNN``, so a reference checkpoint loads.  The reference hands ``num_layers``, ``bias``,
    ``bidirectional`` and ``dropout`` on to ``nn.Embedding``, which raises TypeError for each of them; so do they here --
    every instance is one layer, one direction, with biases and hidden size ``embed_size``.

    ``output_method``:
      'avg_pooling'  (B, 1, E): the sum of h_t over t < lengths[b], divided by max(lengths) of the BATCH (what the
                     reference's pooling over the pad_packed_sequence output computes; not L, not the sample's own length).
                     The fused path: one kernel, no sort, no packing, no host read of the lengths -- capturable in a graph.
      'mean', 'sum'  raise RuntimeError in the reference (dim='N' on an un-named tensor); here 'mean' is 'avg_pooling' and
                     'sum' the unscaled sum -- a deliberate difference, the same one ListIndicesEmbedding documents.
      'none'         (B, max(lengths), E), zeros from each sample's length on; one host read of max(lengths), as in the
                     reference.
      'max_pooling'  the reference tests ``in ['avg_pooling' or 'max_pooling']``, i.e. ``in ['avg_pooling']``, so this
                     method falls into the other branch and AdaptiveMaxPool1d(1) runs over the LAST dim of (B, L', E):
                     the result is (B, max(lengths), 1), the maximum over E.  Kept as it is (every h_t from the kernel,
                     then an ATen amax), since that is what a model built on the reference was trained with.
    ``TRS_SEQ_RNN=0`` and every cell / shape / dtype ``functional.seq_rnn_path`` refuses run the composition: HIP row
    gather, ``rnn_layers`` on a packed sequence, ATen pooling (the fused path is the default by the timing in
    profiles/seq_rnn_kernels.md).  A length <= 0 raises
    there (pack_padded_sequence), as in the reference; the fused path treats it as an empty sequence (zero row) and
    raises the index flag.  A fused sparse optimizer is not implemented for this class: the walk would have to tell the
    positions past a sample's length, which touch no row, from real lookups."""

    _CELLS = {'rnn': nn.RNN, 'lstm': nn.LSTM, 'gru': nn.GRU}
    _RNN_KWARGS = ('num_layers', 'bias', 'bidirectional', 'dropout')

    def __init__(self, embed_size: int, field_size: int, padding_idx: Optional[int] = 0,
                 rnn_method: Optional[str] = 'lstm', output_method: Optional[str] = 'avg_pooling',
                 nn_embedding: Optional[nn.Parameter] = None, **kwargs):
        super().__init__()
        for k in self._RNN_KWARGS:
            if k in kwargs:
                raise TypeError(f"Embedding.__init__() got an unexpected keyword argument '{k}' (the reference passes its "
                                f"RNN kwargs on to nn.Embedding: one layer, one direction, with biases is all there is)")
        _check_embedding_kwargs(kwargs)
        if nn_embedding is not None:
            embed_size = nn_embedding.size('E') if nn_embedding.has_names() else nn_embedding.size(-1)
            self.embedding = nn.Embedding.from_pretrained(_strip(nn_embedding))
        else:
            self.embedding = nn.Embedding(field_size, embed_size, padding_idx=padding_idx, **kwargs)
        self.length = embed_size
        self.padding_idx = self.embedding.padding_idx
        if rnn_method not in self._CELLS:
            raise ValueError('rnn_method only allows ["rnn", "lstm", "gru"].')
        self.rnn_method = rnn_method
        self.rnn_layers = self._CELLS[rnn_method](input_size=embed_size, hidden_size=embed_size, num_layers=1, bias=True,
                                                  batch_first=True, dropout=0.0, bidirectional=False)
        if output_method not in ('avg_pooling', 'max_pooling', 'mean', 'none', 'sum'):
            raise ValueError('output_method only allows ["avg_pooling", "max_pooling", "mean", "none", "sum"].')
        self.output_method = output_method

    def set_fused_optimizer(self, opt):
        if opt is not None:
            raise NotImplementedError('torecsys_amd: a fused sparse optimizer is not implemented for '
                                      'SequenceIndicesEmbedding (positions past a sample\'s length would count as touched '
                                      'rows); use a dense optimizer')
        return super().set_fused_optimizer(opt)

    def set_schema(self, inputs: str, **kwargs):
        lengths = kwargs.get('lengths', None)
        if lengths is None:
            raise ValueError('')
        schema = namedtuple('Schema', ['inputs', 'lengths'])
        self.schema = schema(inputs=[inputs], lengths=lengths)

    def _rnn_params(self):
        r = self.rnn_layers
        return r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0

    def _fused(self, idx: torch.Tensor) -> bool:
        w = self.embedding.weight
        if not (SEQ_RNN_FUSED and w.is_cuda and idx.shape[1] >= 1):
            return False
        if any(p.dtype != w.dtype or p.device != w.device for p in self._rnn_params()):
            return False
        return F_.seq_rnn_path(self.rnn_method, idx.shape[1], w.shape[1], w.dtype) != 0

    def forward(self, inputs: torch.Tensor, lengths: torch.Tensor) -> torch.Tensor:
        idx, lens = _strip(inputs), _strip(lengths)
        if idx.dim() != 2:
            raise ValueError(f'inputs must be (B, L), got {tuple(idx.shape)}')
        if lens.dim() != 1 or lens.shape[0] != idx.shape[0]:
            raise ValueError(f'lengths must be ({idx.shape[0]},), got {tuple(lens.shape)}')
        w, method = self.embedding.weight, self.output_method
        if self._fused(idx):
            mode = {'avg_pooling': 'avg', 'mean': 'avg', 'sum': 'sum'}.get(method, 'none')
            out = F_.seq_rnn(w, idx, lens, *self._rnn_params(), cell=self.rnn_method, mode=mode,
                             padding_idx=self.padding_idx)
            if mode == 'none':
                longest = min(max(int(lens.max()), 0), idx.shape[1]) if lens.numel() else 0      # the one host read
                out = out[:, :longest]
        else:
            rows = F_.gather_rows(w, idx, None, self.padding_idx)                                 # (B, L, E)
            packed = nn.utils.rnn.pack_padded_sequence(rows, lens.cpu(), batch_first=True, enforce_sorted=False)
            seq, _ = self.rnn_layers(packed)
            out, _ = nn.utils.rnn.pad_packed_sequence(seq, batch_first=True)                      # (B, max(lengths), E)
            if method in ('avg_pooling', 'mean'):
                out = out.mean(dim=1, keepdim=True)
            elif method == 'sum':
                out = out.sum(dim=1, keepdim=True)
        if method == 'max_pooling':
            out = out.amax(dim=2, keepdim=True)
        return out.refine_names('B', 'N', 'E')


class ValueInput(BaseInput):
    """inputs/base/value_inp.py:26-44 (pass-through; no kernel)."""

    def __init__(self, num_fields: int, transforms=None):
        super().__init__()
        self.num_fields = num_fields
        self.transforms = transforms
        self.length = 1

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        inputs = _strip(inputs)
        if inputs.dim() == 2:
            inputs = inputs.unsqueeze(dim=-1)
        if self.transforms:
            inputs = self.transforms(inputs)
        inputs.names = ('B', 'N', 'E',)
        return inputs


# TRS_PAIR_FIRST_ORDER=1: Inputs serves the E = 1 first-order table of an FM-family model from the wide table's lookup
# kernel and bucket walk (trs_embed_fm_fields / trs_scatter_rows_first) instead of its own two launches.  Off by default:
# measured on the DeepFM step it is a loss -- the lookup kernel goes from 133 to 162 us and the walk from 176 to 210 us
# (one more dependent 2-byte access per lookup in the two bandwidth-critical kernels) while the separate E = 1 launches
# it removes cost 17 + 28 us: 1.62 vs 1.58 ms per step, and the roofline kernel itself gets slower.
PAIR_FIRST_ORDER = os.environ.get("TRS_PAIR_FIRST_ORDER", "0") == "1"


# 0: every lookup on the caller's stream; 1: lookups beyond the first on the "lookup" side stream, enqueued BEHIND the first
# (the forward stays serial, the backward's bucket walks run side by side); 2: enqueued in FRONT of it (parallel forward)
def _on_hip(t: torch.Tensor) -> bool:
    return t.is_cuda


# a StackedInput of SingleIndexEmbeddings as ONE lookup launch over the separate tables (TRS_STACKED_ONE_LAUNCH=0: its own forward)
STACKED_ONE_LAUNCH = os.environ.get("TRS_STACKED_ONE_LAUNCH", "1") not in ("", "0")
LOOKUP_STREAMS = int(os.environ.get("TRS_LOOKUP_STREAMS", "1") or 0)
_SIDE_LOOKUPS = (SingleIndexEmbedding, MultiIndicesEmbedding, MultiIndicesFieldAwareEmbedding)


class Inputs(BaseInput):
    """Dictionary router, inputs/inputs.py:56-89: for every schema entry gather its named columns,
    ``unsqueeze`` 1-D ones, ``cat`` on dim 1 and call the embedding module.  Integer columns on the HIP device are
    packed by one kernel (trs_pack_columns) instead of N unsqueezes + a cat, and schema entries that name the same
    columns (the E=64 and the E=1 table of one model) receive the SAME index tensor, so the row buckets of the batch
    are built once."""

    def __init__(self, schema: Union[Dict[str, nn.Module], None]):
        super().__init__()
        self.schema = schema if schema is not None else {}
        for k, emb_fn in self.schema.items():
            self.add_module(k, emb_fn)
        self.length = None

    def _first_order_partner(self, key: str) -> Optional[str]:
        """The schema entry whose lookup can ride in ``key``'s kernels: ``key`` is a fuse_fm MultiIndicesEmbedding and
        the partner a MultiIndicesEmbedding(embed_size=1) over the same columns and the same per-field row layout (the
        E-wide table and the first-order weights of one FM-family model).  Decided per call: fused optimizers, dtypes
        and devices can change between steps."""
        a = self.schema[key]
        if not PAIR_FIRST_ORDER:
            return None
        if type(a) is not MultiIndicesEmbedding or not a.fuse_fm or a.flatten or a.padding_idx is not None:
            return None
        if getattr(a, 'fused_optimizer', None) is not None or not a.embedding.weight.is_cuda:
            return None
        wa = a.embedding.weight
        if (wa.shape[1] * wa.element_size()) % 16 != 0:
            return None
        for k, f in self.schema.items():
            if k == key or type(f) is not MultiIndicesEmbedding:
                continue
            if (f.embed_size != 1 or f.flatten or f.fuse_fm or f.padding_idx is not None
                    or getattr(f, 'fused_optimizer', None) is not None):
                continue
            wf = f.embedding.weight
            if (tuple(f.schema.inputs) != tuple(a.schema.inputs) or wf.shape[0] != wa.shape[0] or wf.dtype != wa.dtype
                    or wf.device != wa.device or wf.requires_grad != wa.requires_grad):
                continue
            same = self._same_layout.get((key, k))
            if same is None:      # one device comparison per pair and process (the offsets are construction-time buffers)
                same = f.offsets.numel() == a.offsets.numel() and bool(torch.equal(f.offsets, a.offsets))
                self._same_layout[(key, k)] = same
            if same:
                return k
        return None

    @staticmethod
    def _stacked_single_index_tables(stacked, inputs):
        """(children, their index columns) when ``stacked`` is a StackedInput whose inputs are all plain
        SingleIndexEmbeddings of this package -- one column each, one embed size / dtype / HIP device, no padding row, no
        fused optimizer -- i.e. when F_.gather_rows_tables computes exactly what its forward computes; else None."""
        children = getattr(stacked, 'inputs', None)
        if stacked.__class__.__name__ != 'StackedInput' or not isinstance(children, (list, tuple)) or len(children) < 2:
            return None
        w0 = getattr(getattr(children[0], 'embedding', None), 'weight', None)
        if w0 is None or not _on_hip(w0):
            return None
        raw = []
        for c in children:
            if type(c) is not SingleIndexEmbedding or c.schema is None or len(c.schema.inputs) != 1:
                return None
            w = c.embedding.weight
            if (c.embedding.padding_idx is not None or c.fused_optimizer is not None or w.shape[1] != w0.shape[1]
                    or w.dtype != w0.dtype or w.device != w0.device or not w.is_contiguous()
                    or ((w.shape[1] * w.element_size()) % 16 == 0 and w.data_ptr() % 16 != 0)):
                return None            # (a 16-byte-misaligned table, e.g. a view into a larger buffer: per-child lookups)
            v = inputs[c.schema.inputs[0]]
            v = v.rename(None) if v.has_names() else v
            if v.is_floating_point() or v.device != w0.device or not (v.dim() == 1 or (v.dim() == 2 and v.shape[1] == 1)):
                return None
            raw.append(v)
        if len({v.shape[0] for v in raw}) != 1 or len({v.dtype for v in raw}) != 1 or raw[0].dtype not in (torch.int64, torch.int32):
            return None
        return list(children), raw

    def forward(self, inputs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        outputs = {}
        packed = {}                    # tuple of column names -> packed tensor (shared between schema entries)
        if not hasattr(self, '_same_layout'):
            self._same_layout = {}
        partner = {}                   # first-order entry -> the wide entry that computes it
        for k in self.schema:
            p = self._first_order_partner(k)
            if p is not None and p not in partner:
                partner[p] = k
        # pass 1: every entry's index tensor (column packing runs on the caller's stream, once per column set)
        args = {}
        for k, emb_fn in self.schema.items():
            if k in partner and partner[k] in self.schema:
                continue               # a first-order table served by its partner's pass
            if emb_fn.__class__.__name__ in ['ConcatInput', 'StackedInput']:
                stacked = self._stacked_single_index_tables(emb_fn, inputs) if STACKED_ONE_LAUNCH else None
                if stacked is not None:
                    # N SingleIndexEmbeddings under a StackedInput (stacked_inp.py:94-134: N lookups + a cat, and N
                    # bucket builds + walks in the backward): one lookup launch over the N separate tables, one walk
                    children, raw = stacked
                    names = tuple(c.schema.inputs[0] for c in children)
                    idx = packed.get(names)
                    if idx is None:
                        if F_.pack_columns_supported(raw):
                            idx = F_.pack_columns(raw)
                        else:
                            idx = torch.cat([v.unsqueeze(-1) if v.dim() == 1 else v for v in raw], dim=1)
                        packed[names] = idx
                    out = F_.gather_rows_tables([c.embedding.weight for c in children], idx)
                    out.names = ('B', 'N', 'E',)
                    outputs[k] = out
                    continue
                args[k] = [{i: inputs[i] for i in emb_fn.schema.inputs}]
                continue
            names = tuple(emb_fn.schema.inputs)
            inp = packed.get(names)
            if inp is None:
                raw = [inputs[emb_k] for emb_k in names]
                if F_.pack_columns_supported(raw):
                    inp = F_.pack_columns(raw)
                else:
                    cols = [v.unsqueeze(-1) if v.dim() == 1 else v for v in raw]
                    inp = cols[0] if len(cols) == 1 else torch.cat(cols, dim=1)
                packed[names] = inp
            args[k] = [inp]
            # inputs.py:84 asks for 'SequenceIndexEmbedding', a class the reference does not have (its class is
            # SequenceIndicesEmbedding, which therefore never receives its lengths there); both names are routed here
            if emb_fn.__class__.__name__ in ('SequenceIndicesEmbedding', 'SequenceIndexEmbedding'):
                args[k].append(inputs[emb_fn.schema.lengths])
            elif emb_fn.__class__.__name__ in ('RaggedListIndicesEmbedding', 'RaggedMultiListIndicesEmbedding'):
                # (n,) ids: their offsets, their weights
                args[k].append(inputs[emb_fn.schema.offsets])
                args[k].append(None if emb_fn.schema.weights is None else inputs[emb_fn.schema.weights])
            elif getattr(emb_fn.schema, 'weights', None) is not None:      # ListIndicesEmbedding: per_sample_weights
                args[k].append(inputs[emb_fn.schema.weights])
        # The lookups of a batch are independent of each other: every plain lookup after the first goes onto the "lookup"
        # side stream.  What pays is the BACKWARD: autograd runs a node's backward on the stream of its forward, so the
        # bucket walk of the E = 1 first-order table of an FM-family model (one walk and four small launches, ~45 us at the
        # end of the step) runs beside the dense backward instead.  In the forward the side lookup is enqueued BEHIND the
        # first one (mode 1): beside it (mode 2) the two gathers share the memory pipe and the wide lookup goes from 131 to
        # 157 us for the 17 us it hides.  Measured alternately on one box, DeepFM step: 0: 1.287 ms, 1: 1.259 ms,
        # 2: 1.304 ms (gpurun_out/r05e, r05f).
        side_keys, first_lookup = [], True
        for k in args:
            emb_fn = self.schema[k]
            plain = (type(emb_fn) in _SIDE_LOOKUPS and k not in partner.values()
                     and isinstance(args[k][0], torch.Tensor) and args[k][0].is_cuda)
            if plain and not first_lookup and LOOKUP_STREAMS:
                side_keys.append(k)
            first_lookup = first_lookup and not plain
        joins = []                     # (event, output) of lookups enqueued on the side stream
        def side_lookups():
            for k in side_keys:
                emb_fn, idx_t = self.schema[k], args[k][0]
                out, ev, side = F_.run_on_side(idx_t.device, "lookup", lambda: emb_fn(idx_t))
                idx_t.record_stream(side)
                joins.append((ev, out))
                outputs[k] = out

        with F_.defer_prefetch():      # row-bucket builds start once every lookup of the batch is enqueued
            if LOOKUP_STREAMS == 2:
                side_lookups()
            for k in args:
                if k in outputs or k in side_keys:
                    continue
                emb_fn, inp_args = self.schema[k], args[k]
                feat_key = next((f for f, w in partner.items() if w == k), None)
                if feat_key is not None:
                    # one lookup pass and one bucket walk for the wide table and its first-order companion
                    feat_fn = self.schema[feat_key]
                    idx = inp_args[0].rename(None) if inp_args[0].has_names() else inp_args[0]
                    if idx.dim() != 2 or idx.shape[1] != emb_fn.offsets.numel():
                        raise ValueError(f'inputs must be (B, {emb_fn.offsets.numel()}), got {tuple(idx.shape)}')
                    out, fm, first = F_.embed_fm_fields(emb_fn.embedding.weight, feat_fn.embedding.weight, idx,
                                                        emb_fn.offsets)
                    out._trs_fused_fm = (fm, out._version)
                    out.names = ('B', 'N', 'E',)
                    first.names = ('B', 'N', 'E',)
                    outputs[k] = out
                    outputs[feat_key] = first
                else:
                    outputs[k] = emb_fn(*inp_args)
            if LOOKUP_STREAMS != 2:
                side_lookups()
        if joins:
            main = F_._abi.current_stream_of(joins[0][1].device)
            for ev, out in joins:      # consumers are enqueued on the caller's stream: it waits for the side lookups here
                main.wait_event(ev)
                extra = [t[0] for t in (getattr(out, a, None) for a in ('_trs_fused_fm', '_trs_fused_ipn')) if t is not None]
                for t in [out] + extra:
                    (t.rename(None) if t.has_names() else t).record_stream(main)
        return {k: outputs[k] for k in self.schema}      # schema order, as the reference returns it

    def add_inputs(self, name: Optional[str] = None, model: Optional[nn.Module] = None,
                   schema: Optional[Dict[str, nn.Module]] = None):
        """Register more input fields after construction: one ``name`` -> ``model`` pair, or a whole ``schema`` dict
        (which wins when both are given).  Same contract as inputs/inputs.py:91-130: TypeError for a non-dict schema,
        a non-str name or a non-Module model; AssertionError for a name that is already routed.  Returns self."""
        if schema is None:
            entries = [(name, model)]
        elif isinstance(schema, dict):
            entries = list(schema.items())
        else:
            raise TypeError(f'schema must be a dict of name -> nn.Module, got {type(schema).__name__}')
        for key, module in entries:
            if not isinstance(key, str):
                raise TypeError(f'input field name must be a str, got {type(key).__name__}')
            if key in self.schema:
                raise AssertionError(f'input field {key!r} is already in the schema')
            if not isinstance(module, nn.Module):
                raise TypeError(f'input field {key!r} must map to an nn.Module, got {type(module).__name__}')
            self.schema[key] = module
            self.add_module(key, module)
        return self

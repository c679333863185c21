"""Row-wise int8 (Q8) embedding tables for serving: a table that is only read, stored one byte per element with an fp32
scale and bias per row -- the "fused 8-bit row-wise" layout -- and looked up by HIP kernels that dequantize in registers
(csrc/q8.hip).  Forward only: a Q8 table has no gradient and no optimizer.

The format is part of ``state_dict`` (buffer ``qweight``) and fixed in include/trs_abi.h: a table of V rows x E columns is
a contiguous uint8 (V, S) tensor, S = round_up(E + 8, 16); row = E codes, scale (fp32 LE), bias (fp32 LE), zero padding;
``x[e] = float(c[e]) * scale + bias`` in fp32, the product and the sum each rounded.  At E = 64 a row is 80 bytes against
128 for bf16.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from . import functional as F_
from ._abi import call, ptr, require_device, size_query, stream_ptr, value_dtype_code
from .fused import EmbeddingFM, EmbeddingPairScorer
from .inputs import BaseInput, MultiIndicesEmbedding, RaggedListIndicesEmbedding, _strip, field_offsets


def q8_row_bytes(E: int) -> int:
    """S, the bytes of one Q8 row of E columns: round_up(E + 8, 16)."""
    if not isinstance(E, int) or E <= 0:
        raise ValueError(f"q8_row_bytes: E must be a positive int, got {E!r}")
    return size_query("trs_q8_row_bytes", E)


def quantize_rows(weight: torch.Tensor) -> torch.Tensor:
    """(V, E) float32 / bfloat16 table on the device -> (V, S) uint8 Q8 rows.  Per row: bias = min, scale = (max - bias) /
    255, code = clamp(rint((x - bias) / scale), 0, 255); a constant row dequantizes to itself."""
    weight = _strip(weight.detach())
    if weight.dim() != 2 or weight.shape[1] == 0:
        raise ValueError(f"quantize_rows: weight must be (V, E), got shape {tuple(weight.shape)}")
    code = value_dtype_code(weight)
    dev = require_device(weight)
    V, E = weight.shape
    w = weight.contiguous()
    q = torch.empty(V, q8_row_bytes(E), dtype=torch.uint8, device=dev)
    call("trs_q8_quantize_rows", ptr(w), V, E, code, ptr(q), stream_ptr())
    return q


def dequantize_rows(qrows: torch.Tensor, E: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(V, E) of ``dtype``: every row of a Q8 table dequantized -- the lookup with idx = arange(V)."""
    V = qrows.shape[0] if qrows.dim() == 2 else 0
    idx = torch.arange(V, dtype=torch.int64, device=qrows.device).view(V, 1)
    return F_.gather_rows_q8(qrows, E, idx, None, dtype).view(V, E)


def _no_optimizer(opt):
    if opt is not None:
        raise NotImplementedError("torecsys_amd: a Q8 table is not trained: no fused sparse optimizer (quantize after "
                                  "training, or train the float module)")


def _out_dtype(out_dtype: Optional[torch.dtype], like: Optional[torch.Tensor] = None) -> torch.dtype:
    """``out_dtype``, or (from_float) the float table's dtype where it is None"""
    dt = like.dtype if out_dtype is None and like is not None else out_dtype
    if dt not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out_dtype must be float32 or bfloat16, got {dt}")
    return dt


def _empty_qweight(V: int, E: int) -> torch.Tensor:
    if V <= 0 or E <= 0:
        raise ValueError(f"a Q8 table needs V > 0 rows and E > 0 columns, got V={V}, E={E}")
    return torch.zeros(V, (E + 8 + 15) // 16 * 16, dtype=torch.uint8)


class _QuantizedInput(BaseInput):
    """What the Q8 input modules share: the persistent uint8 buffer ``qweight`` (V, S) and the optimizer refusal."""

    def _set_table(self, V: int, E: int, out_dtype: torch.dtype):
        self.register_buffer('qweight', _empty_qweight(V, E))
        self.field_size, self.embed_size = V, E
        self.out_dtype = _out_dtype(out_dtype)

    def set_fused_optimizer(self, opt):
        _no_optimizer(opt)
        return super().set_fused_optimizer(opt)


class QuantizedMultiIndicesEmbedding(_QuantizedInput):
    """``MultiIndicesEmbedding`` on a Q8 table: (B,N) indices -> (B,N,E) named ('B','N','E') of ``out_dtype``.
    ``offsets`` is the same non-persistent buffer; ``state_dict`` holds ``qweight`` only."""

    def __init__(self, embed_size: int, field_sizes: List[int], out_dtype: torch.dtype = torch.float32):
        super().__init__()
        self._set_table(sum(field_sizes), embed_size, out_dtype)
        self.register_buffer('offsets', field_offsets(field_sizes), persistent=False)
        self.length = embed_size

    @classmethod
    def from_float(cls, module: MultiIndicesEmbedding, out_dtype: Optional[torch.dtype] = None):
        if not isinstance(module, MultiIndicesEmbedding):
            raise TypeError(f"from_float needs a MultiIndicesEmbedding, got {type(module).__name__}")
        if module.flatten:
            raise NotImplementedError("torecsys_amd: QuantizedMultiIndicesEmbedding does not serve flatten=True")
        w = module.embedding.weight
        off = module.offsets
        sizes = torch.diff(torch.cat([off.cpu(), torch.tensor([w.shape[0]])])).tolist()
        q = cls(w.shape[1], sizes, _out_dtype(out_dtype, w)).to(w.device)
        q.qweight.copy_(quantize_rows(w))
        return q

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        idx = _strip(inputs)
        if idx.dim() != 2 or idx.shape[1] != self.offsets.numel():
            raise ValueError(f'inputs must be (B, {self.offsets.numel()}), got {tuple(idx.shape)}')
        out = F_.gather_rows_q8(self.qweight, self.embed_size, idx, self.offsets, self.out_dtype)
        out.names = ('B', 'N', 'E',)
        return out


class QuantizedEmbeddingFM(nn.Module):
    """``fused.EmbeddingFM`` on a Q8 table: ``forward(inputs)`` -> (emb named ('B','N','E') | None, fm named ('B','O'),
    first (B,1) | None) exactly as that module returns them.  The E = 1 first-order table stays a float buffer ``first``
    (V,) of ``out_dtype``: one value per row gains nothing from a scale and a bias of its own."""

    def __init__(self, embed_size: int, field_sizes: List[int], first_order: bool = True, want_block: bool = True,
                 out_dtype: torch.dtype = torch.float32):
        super().__init__()
        V = sum(field_sizes)
        self.register_buffer('qweight', _empty_qweight(V, embed_size))
        self.out_dtype = _out_dtype(out_dtype)
        self.register_buffer('first', torch.zeros(V, dtype=self.out_dtype) if first_order else None)
        self.register_buffer('offsets', field_offsets(field_sizes), persistent=False)
        self.embed_size = embed_size
        self.want_block = want_block

    @classmethod
    def from_float(cls, module: EmbeddingFM, out_dtype: Optional[torch.dtype] = None):
        if not isinstance(module, EmbeddingFM):
            raise TypeError(f"from_float needs a fused.EmbeddingFM, got {type(module).__name__}")
        w = module.emb.embedding.weight
        off = module.emb.offsets
        sizes = torch.diff(torch.cat([off.cpu(), torch.tensor([w.shape[0]])])).tolist()
        q = cls(w.shape[1], sizes, module.feat is not None, module.want_block, _out_dtype(out_dtype, w)).to(w.device)
        q.qweight.copy_(quantize_rows(w))
        if module.feat is not None:
            q.first.copy_(module.feat.embedding.weight.detach().reshape(-1))
        return q

    def set_fused_optimizer(self, opt):
        _no_optimizer(opt)
        return self

    def forward(self, inputs: torch.Tensor):
        emb, fm, first = F_.embed_fm_q8(self.qweight, self.embed_size, _strip(inputs), self.offsets, self.first,
                                        self.want_block, self.out_dtype)
        if emb is not None:
            emb.names = ('B', 'N', 'E',)
        fm.names = ('B', 'O',)
        return emb, fm, first


class QuantizedEmbeddingPairScorer(nn.Module):
    """``fused.EmbeddingPairScorer`` for serving on Q8 tables.  Buffers (persistent): ``qweight``, the target table or the
    one shared table, and ``anchor_qweight``, the anchor table where it is a separate one.  ``topk`` is the retrieval
    kernel over the Q8 rows (functional.topk_scores_q8) and ``rank`` the position of held-out targets among them
    (functional.target_ranks_q8); the anchors are dequantized per batch into ``out_dtype``."""

    def __init__(self, embed_size: int, anchor_size: int, target_size: Optional[int] = None, similarity: str = 'dot',
                 anchor_offset: int = 0, target_offset: int = 0, out_dtype: torch.dtype = torch.float32):
        super().__init__()
        if similarity not in F_.PAIR_SIMS:
            raise ValueError(f"similarity must be one of {sorted(F_.PAIR_SIMS)}, got {similarity!r}")
        self.register_buffer('qweight', _empty_qweight(anchor_size if target_size is None else target_size, embed_size))
        self.register_buffer('anchor_qweight', None if target_size is None else _empty_qweight(anchor_size, embed_size))
        self.embed_size = embed_size
        self.similarity = similarity
        self.anchor_offset, self.target_offset = int(anchor_offset), int(target_offset)
        self.out_dtype = _out_dtype(out_dtype)

    @classmethod
    def from_float(cls, module: EmbeddingPairScorer, out_dtype: Optional[torch.dtype] = None):
        if not isinstance(module, EmbeddingPairScorer):
            raise TypeError(f"from_float needs a fused.EmbeddingPairScorer, got {type(module).__name__}")
        aw = module.anchor.weight
        tw = None if module.target is None else module.target.weight
        q = cls(aw.shape[1], aw.shape[0], None if tw is None else tw.shape[0], module.similarity, module.anchor_offset,
                module.target_offset, _out_dtype(out_dtype, aw)).to(aw.device)
        q.qweight.copy_(quantize_rows(aw if tw is None else tw))
        if tw is not None:
            q.anchor_qweight.copy_(quantize_rows(aw))
        return q

    def set_fused_optimizer(self, opt):
        _no_optimizer(opt)
        return self

    def _anchors(self, anchor_idx: torch.Tensor) -> torch.Tensor:
        """(B, E) of ``out_dtype``: the anchors' dequantized rows"""
        aq = self.qweight if self.anchor_qweight is None else self.anchor_qweight
        idx = _strip(anchor_idx).reshape(-1, 1) + self.anchor_offset
        return F_.gather_rows_q8(aq, self.embed_size, idx, None, self.out_dtype).view(-1, self.embed_size)

    def topk(self, anchor_idx: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None):
        """``EmbeddingPairScorer.topk`` on the Q8 target rows: ``(values (B, k) fp32, ids (B, k) int64)``.  A shared table
        is searched from ``target_offset`` to its end."""
        return F_.topk_scores_q8(self._anchors(anchor_idx), None, self.qweight, self.embed_size, k,
                                 target_lo=self.target_offset, sim=self.similarity, exclude=exclude)

    def rank(self, anchor_idx: torch.Tensor, positive_idx: torch.Tensor, exclude: Optional[torch.Tensor] = None):
        """``EmbeddingPairScorer.rank`` on the Q8 target rows (functional.target_ranks_q8): ``(ranks (B, P) int64,
        label_scores (B, P) fp32)``, the index ``topk`` with the same ``exclude`` would return each id at, were k unbounded;
        ``torecsys_amd.metrics`` takes it as it is.  A shared table is ranked from ``target_offset`` to its end."""
        return F_.target_ranks_q8(self._anchors(anchor_idx), None, self.qweight, self.embed_size, positive_idx,
                                  target_lo=self.target_offset, sim=self.similarity, exclude=exclude)

    def forward(self, anchor_idx: torch.Tensor, target_idx: torch.Tensor) -> torch.Tensor:
        """(B, 1 + K) scores of given pairs.  Not a kernel: a plain composition, both sides dequantized by
        ``gather_rows_q8`` and a batched product (or cosine, eps 1e-8 on each norm) in ATen, fp32."""
        t_idx = _strip(target_idx)
        t_idx = (t_idx.unsqueeze(1) if t_idx.dim() == 1 else t_idx) + self.target_offset
        a = self._anchors(anchor_idx).float().unsqueeze(1)
        t = F_.gather_rows_q8(self.qweight, self.embed_size, t_idx, None, self.out_dtype).float()
        s = (a * t).sum(-1)
        if self.similarity == 'cosine':
            s = s / (a.norm(dim=-1).clamp_min(1e-8) * t.norm(dim=-1).clamp_min(1e-8))
        return s


class QuantizedRaggedListIndicesEmbedding(_QuantizedInput):
    """``RaggedListIndicesEmbedding`` with sum or mean pooling on a Q8 table: ``forward(values, offsets)`` -> (B,1,E) named
    ('B','N','E') of ``out_dtype``; ``include_last_offset``, ``exclude_padding`` (with ``padding_idx``) and ``set_schema``
    as in that module.  Not served: attention, max pooling, per-sample weights."""

    _POOL = {k: v for k, v in RaggedListIndicesEmbedding._POOL.items() if v in ('sum', 'mean')}

    def __init__(self, embed_size: int, field_size: int, padding_idx: Optional[int] = 0,
                 output_method: str = 'avg_pooling', exclude_padding: bool = False, include_last_offset: bool = False,
                 out_dtype: torch.dtype = torch.float32):
        super().__init__()
        if RaggedListIndicesEmbedding._POOL.get(output_method) == 'max':
            raise NotImplementedError("torecsys_amd: max pooling is not served on Q8 tables")
        if output_method not in self._POOL:
            raise ValueError(f'output_method only allows {sorted(self._POOL)}.')
        self._set_table(field_size, embed_size, out_dtype)
        self.length = embed_size
        self.output_method = output_method
        self.padding_idx = padding_idx
        self.exclude_padding = bool(exclude_padding)
        if self.exclude_padding and padding_idx is None:
            raise ValueError('exclude_padding=True needs a padding_idx')
        self.include_last_offset = bool(include_last_offset)

    set_schema = RaggedListIndicesEmbedding.set_schema

    @classmethod
    def from_float(cls, module: RaggedListIndicesEmbedding, out_dtype: Optional[torch.dtype] = None):
        if not isinstance(module, RaggedListIndicesEmbedding):
            raise TypeError(f"from_float needs a RaggedListIndicesEmbedding, got {type(module).__name__}")
        if module.use_attn:
            raise NotImplementedError("torecsys_amd: attention pooling (use_attn=True) is not served on Q8 tables")
        w = module.embedding.weight
        q = cls(w.shape[1], w.shape[0], module.padding_idx, module.output_method, module.exclude_padding,
                module.include_last_offset, _out_dtype(out_dtype, w)).to(w.device)
        q.qweight.copy_(quantize_rows(w))
        return q

    def forward(self, values: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        out = F_.bag_pool_ragged_q8(self.qweight, self.embed_size, _strip(values), _strip(offsets),
                                    self._POOL[self.output_method], self.padding_idx,
                                    exclude_padding=self.exclude_padding, include_last_offset=self.include_last_offset,
                                    out_dtype=self.out_dtype)
        return out.refine_names('B', 'N', 'E')

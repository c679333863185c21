"""Functional layer: torch.autograd.Functions whose forward/backward are calls into libtrs_hip.so.

Every function takes and returns UN-NAMED tensors on one HIP device (the nn.Modules in
``inputs.py`` / ``layers.py`` strip and re-apply the reference's tensor names).  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Tuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _abi
from ._abi import call, index_dtype_code, ptr, require_device, size_query, stream_ptr, value_dtype_code

CHECK_INDICES = os.environ.get("TRS_CHECK_INDICES", "0") not in ("", "0")


def _as_index(idx: torch.Tensor) -> torch.Tensor:
    """Indices are consumed as int64 or int32 directly (the reference's ``.long()`` /
    int64-promotion happens inside the kernel); other int dtypes are widened here."""
    idx = idx.rename(None) if idx.has_names() else idx
    if idx.dtype not in (torch.int64, torch.int32):
        if idx.dtype.is_floating_point or idx.dtype == torch.bool:
            raise TypeError(f"indices must be an integer tensor, got {idx.dtype}")
        idx = idx.long()
    return idx.contiguous()


_lazy_flags = {}          # device -> persistent int32[1]: "some lookup was out of range" (never read unless asked)


class _ErrFlag:
    """Out-of-range flag of one lookup.  The kernels range-check every row id when they are handed a flag (an
    out-of-range lookup then reads as a zero row and contributes no gradient instead of touching foreign memory).
    With TRS_CHECK_INDICES=1 the flag is private to the call and read back at once (IndexError, like nn.Embedding);
    otherwise the calls share one persistent flag per device that nobody waits for -- ``index_errors_seen()`` reads it."""

    def __init__(self, dev):
        if CHECK_INDICES:
            self.t, self.lazy = torch.zeros(1, dtype=torch.int32, device=dev), False
        else:
            t = _lazy_flags.get(dev)
            if t is None:
                t = _lazy_flags[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
            self.t, self.lazy = t, True

    def check(self, what):
        if not self.lazy and int(self.t.item()) != 0:
            raise IndexError(f"{what}: index out of range in self")


def index_errors_seen(device=None, reset: bool = True) -> bool:
    """True when a lookup since the last call had a row id outside its table (synchronises).  Only meaningful without
    TRS_CHECK_INDICES=1 (which raises at the offending call instead)."""
    seen = False
    for dev, t in list(_lazy_flags.items()):
        if device is not None and torch.device(device) != dev:
            continue
        if int(t.item()) != 0:
            seen = True
            if reset:
                t.zero_()
    return seen


# --------------------------------------------------------------------------------------------
# Row-bucketed index of one batch (CSR over destination rows), shared by every table looked up
# with the same index tensor (E=64 embeddings and the E=1 first-order weights).
# --------------------------------------------------------------------------------------------
class RowBuckets:
    __slots__ = ("row_start", "perm", "V", "BN", "N", "ready", "stream")

    def __init__(self, row_start, perm, V, BN, N):
        self.row_start, self.perm, self.V, self.BN, self.N = row_start, perm, V, BN, N
        self.ready = None        # event recorded behind the build on the stream it ran on
        self.stream = None       # that stream (side-stream prefetch or the consumer's own stream for an inline build)

    def built_on(self, stream):
        """Record where the build was enqueued: every consumer on ANOTHER stream (the E = 1 table's walk on the "lookup"
        stream sharing the wide table's entry, or the other way round) waits for the event first."""
        self.stream = stream
        self.ready = torch.cuda.Event()
        self.ready.record(stream)

    def wait(self):
        """Make the current stream wait for the build (no-op when built on this stream)."""
        if self.ready is None:
            return
        cur = _abi.current_stream_of(self.row_start.device)
        if self.stream is not None and cur == self.stream:
            return
        cur.wait_event(self.ready)
        self.row_start.record_stream(cur)
        self.perm.record_stream(cur)


_bucket_cache: List[tuple] = []   # [(key, idx_tensor_kept_alive, RowBuckets)]
_BUCKET_CACHE_SIZE = 2
_side_streams = {}
PREFETCH_BUCKETS = os.environ.get("TRS_PREFETCH_BUCKETS", "1") not in ("", "0")
# priority of the side stream the row buckets are built on (HIP: larger number = lower priority)
SIDE_STREAM_PRIORITY = int(os.environ.get("TRS_SIDE_STREAM_PRIORITY", "0"))
# TRS_PREFETCH_EARLY=1: start the bucket build BEFORE the fused lookup launch (beside the HBM-bound lookup instead of beside
# the first MLP GEMM)
PREFETCH_EARLY = os.environ.get("TRS_PREFETCH_EARLY", "0") not in ("", "0")


def side_stream(dev: torch.device, role: str) -> torch.cuda.Stream:
    """The per-device side stream of a ROLE: "buckets" (row-bucket builds, beside the dense forward), "lookup" (the
    lookups of a batch beyond the first, beside it -- and, because autograd runs a node's backward on its forward's stream,
    their bucket walks beside the first one's).  One stream per role: work of one role must never queue behind another's
    (a lookup behind a bucket build would stall the main stream for the whole build)."""
    side = _side_streams.get((dev, role))
    if side is None:
        side = _side_streams[(dev, role)] = torch.cuda.Stream(device=dev, priority=SIDE_STREAM_PRIORITY)
    return side


def run_on_side(dev: torch.device, role: str, fn):
    """Enqueue ``fn()`` on the role's side stream behind everything the current stream holds so far; returns (result,
    event recorded behind it, the side stream).  The caller makes the consumer's stream wait for the event and tells the
    allocator about tensors that cross (record_stream).  Capture-safe: the side stream forks from the current stream and
    the event wait joins it again."""
    side = side_stream(dev, role)
    main = _abi.current_stream_of(dev)
    side.wait_stream(main)
    torch.cuda.set_stream(side)      # (not ``with torch.cuda.stream``: see prefetch_row_buckets)
    try:
        out = fn()
    finally:
        torch.cuda.set_stream(main)
    ev = torch.cuda.Event()
    ev.record(side)
    return out, ev, side


def _adopt_grads(*grads):
    """A lookup's backward runs on the stream of its forward -- the "lookup" side stream for every lookup of a batch but the
    first -- while the gradients it receives were allocated (and will be freed) under the producer's stream: tell the
    allocator.  No-op until a side lookup has happened."""
    for g in grads:
        if g is not None and g.is_cuda and (g.device, "lookup") in _side_streams:
            cur = _abi.current_stream_of(g.device)
            (g.rename(None) if g.has_names() else g).record_stream(cur)


_offsets_content = {}     # offsets tensor (ptr, version) -> tuple of its values (read back once)


def _offsets_key(offsets):
    """Content key of a per-field offsets vector, so two modules built from the same field sizes (the E=64
    table and the E=1 first-order table of one model) share the row buckets of a batch."""
    if offsets is None:
        return None
    k = (offsets.data_ptr(), offsets._version, offsets.numel())
    v = _offsets_content.get(k)
    if v is None:
        if len(_offsets_content) > 256:
            _offsets_content.clear()
        v = _offsets_content[k] = tuple(offsets.tolist())
    return v


def _bucket_key(idx, offsets, V, check=True, skip_row=None):
    # ``check`` is part of the key: a build that skipped out-of-range ids silently (fixed-capacity padding) must not be
    # handed to a caller that expects the index flag to have been raised for them, nor the other way round
    return (idx.data_ptr(), idx._version, tuple(idx.shape), idx.dtype, _offsets_key(offsets), V, bool(check), skip_row)


def _build_buckets(idx, offsets, V, check: bool = True, skip_row: Optional[int] = None) -> RowBuckets:
    """``check=False``: ids outside [0, V) are skipped WITHOUT raising the index flag (the padding slots of a
    fixed-capacity exchange carry -1; real ids were range-checked when they were looked up).  ``skip_row``: the lookups
    of that row are left out of the index (trs_csr_build_skip: the padding id of a list field, which no walk reads)."""
    B, N = idx.shape
    BN = B * N
    dev = idx.device
    row_start = torch.empty(V + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(max(BN, 1), dtype=torch.int32, device=dev)
    ws_bytes = size_query("trs_csr_workspace_bytes", V, BN)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    flag = _ErrFlag(dev) if check else None
    if skip_row is None:
        call("trs_csr_build", ptr(idx), index_dtype_code(idx), ptr(offsets), B, N, V, ptr(row_start), ptr(perm),
             ptr(ws), ws_bytes, ptr(flag.t if check else None), stream_ptr())
    else:
        call("trs_csr_build_skip", ptr(idx), index_dtype_code(idx), ptr(offsets), B, N, V, int(skip_row), ptr(row_start),
             ptr(perm), ptr(ws), ws_bytes, ptr(flag.t if check else None), stream_ptr())
    if check:
        flag.check("row_buckets")
    return RowBuckets(row_start, perm, V, BN, N)


def row_buckets(idx: torch.Tensor, offsets: Optional[torch.Tensor], V: int, check: bool = True,
                skip_row: Optional[int] = None) -> RowBuckets:
    """Build (or fetch) the CSR for ``idx`` (B,N).  The cache keeps a reference to the index tensor,
    so its storage cannot be recycled for another batch while the entry is live; in-place edits bump
    ``_version`` and miss."""
    key = _bucket_key(idx, offsets, V, check, skip_row)
    for k, _, rb in _bucket_cache:
        if k == key:
            rb.wait()
            return rb
    rb = _build_buckets(idx, offsets, V, check, skip_row)
    # an inline build is shared like a prefetched one (two tables looked up with the same indices, possibly on two
    # streams): it carries its event and stream too
    rb.built_on(_abi.current_stream_of(idx.device))
    _bucket_cache.append((key, idx, rb))
    if len(_bucket_cache) > _BUCKET_CACHE_SIZE:
        _bucket_cache.pop(0)
    return rb


_pending_prefetch: List[tuple] = []
_defer_depth = [0]


class defer_prefetch:
    """Context manager: bucket prefetches requested inside are launched when the block exits.  ``Inputs.forward``
    wraps its loop over the embedding modules with it, so the (atomics-heavy) bucket build starts after ALL
    lookups of the batch have been enqueued and overlaps the dense part of the model instead of the lookups."""

    def __enter__(self):
        _defer_depth[0] += 1
        return self

    def __exit__(self, *exc):
        _defer_depth[0] -= 1
        if _defer_depth[0] == 0:
            reqs = list(_pending_prefetch)
            _pending_prefetch.clear()
            for idx, offsets, V, check, skip_row in reqs:
                prefetch_row_buckets(idx, offsets, V, check, skip_row=skip_row)
        return False


def prefetch_row_buckets(idx: torch.Tensor, offsets: Optional[torch.Tensor], V: int, check: bool = True,
                         now: bool = False, skip_row: Optional[int] = None) -> None:
    """Start building the CSR of this batch on a side stream at FORWARD time: it depends only on the
    indices, is latency-bound (int32 atomics), and hides behind the forward/backward of the dense part
    of the model; the backward's scatter then just waits on an event."""
    if not PREFETCH_BUCKETS:
        return
    if _defer_depth[0] > 0 and not now:
        _pending_prefetch.append((idx, offsets, V, check, skip_row))
        return
    key = _bucket_key(idx, offsets, V, check, skip_row)
    for k, _, _rb in _bucket_cache:
        if k == key:
            return
    dev = idx.device
    side = side_stream(dev, "buckets")
    main = _abi.current_stream_of(dev)
    side.wait_stream(main)
    torch.cuda.set_stream(side)          # not `with torch.cuda.stream(side)`: its constructor and __enter__ each resolve
    try:                                 # the current device through hipGetDeviceCount (~0.1 ms apiece)
        rb = _build_buckets(idx, offsets, V, check, skip_row)
        rb.built_on(side)
    finally:
        torch.cuda.set_stream(main)
    idx.record_stream(side)
    if offsets is not None:
        offsets.record_stream(side)
    _bucket_cache.append((key, idx, rb))
    if len(_bucket_cache) > _BUCKET_CACHE_SIZE:
        _bucket_cache.pop(0)


_clear_hooks: List = []        # other per-batch caches keyed by index-tensor identity (dist.py's route plans)


def clear_caches():
    _bucket_cache.clear()
    _fields_map_cache.clear()
    for hook in _clear_hooks:
        hook()


# --------------------------------------------------------------------------------------------
# N2: index staging -- per-field columns -> one (B, N) index matrix
# --------------------------------------------------------------------------------------------
def pack_columns_supported(cols: Sequence[torch.Tensor]) -> bool:
    """One-pass packing applies to >= 2 integer (int64 / int32, one dtype) contiguous HIP tensors of shape (B,) or
    (B, k) with the same B whose total width fits the kernel's tile."""
    if len(cols) < 2:
        return False
    c0 = cols[0]
    if not c0.is_cuda or c0.dtype not in (torch.int64, torch.int32) or c0.dim() not in (1, 2):
        return False
    W = 0
    for c in cols:
        if (not c.is_cuda or c.device != c0.device or c.dtype != c0.dtype or c.dim() not in (1, 2)
                or c.shape[0] != c0.shape[0] or not c.is_contiguous() or c.has_names()):
            return False
        W += 1 if c.dim() == 1 else c.shape[1]
    return 0 < W <= (127 if c0.dtype == torch.int64 else 255)


def pack_columns(cols: Sequence[torch.Tensor], out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``torch.cat([c.unsqueeze(-1) if c.dim() == 1 else c for c in cols], dim=1)`` in one kernel
    (inputs/inputs.py:75-80); ``out_dtype=torch.int32`` narrows on the way (caller guarantees the range)."""
    if not pack_columns_supported(cols):
        raise ValueError("pack_columns: need >= 2 contiguous int64/int32 HIP tensors of shape (B,) or (B,k), same B")
    c0 = cols[0]
    B = c0.shape[0]
    widths = [1 if c.dim() == 1 else int(c.shape[1]) for c in cols]
    out_dtype = out_dtype or c0.dtype
    if out_dtype not in (torch.int64, torch.int32):
        raise TypeError(f"pack_columns: out_dtype {out_dtype}")
    out = torch.empty(B, sum(widths), dtype=out_dtype, device=c0.device)
    n = len(cols)
    srcs = (ctypes.c_void_p * n)(*[c.data_ptr() for c in cols])
    wid = (ctypes.c_int32 * n)(*widths)
    call("trs_pack_columns", srcs, wid, n, index_dtype_code(c0), B, ptr(out),
         _abi.TRS_I64 if out_dtype == torch.int64 else _abi.TRS_I32, stream_ptr())
    return out


def _bcast_cols(g_bcast: Optional[torch.Tensor], E: int) -> int:
    """trs_scatter_rows' g_fm_cols: E for full (B,E) rows, 1 for one value per sample ((B,) or (B,1) with E > 1)"""
    if g_bcast is None:
        return E
    return 1 if (g_bcast.dim() == 1 or g_bcast.shape[-1] == 1) else E


def _fm_grad_operand(g_fm: torch.Tensor) -> torch.Tensor:
    """The FM gradient as trs_scatter_rows wants it: an expanded (B,1) -> (B,E) gradient (what a ``sum`` over E feeds
    back) is passed as its (B,1) column -- the kernel then reads one value per sample instead of a row of E"""
    if g_fm.dim() == 2 and g_fm.shape[1] > 1 and g_fm.stride(1) == 0:
        return g_fm[:, :1].contiguous()
    return g_fm.contiguous()


def _walk_takes_vectors(table: torch.Tensor, *operands: Optional[torch.Tensor]) -> bool:
    """trs_scatter_rows' choice of walk, restated: rows of 1, 2, 4 ... 64 whole 16-byte vectors behind 16-byte aligned
    pointers are reduced by lane groups; every other width or alignment (E = 12 fp32: three vectors; a table that is a
    misaligned view) takes the element walk -- which has no companion-table form (trs_scatter_rows_first rejects it)."""
    row_bytes = table.shape[1] * table.element_size()
    vecs = row_bytes // 16
    if row_bytes % 16 != 0 or vecs & (vecs - 1) != 0 or vecs > 64:
        return False
    return all(t is None or t.data_ptr() % 16 == 0 for t in operands)


def scatter_rows(rb: RowBuckets, like_table: torch.Tensor, g_rows: Optional[torch.Tensor] = None,
                 g_bcast: Optional[torch.Tensor] = None, fm_sum: Optional[torch.Tensor] = None,
                 padding_row: int = -1, g_rows_batch_stride: int = 0) -> torch.Tensor:
    """Dense gradient of a (V,E) table: see trs_scatter_rows in include/trs_abi.h."""
    V, E = like_table.shape
    grad = torch.empty(V, E, dtype=like_table.dtype, device=like_table.device)
    ws_bytes = size_query("trs_scatter_workspace_bytes", rb.BN, rb.N, E, value_dtype_code(like_table))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=like_table.device)
    call("trs_scatter_rows", ptr(g_rows), g_rows_batch_stride, ptr(g_bcast), _bcast_cols(g_bcast, E), ptr(fm_sum),
         ptr(like_table if fm_sum is not None else None), ptr(rb.row_start), ptr(rb.perm), rb.BN, V, E, rb.N,
         value_dtype_code(like_table), padding_row, ptr(grad), ptr(ws), ws_bytes, stream_ptr())
    return grad


def scatter_rows_first(rb: RowBuckets, like_table: torch.Tensor, like_first: torch.Tensor, g_first: torch.Tensor,
                       g_rows: Optional[torch.Tensor] = None, g_bcast: Optional[torch.Tensor] = None,
                       fm_sum: Optional[torch.Tensor] = None, padding_row: int = -1
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Dense gradients of a (V,E) table and of its first-order companion (V,1) in one bucket walk: ``g_first`` holds
    one value per lookup (B,N[,1]).  See trs_scatter_rows_first in include/trs_abi.h."""
    V, E = like_table.shape
    grad = torch.empty_like(like_table)
    gfirst = torch.empty_like(like_first)
    ws_bytes = size_query("trs_scatter_workspace_bytes", rb.BN, rb.N, E, value_dtype_code(like_table))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=like_table.device)
    call("trs_scatter_rows_first", ptr(g_rows), 0, ptr(g_bcast), _bcast_cols(g_bcast, E), ptr(fm_sum),
         ptr(like_table if fm_sum is not None else None), ptr(rb.row_start), ptr(rb.perm), rb.BN, V, E, rb.N,
         value_dtype_code(like_table), padding_row, ptr(grad), ptr(g_first), ptr(gfirst), ptr(ws), ws_bytes, stream_ptr())
    return grad, gfirst


def _adam_step_dev(opt, table: torch.Tensor, key) -> torch.Tensor:
    """capturable Adam: advance the table's device step counter and refresh its bias-corrected step size (one thread,
    trs_adam_step_size), in front of the update on the same stream; returns the step-size scalar the update reads"""
    step, step_size = opt.step_tensors(table, key)
    call("trs_adam_step_size", ptr(step), ptr(opt.lr_tensor(table.device)), float(opt.beta1), float(opt.beta2),
         ptr(step_size), stream_ptr())
    return step_size


TRS_OPT_ROWWISE = 16      # include/trs_abi.h: flag on optimizer 2, the state is one fp32 per table row


def _sink_args(opt, table: torch.Tensor, key, operands=()):
    """The optimizer tail of trs_scatter_rows_update[_mapped] up to ``state2``: (kind, lr, lr_dev, eps, beta1, beta2,
    state, state2).  A ``capturable`` optimizer hands its step size over in device memory (lr_dev; eagerly and under
    capture alike), any other by value.  For Adam this advances the table's step.  ``operands``: the tensors of the call
    whose alignment enters the library's choice of walk (what ``_walk_takes_vectors`` takes)."""
    capturable = getattr(opt, "capturable", False)
    lr, lr_dev = float(opt.lr), opt.lr_tensor(table.device) if capturable else None
    beta1 = beta2 = 0.0
    state = state2 = None
    kind = opt.kind
    if opt.kind == 3:
        if not capturable and torch.cuda.is_current_stream_capturing():
            # the bias-corrected step size lr*sqrt(1-b2^t)/(1-b1^t) is computed on the host per step and passed by
            # value: a captured launch would replay the capture-time t for ever (~0.18*lr with default betas)
            raise RuntimeError("torecsys_amd: FusedSparseAdam cannot be captured into a hipGraph (its per-step bias "
                               "correction is a host-side scalar); use FusedSparseSGD / FusedSparseAdagrad under "
                               "GraphedStep, or run the Adam step eagerly")
        state, state2 = opt.state_for(table, key)
        beta1, beta2 = float(opt.beta1), float(opt.beta2)
        if capturable:
            lr_dev = _adam_step_dev(opt, table, key)
        else:
            lr = float(opt.next_step_size(table, key))
    elif opt.kind == 2:
        if getattr(opt, "rowwise", False) and table.shape[1] != 1:
            # one accumulator per row: the lanes of a row must sit in one lane group.  (E == 1, DeepFM's first-order
            # table, always takes the element walk -- and there the rule is element-wise Adagrad on the (V,) state
            # seen as (V, 1): plain optimizer 2 below.)
            if not _walk_takes_vectors(table, table, *operands):
                raise NotImplementedError(
                    f"FusedSparseRowWiseAdagrad: a table of rows of {table.shape[1]} x {table.dtype} "
                    f"({table.shape[1] * table.element_size()} bytes; table and gradient operands 16-byte aligned: "
                    f"{all(t is None or t.data_ptr() % 16 == 0 for t in (table, *operands))}) takes "
                    "the element walk, which has no row-wise form: rows must be whole 16-byte vectors, 1..64 of them a "
                    "power of two, behind 16-byte aligned pointers")
            kind = 2 | TRS_OPT_ROWWISE
        state = opt.state_for(table, key)
    return kind, lr, ptr(lr_dev), float(opt.eps), beta1, beta2, ptr(state), ptr(state2)


def _sr_args(opt, table: torch.Tensor, key) -> tuple:
    """What the stochastic-rounding entries take behind the plain argument list -- (seed, t, t_dev) -- or () when the update
    goes to the plain entry: the option is off, or the table is fp32 (nothing to round).  Takes the table's next update
    number: by value from the host counter, or, for a ``capturable`` optimizer, from its device counter, advanced here by
    one thread (trs_sr_advance) in front of the update on the same stream.  Call it after ``_sink_args`` has accepted the
    table."""
    if not getattr(opt, "stochastic_rounding", False) or table.dtype != torch.bfloat16:
        return ()
    t, t_dev = opt.next_update(table, key)
    if t_dev is not None:
        call("trs_sr_advance", ptr(t_dev), stream_ptr())
    return opt.seed, t, ptr(t_dev)


def scatter_rows_update(rb: RowBuckets, table: torch.Tensor, opt, g_rows: Optional[torch.Tensor] = None,
                        g_bcast: Optional[torch.Tensor] = None, fm_sum: Optional[torch.Tensor] = None,
                        padding_row: int = -1, key=None, g_rows_batch_stride: int = 0) -> None:
    """Fused sparse optimizer step: the bucketed gradient of every looked-up row is applied to ``table`` in
    place (see trs_scatter_rows_update); no gradient tensor is produced.  A ``capturable`` optimizer's step size is read
    from device memory (eagerly and under capture alike).  ``g_rows_batch_stride`` as in ``scatter_rows``."""
    V, E = table.shape
    if not table.is_contiguous():
        raise ValueError("fused optimizer needs a contiguous table")
    ws_bytes = size_query("trs_scatter_workspace_bytes", rb.BN, rb.N, E, value_dtype_code(table))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=table.device)
    # (a per-sample FM gradient is read as scalars: its own alignment does not matter)
    scal = g_bcast is not None and _bcast_cols(g_bcast, E) == 1 and E > 1 and fm_sum is not None
    sink = _sink_args(opt, table, key, (g_rows, None if scal else g_bcast, fm_sum))
    sr = _sr_args(opt, table, key)
    call("trs_scatter_rows_update_sr" if sr else "trs_scatter_rows_update", ptr(g_rows), g_rows_batch_stride, ptr(g_bcast),
         _bcast_cols(g_bcast, E), ptr(fm_sum), ptr(table), ptr(rb.row_start), ptr(rb.perm), rb.BN, V, E, rb.N,
         value_dtype_code(table), padding_row, *sink, ptr(ws), ws_bytes, stream_ptr(), *sr)


def scatter_rows_update_mapped(rb: RowBuckets, table: torch.Tensor, opt, g_rows: torch.Tensor, row_map: torch.Tensor,
                               key=None):
    """Fused sparse optimizer step where the bucketed rows are a compact list of distinct table rows:
    ``rb`` buckets the K rows of ``g_rows`` by compact row u (rb.V = U), ``row_map[u]`` (int32, distinct) is the table
    row that u updates; entries outside [0, V) -- the empty slots of ``compact_rows`` -- update nothing.  See
    trs_scatter_rows_update_mapped."""
    V, E = table.shape
    if not table.is_contiguous():
        raise ValueError("fused optimizer needs a contiguous table")
    if row_map.dtype != torch.int32 or row_map.numel() != rb.V:
        raise ValueError("row_map must be int32 with one entry per bucketed row")
    ws_bytes = size_query("trs_scatter_workspace_bytes", rb.BN, 1, E, value_dtype_code(table))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=table.device)
    g_rows = g_rows.contiguous()
    sink = _sink_args(opt, table, key, (g_rows,))
    sr = _sr_args(opt, table, key)
    call("trs_scatter_rows_update_mapped_sr" if sr else "trs_scatter_rows_update_mapped", ptr(g_rows), ptr(table),
         ptr(row_map), ptr(rb.row_start), ptr(rb.perm), rb.BN, rb.V, V, E, value_dtype_code(table), *sink, ptr(ws),
         ws_bytes, stream_ptr(), *sr)


def compact_rows(ids: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Distinct rows of ``ids`` (K int32 row ids with repeats; negative = padding) without a sort or a host read:
    ``row_map`` (T + 1 int32, T = the smallest power of two >= 2K) holds every id >= 0 in exactly one slot and -1 in the
    others, ``inv`` (K int32) the slot of every position (T, whose key is -1, for negative ids).  Shapes depend on K
    alone; which slot an id gets is unspecified.  ``out``: (row_map, inv) buffers of those shapes to write into.  See
    trs_compact_rows."""
    require_device(ids)
    if ids.dtype != torch.int32:
        raise TypeError(f"compact_rows: ids must be int32, got {ids.dtype}")
    ids = ids.reshape(-1).contiguous()
    K = ids.numel()
    T = size_query("trs_compact_rows_slots", K)
    if out is not None:
        row_map, inv = out
        require_device(ids, row_map, inv)
        if (row_map.dtype != torch.int32 or inv.dtype != torch.int32 or row_map.numel() != T + 1 or inv.numel() != K
                or not row_map.is_contiguous() or not inv.is_contiguous()):
            raise ValueError(f"compact_rows: out must be contiguous int32 tensors of {T + 1} and {K} elements")
    else:
        row_map = torch.empty(T + 1, dtype=torch.int32, device=ids.device)
        inv = torch.empty(K, dtype=torch.int32, device=ids.device)
    call("trs_compact_rows", ptr(ids), K, ptr(row_map), T, ptr(inv), stream_ptr())
    return row_map, inv


def compact_rows_dense(ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``compact_rows`` with the U distinct ids numbered densely: ``dense_map`` (K + 1 int32) holds them in rows
    [0, U) and -1 behind (row K included), ``inv`` (K int32) the row of every position (K for negative ids).  The row
    space a bucket build / walk behind it covers is K + 1 instead of the T + 1 >= 2K + 1 hash slots; U is not read
    back.  See trs_compact_rows_dense."""
    require_device(ids)
    if ids.dtype != torch.int32:
        raise TypeError(f"compact_rows_dense: ids must be int32, got {ids.dtype}")
    ids = ids.reshape(-1).contiguous()
    K = ids.numel()
    dense_map = torch.empty(K + 1, dtype=torch.int32, device=ids.device)
    inv = torch.empty(K, dtype=torch.int32, device=ids.device)
    ws_bytes = size_query("trs_compact_rows_dense_workspace_bytes", K)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=ids.device)
    call("trs_compact_rows_dense", ptr(ids), K, ptr(dense_map), ptr(inv), ptr(ws), ws_bytes, stream_ptr())
    return dense_map, inv


def _apply_or_grad(rb, weight, opt, key=None, **kw):
    """dense gradient (default) or in-place fused optimizer step (returns None).  ``key``: the object the optimizer
    state is filed under -- the parameter itself when ``weight`` is a reshaped view of it (a view is a new Python object
    on every call: keyed by the view, the state would be re-created, and leaked, every step)."""
    if opt is None:
        return scatter_rows(rb, weight, **kw)
    with torch.no_grad():
        scatter_rows_update(rb, weight.data, opt, key=weight if key is None else key, **kw)
    return None


# --------------------------------------------------------------------------------------------
# K1: gather
# --------------------------------------------------------------------------------------------
class _GatherRows(Function):
    @staticmethod
    def forward(ctx, weight, idx, offsets, padding_idx, opt=None):
        require_device(weight, idx, offsets)
        B, N = idx.shape
        V, E = weight.shape
        w = weight.contiguous()
        out = torch.empty(B, N, E, dtype=w.dtype, device=w.device)
        flag = _ErrFlag(w.device)
        call("trs_gather_rows", ptr(w), V, E, value_dtype_code(w), ptr(idx), index_dtype_code(idx), ptr(offsets),
             B, N, ptr(out), ptr(flag.t), stream_ptr())
        flag.check("gather_rows")
        if ctx.needs_input_grad[0] and E * w.element_size() >= 16:      # False under torch.no_grad(): no backward, no buckets
            # (narrow tables -- the E=1 first-order weights -- leave the prefetch to the wide table that shares
            # their indices, so the bucket build overlaps the dense part of the model, not the lookups)
            prefetch_row_buckets(idx, offsets, V)
        ctx.save_for_backward(idx, offsets, weight)
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        ctx.opt = opt
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        idx, offsets, weight = ctx.saved_tensors
        _adopt_grads(g)
        rb = row_buckets(idx, offsets, weight.shape[0])
        if g.dim() == 3 and g.shape[1] > 1 and g.stride(1) == 0:
            # the same gradient row for every field of a sample (the backward of a sum over the fields, e.g. the models'
            # first-order term): read as one (B,E) row per sample instead of materialising the expanded (B,N,E) block
            grad = _apply_or_grad(rb, weight, ctx.opt, g_bcast=g[:, 0, :].contiguous(), padding_row=ctx.padding_idx)
        else:
            grad = _apply_or_grad(rb, weight, ctx.opt, g_rows=g.contiguous(), padding_row=ctx.padding_idx)
        return grad, None, None, None, None


def gather_rows(weight: torch.Tensor, idx: torch.Tensor, offsets: Optional[torch.Tensor] = None,
                padding_idx: Optional[int] = None, opt=None) -> torch.Tensor:
    """out[b,n,:] = weight[idx[b,n] + offsets[n], :]; dense-gradient backward."""
    idx = _as_index(idx)
    if idx.dim() == 1:
        idx = idx.unsqueeze(-1)
    if idx.dim() != 2:
        raise ValueError(f"indices must be (B, N), got shape {tuple(idx.shape)}")
    return _GatherRows.apply(weight, idx, offsets, _norm_padding("gather_rows", padding_idx, weight.shape[0]), opt)


# --------------------------------------------------------------------------------------------
# bag pooling: (B, L) list of ids -> one pooled row per sample
# --------------------------------------------------------------------------------------------
BAG_MODES = {"sum": 0, "mean": 1, "max": 2}


def _norm_padding(op, padding_idx, V, exclude_padding=False):
    """``padding_idx`` counted from the front; ``exclude_padding`` needs it to name a row of the table."""
    if padding_idx is not None and padding_idx < 0:
        padding_idx = V + padding_idx
    if exclude_padding:
        if padding_idx is None:
            raise ValueError(f"{op}: exclude_padding=True needs a padding_idx")
        if not 0 <= padding_idx < V:
            raise ValueError(f"{op}: exclude_padding=True needs a padding row inside the table, got {padding_idx} "
                             f"for {V} rows")
    return padding_idx


def _skip_row(padding_idx, V):
    """The padding id is left out of the row buckets: no walk reads that bucket, and filing a third or more of all
    positions under one row serialises the build (22 ms against 0.2 ms, profiles/bag_kernels.md)."""
    return padding_idx if 0 <= padding_idx < V else None


def _check_psw(op, psw, mode, weight, shape, flatten):
    """``per_sample_weights`` as the kernels read them: ``shape`` -- (B, L), or (n,) with ``flatten`` (an (n, 1) column
    is taken as (n,)) --, the table's dtype and device, ``sum`` only."""
    if psw is None:
        return None
    if mode != "sum":
        raise ValueError(f"{op}: per_sample_weights is only supported for mode='sum', got {mode!r}")
    psw = psw.rename(None) if psw.has_names() else psw
    if flatten and psw.dim() == 2 and psw.shape[1] == 1:
        psw = psw.reshape(-1)
    if tuple(psw.shape) != tuple(shape):
        raise ValueError(f"{op}: per_sample_weights must be {'(n,)' if flatten else '(B, L)'} = {tuple(shape)}, got "
                         f"{tuple(psw.shape)}")
    if psw.dtype != weight.dtype:
        raise ValueError(f"{op}: per_sample_weights must have the table's dtype {weight.dtype}, got {psw.dtype}")
    if psw.device != weight.device:
        raise ValueError(f"{op}: per_sample_weights must be on the table's device {weight.device}, got {psw.device}")
    return psw


def _save_optional(ctx, fixed, optional):
    """save_for_backward of ``fixed`` tensors and of those of ``optional`` that exist; _load_optional gives all back."""
    ctx.has = tuple(t is not None for t in optional)
    ctx.save_for_backward(*fixed, *[t for t in optional if t is not None])


def _load_optional(ctx):
    saved = list(ctx.saved_tensors)
    fixed = saved[:len(saved) - sum(ctx.has)]
    rest = saved[len(fixed):]
    return (*fixed, *[rest.pop(0) if h else None for h in ctx.has])


def _live_mean_grad(g2, inv_cnt):
    """The (bags, E) gradient as the walks read it.  Mean over the live positions (``inv_cnt`` given): times 1 / cnt[b]
    in fp32, rounded once to the table's dtype."""
    return (g2 * inv_cnt.unsqueeze(1)).to(g2.dtype) if inv_cnt is not None else g2.contiguous()


class _BagPool(Function):
    """bag_pool. Neither exclusion nor weights: trs_bag_pool_fwd, every position counts.  ``exclude_padding`` and / or
    ``per_sample_weights``: trs_bag_pool_masked_fwd.  Both build the same row buckets (padding id skipped), so the
    sum / mean / max backward are the same walks; only the scale of the mean differs (1 / L, or 1 / live count)."""

    @staticmethod
    def forward(ctx, weight, idx, psw, mode, padding_idx, exclude, opt=None):
        require_device(weight, idx, psw)
        B, L = idx.shape
        V, E = weight.shape
        w = weight.contiguous()
        wts = psw.contiguous() if psw is not None else None
        masked = exclude or wts is not None
        out = torch.empty(B, E, dtype=w.dtype, device=w.device)
        # the winning list positions, uint16 bit patterns (L <= 65535) in an int16 tensor
        amax = torch.empty(B, E, dtype=torch.int16, device=w.device) if mode == 2 else None
        # 1 / (live positions of the bag), 0 for an empty one: written by the kernel, never read back here
        inv_cnt = torch.empty(B, dtype=torch.float32, device=w.device) if masked and mode == 1 else None
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        ctx.exclude_row = ctx.padding_idx if exclude else -1
        flag = _ErrFlag(w.device)
        if masked:
            call("trs_bag_pool_masked_fwd", ptr(w), V, E, value_dtype_code(w), ptr(idx), index_dtype_code(idx), B, L,
                 mode, ctx.exclude_row, ptr(wts), ptr(out), ptr(amax), ptr(inv_cnt), ptr(flag.t), stream_ptr())
        else:
            call("trs_bag_pool_fwd", ptr(w), V, E, value_dtype_code(w), ptr(idx), index_dtype_code(idx), B, L, mode,
                 ptr(out), ptr(amax), ptr(flag.t), stream_ptr())
        flag.check("bag_pool")
        ctx.skip = _skip_row(ctx.padding_idx, V)
        if ctx.needs_input_grad[0]:
            prefetch_row_buckets(idx, None, V, skip_row=ctx.skip)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:      # else there is no backward: nothing is kept
            _save_optional(ctx, (idx, weight), (wts, amax, inv_cnt))
        ctx.mode = mode
        ctx.opt = opt
        return out.unsqueeze(1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        idx, weight, wts, amax, inv_cnt = _load_optional(ctx)
        _adopt_grads(g)
        V, E = weight.shape
        B, L = idx.shape
        g2 = g.reshape(B, E)
        grad = dw = None
        if wts is not None and ctx.needs_input_grad[2]:
            g2 = g2.contiguous()
            dw = torch.empty(B, L, dtype=wts.dtype, device=wts.device)
            call("trs_bag_weight_grad", ptr(g2), ptr(weight.contiguous()), V, E, value_dtype_code(weight), ptr(idx),
                 index_dtype_code(idx), B, L, ctx.exclude_row, ptr(dw), stream_ptr())
        if ctx.needs_input_grad[0]:
            rb = row_buckets(idx, None, V, skip_row=ctx.skip)
            if amax is not None or wts is not None:
                # max: the winner's position takes g; weighted sum: every bucketed position takes w * g
                entry, operand = ("argmax", amax) if amax is not None else ("weighted", wts)
                g2 = g2.contiguous()
                grad = torch.empty(V, E, dtype=weight.dtype, device=weight.device)
                ws_bytes = size_query(f"trs_scatter_{entry}_workspace_bytes", rb.BN, E)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=weight.device)
                call(f"trs_scatter_rows_{entry}", ptr(g2), ptr(operand), ptr(rb.row_start), ptr(rb.perm), rb.BN, V, E, L,
                     value_dtype_code(weight), ctx.padding_idx, ptr(grad), ptr(ws), ws_bytes, stream_ptr())
            else:
                # sum / mean: the per-sample gradient broadcast over the bucketed positions (mean over all L positions:
                # times 1 / L first, on (B,E))
                g2 = g2 * (1.0 / L) if ctx.mode == 1 and inv_cnt is None else _live_mean_grad(g2, inv_cnt)
                grad = _apply_or_grad(rb, weight, ctx.opt, g_bcast=g2, padding_row=ctx.padding_idx)
        return grad, None, dw, None, None, None, None


def bag_pool(weight: torch.Tensor, idx: torch.Tensor, mode: str = "mean", padding_idx: Optional[int] = None,
             opt=None, *, exclude_padding: bool = False, per_sample_weights: Optional[torch.Tensor] = None
             ) -> torch.Tensor:
    """(B,1,E) pooled rows of a padded (B,L) list of ids: ``sum`` / ``mean`` / ``max`` (first position wins a tie) in one
    pass over the looked-up rows -- the (B,L,E) block of list_indices_emb.py:124-152 is never formed.  ``padding_idx``:
    the table row that receives no gradient.  ``opt``: fused sparse optimizer (sum / mean only, not with weights).

    By default every position counts (``mean`` = sum / L) and the padding row is read like any other, as F.embedding
    does.  ``exclude_padding=True`` (needs ``padding_idx``) is nn.EmbeddingBag's ``padding_idx``: positions holding the
    padding id are not read and take no part -- sum and max over the live positions, mean over their count, an empty bag
    a zero row (max: L <= 65534).  ``per_sample_weights`` (B,L), of the table's dtype and device, ``sum`` only:
    out[b] = sum_l w[b,l] * table[idx[b,l]] over all positions, or over the live ones with ``exclude_padding``; it may
    require grad (dw[b,l] = <g[b], table[idx[b,l]]>, 0 at excluded positions)."""
    if mode not in BAG_MODES:
        raise ValueError(f'bag_pool: mode must be one of {sorted(BAG_MODES)}, got {mode!r}')
    idx = _as_index(idx)
    if idx.dim() != 2 or idx.shape[1] < 1:
        raise ValueError(f"indices must be (B, L) with L >= 1, got shape {tuple(idx.shape)}")
    if idx.shape[1] > 65535:
        raise ValueError(f"bag_pool: list length {idx.shape[1]} exceeds 65535")
    if weight.dim() != 2:
        raise ValueError(f"weight must be (V, E), got shape {tuple(weight.shape)}")
    if opt is not None and mode == "max":
        raise NotImplementedError("torecsys_amd: max pooling with a fused sparse optimizer is not implemented "
                                  "(use sum / mean pooling, or a dense optimizer)")
    padding_idx = _norm_padding("bag_pool", padding_idx, weight.shape[0], exclude_padding)
    if exclude_padding and mode == "max" and idx.shape[1] > 65534:
        raise ValueError(f"bag_pool: max pooling with exclude_padding=True: list length {idx.shape[1]} exceeds "
                         "65534 (0xFFFF marks an empty bag)")
    psw = _check_psw("bag_pool", per_sample_weights, mode, weight, idx.shape, flatten=False)
    if psw is not None and opt is not None:
        raise NotImplementedError("torecsys_amd: per_sample_weights with a fused sparse optimizer is not "
                                  "implemented (use a dense optimizer)")
    return _BagPool.apply(weight, idx, psw, BAG_MODES[mode], padding_idx, bool(exclude_padding), opt)


def bag_ragged_long_len() -> int:
    """Bags of more ids than this are reduced by a whole wave each (the second tier of trs_bag_pool_ragged_fwd)."""
    return size_query("trs_bag_ragged_long_len")


def _bag_mapped_grads(g2, weight, ids, owner, wts, amax, n, nbags, padding_row, exclude_row, check, need):
    """(table gradient, weight gradient) of bags whose lookups find their bag in a map: ``ids`` (n,) are the table rows
    looked up, ``owner`` (n,) int32 the bag of each (below zero: none; None: no lookup belongs to a bag), ``g2``
    (nbags, E) the bags' gradients (_live_mean_grad).  ``need``: which of the two is wanted; ``check``: whether the
    bucket build flags ids outside the table."""
    need_grad, need_dw = need
    V, E = weight.shape
    dev = weight.device
    grad = dw = None
    if owner is None:
        if need_grad:
            grad = torch.zeros(V, E, dtype=weight.dtype, device=dev)
        if need_dw:
            dw = torch.zeros(n, dtype=wts.dtype, device=dev)
        return grad, dw
    if need_dw:
        dw = torch.empty(n, dtype=wts.dtype, device=dev)
        call("trs_bag_weight_grad_ragged", ptr(g2), ptr(weight.contiguous()), V, E, value_dtype_code(weight), ptr(ids),
             index_dtype_code(ids), n, ptr(owner), exclude_row, ptr(dw), stream_ptr())
    if need_grad:
        rb = row_buckets(ids.view(n, 1), None, V, check=check, skip_row=_skip_row(padding_row, V))
        grad = torch.empty(V, E, dtype=weight.dtype, device=dev)
        ws_bytes = size_query("trs_scatter_ragged_workspace_bytes", n, E)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        call("trs_scatter_rows_ragged", ptr(g2), ptr(owner), ptr(wts), ptr(amax), ptr(rb.row_start), ptr(rb.perm), n,
             nbags, V, E, value_dtype_code(weight), padding_row, ptr(grad), ptr(ws), ws_bytes, stream_ptr())
    return grad, dw


class _BagPoolRagged(Function):
    """bag_pool on one flat id vector (n,) plus offsets (trs_bag_pool_ragged_fwd).  Nothing here reads a tensor back:
    the offsets are range-checked on the device and ``n`` is the shape of ``ids``.  The row buckets are those of the
    ids seen as an (n, 1) batch; the lookup -> sample map (trs_bag_owner) is built in the backward only."""

    @staticmethod
    def forward(ctx, weight, ids, offsets, psw, mode, padding_idx, exclude, B):
        require_device(weight, ids, offsets, psw)
        n = ids.shape[0]
        V, E = weight.shape
        w = weight.contiguous()
        wts = psw.contiguous() if psw is not None else None
        dev = w.device
        out = torch.empty(B, E, dtype=w.dtype, device=dev)
        amax = torch.empty(B, E, dtype=torch.int32, device=dev) if mode == 2 else None      # flat winner positions
        inv_cnt = torch.empty(B, dtype=torch.float32, device=dev) if mode == 1 else None
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        ctx.exclude_row = ctx.padding_idx if exclude else -1
        ws_bytes = size_query("trs_bag_ragged_workspace_bytes", B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        flag = _ErrFlag(dev)
        call("trs_bag_pool_ragged_fwd", ptr(w), V, E, value_dtype_code(w), ptr(ids), index_dtype_code(ids), n,
             ptr(offsets), index_dtype_code(offsets), offsets.shape[0], B, mode, ctx.exclude_row, ptr(wts), ptr(out),
             ptr(amax), ptr(inv_cnt), ptr(ws), ws_bytes, ptr(flag.t), stream_ptr())
        flag.check("bag_pool_ragged")
        if ctx.needs_input_grad[0] and n > 0 and B > 0:
            prefetch_row_buckets(ids.view(n, 1), None, V, skip_row=_skip_row(ctx.padding_idx, V))
        _save_optional(ctx, (ids, offsets, weight), (wts, amax, inv_cnt))
        ctx.B = B
        return out.unsqueeze(1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ids, offsets, weight, wts, amax, inv_cnt = _load_optional(ctx)
        _adopt_grads(g)
        n, B = ids.shape[0], ctx.B
        need = (ctx.needs_input_grad[0], wts is not None and ctx.needs_input_grad[3])
        g2 = _live_mean_grad(g.reshape(B, weight.shape[1]), inv_cnt)
        bag_of = None
        if any(need) and n > 0 and B > 0:
            bag_of = torch.empty(n, dtype=torch.int32, device=weight.device)
            call("trs_bag_owner", ptr(offsets), index_dtype_code(offsets), offsets.shape[0], B, n, ptr(bag_of),
                 stream_ptr())
        grad, dw = _bag_mapped_grads(g2, weight, ids, bag_of, wts, amax, n, B, ctx.padding_idx, ctx.exclude_row, True,
                                     need)
        return grad, None, None, dw, None, None, None, None


def bag_pool_ragged(weight: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, mode: str = "mean",
                    padding_idx: Optional[int] = None, *, exclude_padding: bool = False,
                    per_sample_weights: Optional[torch.Tensor] = None, include_last_offset: bool = False,
                    opt=None) -> torch.Tensor:
    """(B,1,E) pooled rows of RAGGED bags, nn.EmbeddingBag's calling form: ``ids`` (n,) or (n,1) is one flat vector of
    row ids, ``offsets`` (int64 / int32) says where each sample's bag begins; bag b is ids[offsets[b]:offsets[b+1]], the
    last one runs to n -- or, with ``include_last_offset=True``, B = len(offsets) - 1 and ids behind offsets[-1] belong to
    no bag.  ``sum`` / ``mean`` (over the bag's own length; an empty bag is a zero row) / ``max`` (first position wins a
    tie) in one pass: nothing is padded, no bag length is read on the host, a few very long bags are reduced by a wave
    each.  ``padding_idx``, ``exclude_padding`` and ``per_sample_weights`` (n,) mean what they mean in ``bag_pool``.

    Offsets are checked on the device: they are clamped to [0, n], and an offset outside it or a decreasing pair (that bag
    is empty) raises the index flag (``index_errors_seen()``; IndexError with TRS_CHECK_INDICES=1).  A fused sparse
    optimizer is not served."""
    if mode not in BAG_MODES:
        raise ValueError(f'bag_pool_ragged: mode must be one of {sorted(BAG_MODES)}, got {mode!r}')
    if opt is not None:
        raise NotImplementedError("torecsys_amd: ragged bags with a fused sparse optimizer are not implemented: the "
                                  "fused-update walks find the sample of a lookup by dividing its position by the list "
                                  "length, which ragged bags do not have (use a dense optimizer)")
    ids = _as_index(ids)
    if ids.dim() == 2 and ids.shape[1] == 1:
        ids = ids.reshape(-1)
    if ids.dim() != 1:
        raise ValueError(f"ids must be (n,) or (n, 1), got shape {tuple(ids.shape)}")
    offsets = _as_index(offsets)
    if offsets.dim() != 1:
        raise ValueError(f"offsets must be one-dimensional, got shape {tuple(offsets.shape)}")
    B = offsets.shape[0] - 1 if include_last_offset else offsets.shape[0]
    if B < 0:
        raise ValueError("bag_pool_ragged: include_last_offset=True needs at least one offset")
    if ids.shape[0] >= 2 ** 31 - 1:
        raise ValueError(f"bag_pool_ragged: {ids.shape[0]} ids, must be below 2^31 - 1")
    if weight.dim() != 2:
        raise ValueError(f"weight must be (V, E), got shape {tuple(weight.shape)}")
    padding_idx = _norm_padding("bag_pool_ragged", padding_idx, weight.shape[0], exclude_padding)
    psw = _check_psw("bag_pool_ragged", per_sample_weights, mode, weight, ids.shape, flatten=True)
    return _BagPoolRagged.apply(weight, ids, offsets, psw, BAG_MODES[mode], padding_idx, bool(exclude_padding), B)


_fields_map_cache: List[tuple] = []   # [(key, tensors kept alive, (out_row_of, rows))]


def _fields_map(values, offsets, field_offsets, B, F, V):
    """(out_row_of (n,) int32, rows (n,) int64) of trs_bag_owner_fields.  The last two maps are kept, keyed like the row
    buckets by the identity and version of their inputs (which the cache keeps alive) and by the stream: the same batch
    looked up again finds the same ``rows`` tensor and therefore the same row buckets, so its table gradient is summed in
    the same order -- bit for bit -- and the map is not rebuilt."""
    stream = _abi.current_stream_of(values.device)
    key = (values.data_ptr(), values._version, values.shape[0], values.dtype, offsets.data_ptr(), offsets._version,
           offsets.shape[0], offsets.dtype, field_offsets.data_ptr(), field_offsets._version, B, F, V, stream)
    for k, _, m in _fields_map_cache:
        if k == key:
            return m
    n = values.shape[0]
    out_row_of = torch.empty(n, dtype=torch.int32, device=values.device)
    rows = torch.empty(n, dtype=torch.int64, device=values.device)
    call("trs_bag_owner_fields", ptr(values), index_dtype_code(values), n, ptr(offsets), index_dtype_code(offsets),
         offsets.shape[0], B, F, V, ptr(field_offsets), ptr(out_row_of), ptr(rows), stream_ptr())
    _fields_map_cache.append((key, (values, offsets, field_offsets), (out_row_of, rows)))
    if len(_fields_map_cache) > _BUCKET_CACHE_SIZE:
        _fields_map_cache.pop(0)
    return out_row_of, rows


class _BagPoolFields(Function):
    """bag_pool_ragged over the bags of F fields of one table (trs_bag_pool_fields_fwd): one forward pass writes the
    (B, F, E) block.  The map of every position to its out row and table row (trs_bag_owner_fields) is built in the
    FORWARD when a gradient will need it, so the row buckets of the table rows can start on the side stream there; the
    gradients are the walks of _BagPoolRagged on that map.  Nothing here reads a tensor back."""

    @staticmethod
    def forward(ctx, weight, values, offsets, field_offsets, psw, mode, B, F):
        require_device(weight, values, offsets, field_offsets, psw)
        n = values.shape[0]
        V, E = weight.shape
        w = weight.contiguous()
        wts = psw.contiguous() if psw is not None else None
        dev = w.device
        FB = F * B
        out = torch.empty(FB, E, dtype=w.dtype, device=dev)
        amax = torch.empty(FB, E, dtype=torch.int32, device=dev) if mode == 2 else None      # flat winner positions
        inv_cnt = torch.empty(FB, dtype=torch.float32, device=dev) if mode == 1 else None
        ws_bytes = size_query("trs_bag_fields_workspace_bytes", FB)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        flag = _ErrFlag(dev)
        call("trs_bag_pool_fields_fwd", ptr(w), V, E, value_dtype_code(w), ptr(values), index_dtype_code(values), n,
             ptr(offsets), index_dtype_code(offsets), offsets.shape[0], B, F, ptr(field_offsets), mode, ptr(wts), ptr(out),
             ptr(amax), ptr(inv_cnt), ptr(ws), ws_bytes, ptr(flag.t), stream_ptr())
        flag.check("bag_pool_fields")
        need_dw = wts is not None and ctx.needs_input_grad[4]
        out_row_of = rows = None
        if (ctx.needs_input_grad[0] or need_dw) and n > 0 and B > 0:      # a frozen table without weights: no map
            out_row_of, rows = _fields_map(values, offsets, field_offsets, B, F, V)
            if ctx.needs_input_grad[0]:
                # rows holds -1 where no bag holds the position or the id lies outside its field (flagged by the forward):
                # the build leaves them out, and must not flag the positions behind the last bag
                prefetch_row_buckets(rows.view(n, 1), None, V, check=False)
        _save_optional(ctx, (weight,), (wts, amax, inv_cnt, out_row_of, rows))
        ctx.FB, ctx.n = FB, n
        return out.view(B, F, E)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        weight, wts, amax, inv_cnt, out_row_of, rows = _load_optional(ctx)
        _adopt_grads(g)
        need = (ctx.needs_input_grad[0], wts is not None and ctx.needs_input_grad[4])
        # the table rows are the lookup ids; there is no padding row, and the forward has flagged what the build leaves out
        g2 = _live_mean_grad(g.reshape(ctx.FB, weight.shape[1]), inv_cnt)
        grad, dw = _bag_mapped_grads(g2, weight, rows, out_row_of, wts, amax, ctx.n, ctx.FB, -1, -1, False, need)
        return grad, None, None, None, dw, None, None, None


def bag_pool_fields(weight: torch.Tensor, values: torch.Tensor, offsets: torch.Tensor, field_offsets: torch.Tensor,
                    mode: str = "mean", *, per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,F,E) pooled rows of the RAGGED bags of F multi-valued fields that share one table, in one pass: the "keyed
    jagged" layout of feature pipelines.  ``field_offsets`` (F+1,) int64, on the table's device, is the exclusive prefix
    sum of the field sizes: field f owns the table rows [field_offsets[f], field_offsets[f+1]).  ``values`` (n,) or (n,1)
    holds RAW per-field ids; ``offsets`` (F*B + 1,) int64 / int32 is FIELD-MAJOR: bag j = f*B + b is
    values[offsets[j]:offsets[j+1]], the last entry closes the last bag and values behind it belong to no bag.
    out[b,f] = ``sum`` / ``mean`` (over the bag's own length; an empty bag is a zero row) / ``max`` (first position wins a
    tie) of table[values[p] + field_offsets[f]] -- what F calls of ``bag_pool_ragged`` on the fields' table slices and a
    ``cat`` give, bit for bit, without the F passes and the copy.  ``per_sample_weights`` (n,), of the table's dtype,
    ``sum`` only; it may require grad.

    An id is checked against its own field: one outside [0, field size) reads as a zero row, raises the index flag
    (``index_errors_seen()``; IndexError with TRS_CHECK_INDICES=1), counts in the mean's divisor and gets no gradient --
    it never reads a neighbouring field's row.  Offsets are checked on the device as ``bag_pool_ragged`` checks them.
    There is no padding id, and a fused sparse optimizer is not served."""
    if mode not in BAG_MODES:
        raise ValueError(f'bag_pool_fields: mode must be one of {sorted(BAG_MODES)}, got {mode!r}')
    values = _as_index(values)
    if values.dim() == 2 and values.shape[1] == 1:
        values = values.reshape(-1)
    if values.dim() != 1:
        raise ValueError(f"values must be (n,) or (n, 1), got shape {tuple(values.shape)}")
    offsets = _as_index(offsets)
    if offsets.dim() != 1:
        raise ValueError(f"offsets must be one-dimensional, got shape {tuple(offsets.shape)}")
    if weight.dim() != 2:
        raise ValueError(f"weight must be (V, E), got shape {tuple(weight.shape)}")
    fo = field_offsets.rename(None) if field_offsets.has_names() else field_offsets
    if fo.dim() != 1 or fo.shape[0] < 2 or fo.dtype != torch.int64:
        raise ValueError(f"bag_pool_fields: field_offsets must be (F + 1,) int64 with F >= 1, got {tuple(fo.shape)} "
                         f"{fo.dtype}")
    if fo.device != weight.device:
        raise ValueError(f"bag_pool_fields: field_offsets must be on the table's device {weight.device}, got {fo.device}")
    F = fo.shape[0] - 1
    if offsets.shape[0] < 1 or (offsets.shape[0] - 1) % F != 0:
        raise ValueError(f"bag_pool_fields: {offsets.shape[0]} offsets for {F} fields, must be F*B + 1 (field-major, the "
                         f"last one closes the last bag)")
    B = (offsets.shape[0] - 1) // F
    if values.shape[0] >= 2 ** 31 - 1 or F * B >= 2 ** 31 - 1:
        raise ValueError(f"bag_pool_fields: {values.shape[0]} values and {F * B} bags, both must be below 2^31 - 1")
    psw = _check_psw("bag_pool_fields", per_sample_weights, mode, weight, values.shape, flatten=True)
    return _BagPoolFields.apply(weight, values, offsets, fo.contiguous(), psw, BAG_MODES[mode], B, F)


# --------------------------------------------------------------------------------------------
# attention pooling: self-attention over the rows of a (B, L) list of ids, then sum / mean over the list
# --------------------------------------------------------------------------------------------
ATTN_POOL_MODES = {"sum": 0, "mean": 1}


def attn_pool_path(L: int, E: int, H: int, dtype: torch.dtype) -> int:
    """0: no fused kernel for this shape (callers keep the ATen composition), 1: vector path, 2: MFMA path
    (trs_attn_pool_path; a pure function, callable without a device)."""
    if dtype not in (torch.float32, torch.bfloat16):
        return 0
    code = _abi.TRS_F32 if dtype == torch.float32 else _abi.TRS_BF16
    return size_query("trs_attn_pool_path", int(L), int(E), int(H), code)


class _AttnPool(Function):
    @staticmethod
    def forward(ctx, weight, idx, w_qk, b_qk, num_heads, mode, padding_idx, opt=None):
        require_device(weight, idx, w_qk, b_qk)
        B, L = idx.shape
        V, E = weight.shape
        H = int(num_heads)
        w = weight.contiguous()
        wq = w_qk.contiguous()
        bq = b_qk.contiguous() if b_qk is not None else None
        out = torch.empty(B, H, E, dtype=w.dtype, device=w.device)
        flag = _ErrFlag(w.device)
        call("trs_attn_pool_fwd", ptr(w), V, E, value_dtype_code(w), ptr(idx), index_dtype_code(idx), B, L, ptr(wq),
             ptr(bq), H, mode, ptr(out), ptr(flag.t), stream_ptr())
        flag.check("attn_pool")
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        ctx.skip = _skip_row(ctx.padding_idx, V)
        if ctx.needs_input_grad[0]:
            prefetch_row_buckets(idx, None, V, skip_row=ctx.skip)
        # nothing but the inputs is kept: the backward recomputes Q, K and the probabilities from the table rows
        ctx.save_for_backward(idx, weight, w_qk, b_qk)
        ctx.H, ctx.mode, ctx.opt = H, mode, opt
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        idx, weight, w_qk, b_qk = ctx.saved_tensors
        _adopt_grads(g)
        B, L = idx.shape
        V, E = weight.shape
        H = ctx.H
        dev = weight.device
        if B == 0:
            return (torch.zeros_like(weight) if ctx.opt is None else None, None, torch.zeros_like(w_qk),
                    None if b_qk is None else torch.zeros_like(b_qk), None, None, None, None)
        w = weight.contiguous()
        wq = w_qk.contiguous()
        bq = b_qk.contiguous() if b_qk is not None else None
        code = value_dtype_code(w)
        blocks = size_query("trs_attn_pool_blocks", B, L, E, H, code, 1)
        dx = torch.empty(B, L, E, dtype=w.dtype, device=dev)
        dw_part = torch.empty(blocks, 2 * E, E, dtype=torch.float32, device=dev)
        db_part = torch.empty(blocks, 2 * E, dtype=torch.float32, device=dev)
        ws_bytes = size_query("trs_attn_pool_bwd_workspace_bytes", blocks, L, E, H)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        # the row flag was raised by the forward; the backward range-checks without a flag of its own
        call("trs_attn_pool_bwd", ptr(w), V, E, code, ptr(idx), index_dtype_code(idx), B, L, ptr(wq), ptr(bq), H, ctx.mode,
             ptr(g.contiguous()), ptr(dx), ptr(dw_part), ptr(db_part), blocks, ptr(ws), ws_bytes, None, stream_ptr())
        g_wqk = dw_part.sum(0).to(w_qk.dtype) if ctx.needs_input_grad[2] else None          # fixed order: reproducible
        g_bqk = db_part.sum(0).to(b_qk.dtype) if b_qk is not None and ctx.needs_input_grad[3] else None
        grad = None
        if ctx.needs_input_grad[0]:
            rb = row_buckets(idx, None, V, skip_row=ctx.skip)
            grad = _apply_or_grad(rb, weight, ctx.opt, g_rows=dx, padding_row=ctx.padding_idx)
        return grad, None, g_wqk, g_bqk, None, None, None, None


def attn_pool(weight: torch.Tensor, idx: torch.Tensor, w_qk: torch.Tensor, b_qk: Optional[torch.Tensor], num_heads: int,
              mode: str = "mean", padding_idx: Optional[int] = None, opt=None) -> torch.Tensor:
    """(B, H, E): per head the attention-weighted pooled table rows of a padded (B, L) list of ids,
    ``sum_m pbar_h[m] * weight[idx[b, m]]`` with ``pbar_h`` the column sums (``sum``) or means (``mean``) of
    ``softmax((X Wq_h^T + bq_h)(X Wk_h^T + bk_h)^T / sqrt(E / H))`` -- everything of "multi-head self-attention over the
    bag, then pool" that depends on the list positions, in one HIP pass per direction (csrc/attn_pool.hip).  ``w_qk``
    (2E, E) / ``b_qk`` (2E) or None: the query and key rows of ``in_proj_weight`` / ``in_proj_bias``.  Every position
    takes part, padding included.  ``padding_idx``: the table row that receives no gradient.  ``opt``: fused sparse
    optimizer for the table.  Raises for shapes ``attn_pool_path`` refuses."""
    if mode not in ATTN_POOL_MODES:
        raise ValueError(f'attn_pool: mode must be one of {sorted(ATTN_POOL_MODES)}, got {mode!r}')
    idx = _as_index(idx)
    if idx.dim() != 2 or idx.shape[1] < 1:
        raise ValueError(f"indices must be (B, L) with L >= 1, got shape {tuple(idx.shape)}")
    if weight.dim() != 2:
        raise ValueError(f"weight must be (V, E), got shape {tuple(weight.shape)}")
    E = weight.shape[1]
    if tuple(w_qk.shape) != (2 * E, E) or (b_qk is not None and tuple(b_qk.shape) != (2 * E,)):
        raise ValueError(f"attn_pool: w_qk must be ({2 * E}, {E}) and b_qk ({2 * E},)")
    if w_qk.dtype != weight.dtype or (b_qk is not None and b_qk.dtype != weight.dtype):
        raise TypeError("attn_pool: w_qk / b_qk must have the table's dtype")
    if attn_pool_path(idx.shape[1], E, num_heads, weight.dtype) == 0:
        raise NotImplementedError(f"torecsys_amd: attn_pool does not cover L={idx.shape[1]}, E={E}, H={num_heads}, "
                                  f"{weight.dtype} (1 <= L <= 64, E <= 128, E % H == 0, fp32 / bf16)")
    if padding_idx is not None and padding_idx < 0:
        padding_idx = weight.shape[0] + padding_idx
    return _AttnPool.apply(weight, idx, w_qk, b_qk, num_heads, ATTN_POOL_MODES[mode], padding_idx, opt)


def attn_pool_layer(weight: torch.Tensor, idx: torch.Tensor, in_proj_weight: torch.Tensor,
                    in_proj_bias: Optional[torch.Tensor], out_w: torch.Tensor, out_b: Optional[torch.Tensor],
                    num_heads: int, mode: str = "mean", padding_idx: Optional[int] = None, opt=None) -> torch.Tensor:
    """(B, 1, E): ``nn.MultiheadAttention`` (no masks, no dropout) over the looked-up rows of a (B, L) list followed by the
    sum / mean over the list.  ``attn_pool`` covers what depends on the positions; the value and output projections act
    on its (B, H, E) result: ``y = concat_h(xt_h Wv_h^T + c' bv_h) Wout^T + c' bout`` with c' = 1 (mean) or L (sum)."""
    E = weight.shape[1]
    H = int(num_heads)
    d = E // H
    L = idx.shape[1]
    xt = attn_pool(weight, idx, in_proj_weight[:2 * E], None if in_proj_bias is None else in_proj_bias[:2 * E], H, mode,
                   padding_idx, opt)
    B = xt.shape[0]
    cb = 1.0 if mode == "mean" else float(L)
    wv = in_proj_weight[2 * E:].reshape(H, d, E)
    o = torch.bmm(xt.transpose(0, 1), wv.transpose(1, 2)).transpose(0, 1).reshape(B, E)      # (H,B,E)x(H,E,d) -> (B, H*d)
    if in_proj_bias is not None:
        o = o + cb * in_proj_bias[2 * E:]
    y = torch.nn.functional.linear(o, out_w)
    if out_b is not None:
        y = y + cb * out_b
    return y.unsqueeze(1)


class _AttnPoolRagged(Function):
    """attn_pool on one flat id vector (n,) plus offsets (trs_attn_pool_ragged_fwd): _AttnPool's recompute-in-backward
    shape with _BagPoolRagged's operands.  Nothing here reads a tensor back: offsets, live counts and the ``max_length``
    cap are checked on the device.  The row buckets are those of the ids seen as an (n, 1) batch."""

    @staticmethod
    def forward(ctx, weight, ids, offsets, w_qk, b_qk, num_heads, mode, padding_idx, exclude, B, max_length):
        require_device(weight, ids, offsets, w_qk, b_qk)
        n = ids.shape[0]
        V, E = weight.shape
        H = int(num_heads)
        w = weight.contiguous()
        wq = w_qk.contiguous()
        bq = b_qk.contiguous() if b_qk is not None else None
        dev = w.device
        out = torch.empty(B, H, E, dtype=w.dtype, device=dev)
        cnt = torch.empty(B, dtype=torch.float32, device=dev)
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        ctx.exclude_row = ctx.padding_idx if exclude else -1
        flag = _ErrFlag(dev)
        call("trs_attn_pool_ragged_fwd", ptr(w), V, E, value_dtype_code(w), ptr(ids), index_dtype_code(ids), n,
             ptr(offsets), index_dtype_code(offsets), offsets.shape[0], B, max_length, ctx.exclude_row, ptr(wq), ptr(bq),
             H, mode, ptr(out), ptr(cnt), ptr(flag.t), stream_ptr())
        flag.check("attn_pool_ragged")
        ctx.skip = _skip_row(ctx.padding_idx, V)
        if ctx.needs_input_grad[0] and n > 0 and B > 0:
            prefetch_row_buckets(ids.view(n, 1), None, V, skip_row=ctx.skip)
        # nothing but the inputs is kept: the backward finds the live ids again and recomputes Q, K and the probabilities
        ctx.save_for_backward(ids, offsets, weight, w_qk, b_qk)
        ctx.H, ctx.mode, ctx.B, ctx.max_length = H, mode, B, max_length
        ctx.mark_non_differentiable(cnt)
        return out, cnt

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_cnt):
        ids, offsets, weight, w_qk, b_qk = ctx.saved_tensors
        _adopt_grads(g)
        n, B, H = ids.shape[0], ctx.B, ctx.H
        V, E = weight.shape
        dev = weight.device
        if B == 0:
            return (torch.zeros_like(weight), None, None, torch.zeros_like(w_qk),
                    None if b_qk is None else torch.zeros_like(b_qk), None, None, None, None, None, None)
        w = weight.contiguous()
        wq = w_qk.contiguous()
        bq = b_qk.contiguous() if b_qk is not None else None
        code = value_dtype_code(w)
        blocks = size_query("trs_attn_pool_ragged_blocks", B, ctx.max_length, E, H, code, 1)
        # the kernel writes the rows of the positions a bag takes; this zero-fill makes every other row (excluded, beyond
        # max_length, in an empty range or in no bag) an exact zero
        dx = torch.zeros(n, E, dtype=w.dtype, device=dev)
        dw_part = torch.empty(blocks, 2 * E, E, dtype=torch.float32, device=dev)
        db_part = torch.empty(blocks, 2 * E, dtype=torch.float32, device=dev)
        ws_bytes = size_query("trs_attn_pool_ragged_bwd_workspace_bytes", blocks, ctx.max_length, E, H)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        # every flag was raised by the forward; the backward checks ranges without a flag of its own
        call("trs_attn_pool_ragged_bwd", ptr(w), V, E, code, ptr(ids), index_dtype_code(ids), n, ptr(offsets),
             index_dtype_code(offsets), offsets.shape[0], B, ctx.max_length, ctx.exclude_row, ptr(wq), ptr(bq), H, ctx.mode,
             ptr(g.contiguous()), ptr(dx), ptr(dw_part), ptr(db_part), blocks, ptr(ws), ws_bytes, None, stream_ptr())
        g_wqk = dw_part.sum(0).to(w_qk.dtype) if ctx.needs_input_grad[3] else None          # fixed order: reproducible
        g_bqk = db_part.sum(0).to(b_qk.dtype) if b_qk is not None and ctx.needs_input_grad[4] else None
        grad = None
        if ctx.needs_input_grad[0]:
            if n == 0:
                grad = torch.zeros_like(weight)
            else:
                rb = row_buckets(ids.view(n, 1), None, V, skip_row=ctx.skip)
                grad = scatter_rows(rb, weight, g_rows=dx, padding_row=ctx.padding_idx)
        return grad, None, None, g_wqk, g_bqk, None, None, None, None, None, None


def attn_pool_ragged(weight: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, w_qk: torch.Tensor,
                     b_qk: Optional[torch.Tensor], num_heads: int, mode: str = "mean", padding_idx: Optional[int] = None, *,
                     max_length: int, exclude_padding: bool = False,
                     include_last_offset: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``attn_pool`` for RAGGED bags (``ids`` (n,) or (n,1) plus ``offsets``, as ``bag_pool_ragged`` takes them): a bag
    attends to its own ids and nothing else.  Returns ``(xt (B, H, E), cnt (B,) fp32)``: per head
    ``sum_m pbar_h[m] * weight[ids_b[m]]`` over the L_b ids the bag holds, ``pbar_h`` the column sums (``sum``) or the
    column sums / L_b (``mean``) of the bag's own (L_b, L_b) softmax, and ``cnt[b] = L_b`` (not differentiable).  With
    ``exclude_padding=True`` the ids equal to ``padding_idx`` are removed from the bag first (no key-padding mask
    exists).  ``max_length`` (1..64) sizes the kernels' working set and caps a bag: the first ``max_length`` live ids are
    taken, the others contribute nothing, and a longer bag raises the index flag (``index_errors_seen()``; IndexError with
    TRS_CHECK_INDICES=1) -- as an out-of-range id or offset does.  An empty bag gives a zero block and ``cnt = 0``.  No
    length is read on the host.  Raises for shapes ``attn_pool_path(max_length, E, H, dtype)`` refuses."""
    if mode not in ATTN_POOL_MODES:
        raise ValueError(f'attn_pool_ragged: mode must be one of {sorted(ATTN_POOL_MODES)}, got {mode!r}')
    max_length = int(max_length)
    if not 1 <= max_length <= 64:
        raise ValueError(f"attn_pool_ragged: max_length must be in [1, 64], got {max_length}")
    ids = _as_index(ids)
    if ids.dim() == 2 and ids.shape[1] == 1:
        ids = ids.reshape(-1)
    if ids.dim() != 1:
        raise ValueError(f"ids must be (n,) or (n, 1), got shape {tuple(ids.shape)}")
    offsets = _as_index(offsets)
    if offsets.dim() != 1:
        raise ValueError(f"offsets must be one-dimensional, got shape {tuple(offsets.shape)}")
    B = offsets.shape[0] - 1 if include_last_offset else offsets.shape[0]
    if B < 0:
        raise ValueError("attn_pool_ragged: include_last_offset=True needs at least one offset")
    if ids.shape[0] >= 2 ** 31 - 1:
        raise ValueError(f"attn_pool_ragged: {ids.shape[0]} ids, must be below 2^31 - 1")
    if weight.dim() != 2:
        raise ValueError(f"weight must be (V, E), got shape {tuple(weight.shape)}")
    V, E = weight.shape
    if tuple(w_qk.shape) != (2 * E, E) or (b_qk is not None and tuple(b_qk.shape) != (2 * E,)):
        raise ValueError(f"attn_pool_ragged: w_qk must be ({2 * E}, {E}) and b_qk ({2 * E},)")
    if w_qk.dtype != weight.dtype or (b_qk is not None and b_qk.dtype != weight.dtype):
        raise TypeError("attn_pool_ragged: w_qk / b_qk must have the table's dtype")
    if attn_pool_path(max_length, E, num_heads, weight.dtype) == 0:
        raise NotImplementedError(f"torecsys_amd: attn_pool_ragged does not cover max_length={max_length}, E={E}, "
                                  f"H={num_heads}, {weight.dtype} (E <= 128, E % H == 0, fp32 / bf16)")
    padding_idx = _norm_padding("attn_pool_ragged", padding_idx, V, exclude_padding)
    return _AttnPoolRagged.apply(weight, ids, offsets, w_qk, b_qk, num_heads, ATTN_POOL_MODES[mode], padding_idx,
                                 bool(exclude_padding), B, max_length)


def attn_pool_ragged_layer(weight: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, in_proj_weight: torch.Tensor,
                           in_proj_bias: Optional[torch.Tensor], out_w: torch.Tensor, out_b: Optional[torch.Tensor],
                           num_heads: int, mode: str = "mean", padding_idx: Optional[int] = None, *, max_length: int,
                           exclude_padding: bool = False, include_last_offset: bool = False) -> torch.Tensor:
    """(B, 1, E): per bag, ``nn.MultiheadAttention`` (no masks, no dropout) over the bag's own rows followed by the sum /
    mean over them.  ``attn_pool_ragged`` covers what depends on the positions; the value and output projections act on
    its (B, H, E) result as in ``attn_pool_layer``, with a per-sample bias factor c'[b] = L_b (sum) or [L_b > 0] (mean),
    so an empty bag is an exact zero row in both modes."""
    E = weight.shape[1]
    H = int(num_heads)
    d = E // H
    xt, cnt = attn_pool_ragged(weight, ids, offsets, in_proj_weight[:2 * E],
                               None if in_proj_bias is None else in_proj_bias[:2 * E], H, mode, padding_idx,
                               max_length=max_length, exclude_padding=exclude_padding,
                               include_last_offset=include_last_offset)
    B = xt.shape[0]
    cb = (cnt if mode == "sum" else (cnt > 0)).to(xt.dtype).unsqueeze(1)                     # (B, 1)
    wv = in_proj_weight[2 * E:].reshape(H, d, E)
    o = torch.bmm(xt.transpose(0, 1), wv.transpose(1, 2)).transpose(0, 1).reshape(B, E)      # (H,B,E)x(H,E,d) -> (B, H*d)
    if in_proj_bias is not None:
        o = o + cb * in_proj_bias[2 * E:]
    y = torch.nn.functional.linear(o, out_w)
    if out_b is not None:
        y = y + cb * out_b
    return y.unsqueeze(1)


# --------------------------------------------------------------------------------------------
# residual self-attention over a short list: x + nn.MultiheadAttention(x, x, x), un-pooled
# --------------------------------------------------------------------------------------------
def self_attn_path(L: int, E: int, H: int, dtype: torch.dtype) -> int:
    """0: no fused kernel for this shape (callers keep the ATen composition), 1: vector path, 2: MFMA path
    (trs_self_attn_path; a pure function, callable without a device)."""
    if dtype not in (torch.float32, torch.bfloat16):
        return 0
    code = _abi.TRS_F32 if dtype == torch.float32 else _abi.TRS_BF16
    return size_query("trs_self_attn_path", int(L), int(E), int(H), code)


class _SelfAttnResidual(Function):
    @staticmethod
    def forward(ctx, x, w_in, b_in, w_out, b_out, num_heads):
        require_device(x, w_in, b_in, w_out, b_out)
        B, L, E = x.shape
        H = int(num_heads)
        xc = x.contiguous()
        y = torch.empty(B, L, E, dtype=x.dtype, device=x.device)
        call("trs_self_attn_fwd", ptr(xc), B, L, E, H, value_dtype_code(xc), ptr(w_in.contiguous()),
             ptr(None if b_in is None else b_in.contiguous()), ptr(w_out.contiguous()),
             ptr(None if b_out is None else b_out.contiguous()), ptr(y), stream_ptr())
        # nothing but the inputs is kept: the backward recomputes Q, K, V, the probabilities and O from x
        ctx.save_for_backward(x, w_in, b_in, w_out, b_out)
        ctx.H = H
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w_in, b_in, w_out, b_out = ctx.saved_tensors
        B, L, E = x.shape
        need = ctx.needs_input_grad
        if B == 0:
            return tuple(torch.zeros_like(t) if t is not None and n else None
                         for t, n in zip((x, w_in, b_in, w_out, b_out), need)) + (None,)
        dev = x.device
        xc = x.contiguous()
        code = value_dtype_code(xc)
        blocks = size_query("trs_self_attn_blocks", B, L, E, ctx.H, code, 1)
        ws_bytes = size_query("trs_self_attn_bwd_workspace_bytes", blocks, E)
        slabs = torch.empty(blocks, 4 * E * E + 4 * E, dtype=torch.float32, device=dev)
        dx = torch.empty(B, L, E, dtype=x.dtype, device=dev) if need[0] else None
        call("trs_self_attn_bwd", ptr(xc), B, L, E, ctx.H, code, ptr(w_in.contiguous()),
             ptr(None if b_in is None else b_in.contiguous()), ptr(w_out.contiguous()),
             ptr(None if b_out is None else b_out.contiguous()), ptr(g.contiguous()), ptr(dx), ptr(slabs), ws_bytes,
             blocks, stream_ptr())
        tot = slabs.sum(0)          # fixed order: reproducible
        o1, o2, o3 = 3 * E * E, 4 * E * E, 4 * E * E + 3 * E
        g_win = tot[:o1].view(3 * E, E).to(w_in.dtype) if need[1] else None
        g_bin = tot[o2:o3].to(b_in.dtype) if b_in is not None and need[2] else None
        g_wout = tot[o1:o2].view(E, E).to(w_out.dtype) if need[3] else None
        g_bout = tot[o3:].to(b_out.dtype) if b_out is not None and need[4] else None
        return dx, g_win, g_bin, g_wout, g_bout, None


def self_attn_residual(x: torch.Tensor, in_proj_weight: torch.Tensor, in_proj_bias: Optional[torch.Tensor],
                       out_w: torch.Tensor, out_b: Optional[torch.Tensor], num_heads: int) -> torch.Tensor:
    """(B, L, E) in ``x``'s dtype: ``x + nn.MultiheadAttention(E, num_heads)(x, x, x)`` over the list dimension of a
    batch-first (B, L, E) block, without masks or dropout, in one HIP pass per direction (csrc/self_attn.hip).
    ``in_proj_weight`` (3E, E), ``out_w`` (E, E); ``in_proj_bias`` (3E) and ``out_b`` (E) are both given or both None.
    The backward recomputes everything from ``x``; the weight gradients are reduced in a fixed order (same bits on every
    call).  Raises for shapes ``self_attn_path`` refuses."""
    if x.dim() != 3:
        raise ValueError(f"self_attn_residual: x must be (B, L, E), got shape {tuple(x.shape)}")
    B, L, E = x.shape
    if tuple(in_proj_weight.shape) != (3 * E, E) or tuple(out_w.shape) != (E, E):
        raise ValueError(f"self_attn_residual: in_proj_weight must be ({3 * E}, {E}) and out_w ({E}, {E})")
    if (in_proj_bias is None) != (out_b is None):
        raise ValueError("self_attn_residual: in_proj_bias and out_b are both given or both None")
    if in_proj_bias is not None and (tuple(in_proj_bias.shape) != (3 * E,) or tuple(out_b.shape) != (E,)):
        raise ValueError(f"self_attn_residual: in_proj_bias must be ({3 * E},) and out_b ({E},)")
    if any(t is not None and t.dtype != x.dtype for t in (in_proj_weight, in_proj_bias, out_w, out_b)):
        raise TypeError("self_attn_residual: the parameters must have x's dtype")
    if self_attn_path(L, E, num_heads, x.dtype) == 0:
        raise NotImplementedError(f"torecsys_amd: self_attn_residual does not cover L={L}, E={E}, H={num_heads}, {x.dtype} "
                                  f"(1 <= L <= 64, E <= 128, E % H == 0, fp32 / bf16)")
    return _SelfAttnResidual.apply(x, in_proj_weight, in_proj_bias, out_w, out_b, num_heads)


# --------------------------------------------------------------------------------------------
# K1+K2(+K8): fused lookup + FM (+ first-order sum)
# --------------------------------------------------------------------------------------------
class _EmbedFM(Function):
    """``fields=True``: the first-order output is the per-field tensor (B,N,1) the reference's models consume (one value
    per lookup, trs_embed_fm_fields) instead of its sum (B,1); the backward then takes both tables' dense gradients from
    one bucket walk (trs_scatter_rows_first)."""

    @staticmethod
    def forward(ctx, weight, idx, offsets, first_weight, want_emb, opt=None, fields=False, padding_idx=None):
        require_device(weight, idx, offsets, first_weight)
        B, N = idx.shape
        V, E = weight.shape
        w = weight.contiguous()
        dev = w.device
        emb = torch.empty(B, N, E, dtype=w.dtype, device=dev) if want_emb else None
        fm = torch.empty(B, E, dtype=w.dtype, device=dev)
        fm_sum = torch.empty(B, E, dtype=torch.float32, device=dev)
        first = None
        fw = None
        if first_weight is not None:
            if first_weight.dtype != w.dtype or first_weight.numel() != V:
                raise ValueError("first-order table must be (V,1) with the embedding table's dtype")
            fw = first_weight.contiguous()
            first = torch.empty((B, N, 1) if fields else (B, 1), dtype=w.dtype, device=dev)
        elif fields:
            raise ValueError("fields=True needs the first-order table")
        flag = _ErrFlag(dev)
        if PREFETCH_EARLY and (ctx.needs_input_grad[0] or ctx.needs_input_grad[3]):
            prefetch_row_buckets(idx, offsets, V, now=True)
        call("trs_embed_fm_fields" if fields else "trs_embed_fm", ptr(w), V, E, value_dtype_code(w), ptr(idx),
             index_dtype_code(idx), ptr(offsets), B, N, ptr(emb), ptr(fm), ptr(fm_sum), ptr(fw), ptr(first), ptr(flag.t),
             stream_ptr())
        flag.check("embed_fm")
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[3]:
            prefetch_row_buckets(idx, offsets, V)
        ctx.save_for_backward(idx, offsets, weight, first_weight, fm_sum)
        ctx.want_emb = want_emb
        ctx.opt = opt
        ctx.fields = bool(fields)
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        ctx.set_materialize_grads(False)   # unused outputs arrive as None, not as zero blocks
        outs = (emb if want_emb else fm.new_empty(0), fm, first if first is not None else fm.new_empty(0))
        if not want_emb:
            ctx.mark_non_differentiable(outs[0])
        if first is None:
            ctx.mark_non_differentiable(outs[2])
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g_emb, g_fm, g_first):
        idx, offsets, weight, first_weight, fm_sum = ctx.saved_tensors
        _adopt_grads(g_emb, g_fm, g_first)
        V, E = weight.shape
        rb = row_buckets(idx, offsets, V)
        gw = gfw = None
        has_emb = ctx.want_emb and g_emb is not None
        has_fm = g_fm is not None
        pad = ctx.padding_idx      # nn.Embedding(padding_idx=): that row of the E-wide table receives no gradient
        if (ctx.fields and ctx.opt is None and g_first is not None and (has_emb or has_fm) and pad < 0
                and ctx.needs_input_grad[0] and ctx.needs_input_grad[3]):
            g_rows = g_emb.contiguous() if has_emb else None
            g_bcast = _fm_grad_operand(g_fm) if has_fm else None
            # (a per-sample FM gradient is read as scalars: its own alignment does not matter)
            if _walk_takes_vectors(weight, g_rows, weight if has_fm else None,
                                   g_bcast if has_fm and _bcast_cols(g_bcast, E) == E else None):
                gw, gfw = scatter_rows_first(rb, weight, first_weight, g_first.contiguous(), g_rows=g_rows,
                                             g_bcast=g_bcast, fm_sum=fm_sum if has_fm else None)
                return gw, None, None, gfw, None, None, None, None
        if ctx.needs_input_grad[0]:
            if has_emb or has_fm:
                gw = _apply_or_grad(rb, weight, ctx.opt, g_rows=g_emb.contiguous() if has_emb else None,
                                    g_bcast=_fm_grad_operand(g_fm) if has_fm else None, fm_sum=fm_sum if has_fm else None,
                                    padding_row=pad)
            elif ctx.opt is None:
                gw = torch.zeros_like(weight)
        if first_weight is not None and ctx.needs_input_grad[3]:
            if g_first is not None:
                if ctx.fields:       # one gradient value per lookup: the E = 1 table's own bucketed scatter
                    gfw = _apply_or_grad(rb, first_weight.reshape(V, 1), ctx.opt, key=first_weight,
                                         g_rows=g_first.contiguous())
                else:
                    gfw = _apply_or_grad(rb, first_weight.reshape(V, 1), ctx.opt, key=first_weight,
                                         g_bcast=g_first.contiguous().reshape(-1, 1))
                gfw = None if gfw is None else gfw.reshape(first_weight.shape)
            elif ctx.opt is None:
                gfw = torch.zeros_like(first_weight)
        return gw, None, None, gfw, None, None, None, None


def embed_fm(weight: torch.Tensor, idx: torch.Tensor, offsets: Optional[torch.Tensor] = None,
             first_weight: Optional[torch.Tensor] = None, want_emb: bool = True, opt=None,
             padding_idx: Optional[int] = None
             ) -> Tuple[Optional[torch.Tensor], torch.Tensor, Optional[torch.Tensor]]:
    """One pass over the looked-up rows: (emb (B,N,E) | None, fm (B,E), first (B,1) | None).  ``padding_idx``: the
    table row nn.Embedding(padding_idx=) keeps gradient-free (multi_indices_emb.py:48 forwards it); the forward reads
    that row like any other, as F.embedding does."""
    idx = _as_index(idx)
    if idx.dim() != 2:
        raise ValueError(f"indices must be (B, N), got shape {tuple(idx.shape)}")
    if padding_idx is not None and padding_idx < 0:
        padding_idx = weight.shape[0] + padding_idx
    emb, fm, first = _EmbedFM.apply(weight, idx, offsets, first_weight, want_emb, opt, False, padding_idx)
    return (emb if want_emb else None), fm, (first if first_weight is not None else None)


def embed_fm_fields(weight: torch.Tensor, first_weight: torch.Tensor, idx: torch.Tensor,
                    offsets: Optional[torch.Tensor] = None, opt=None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The lookup of an embedding table, the FM term of the looked-up rows and the per-field lookup of the first-order
    table that shares the indices, in one pass: (emb (B,N,E), fm (B,E), first (B,N,1))."""
    idx = _as_index(idx)
    if idx.dim() != 2:
        raise ValueError(f"indices must be (B, N), got shape {tuple(idx.shape)}")
    return _EmbedFM.apply(weight, idx, offsets, first_weight, True, opt, True)


# --------------------------------------------------------------------------------------------
# K2: FM on a materialised block
# --------------------------------------------------------------------------------------------
class _FMLayer(Function):
    @staticmethod
    def forward(ctx, x):
        require_device(x)
        x = x.contiguous()
        B, N, E = x.shape
        fm = torch.empty(B, E, dtype=x.dtype, device=x.device)
        fm_sum = torch.empty(B, E, dtype=torch.float32, device=x.device)
        call("trs_fm_fwd", ptr(x), B, N, E, value_dtype_code(x), ptr(fm), ptr(fm_sum), stream_ptr())
        ctx.save_for_backward(x, fm_sum)
        return fm

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, fm_sum = ctx.saved_tensors
        B, N, E = x.shape
        dx = torch.empty_like(x)
        call("trs_fm_bwd", ptr(x), ptr(g.contiguous()), ptr(fm_sum), B, N, E, value_dtype_code(x), ptr(dx),
             stream_ptr())
        return dx


def fm_layer(x: torch.Tensor) -> torch.Tensor:
    if x.dim() != 3:
        raise ValueError(f"FM input must be (B, N, E), got {tuple(x.shape)}")
    return _FMLayer.apply(x)


# --------------------------------------------------------------------------------------------
# I3: field-aware gather  (B,N) -> (B,N*N,E)
# --------------------------------------------------------------------------------------------
_ptr_table_cache = {}


def _pointer_table(tensors: Sequence[torch.Tensor]) -> torch.Tensor:
    """Device array of base pointers (cached per pointer tuple: a blocking 8*N-byte upload otherwise)."""
    key = tuple(t.data_ptr() for t in tensors)
    tab = _ptr_table_cache.get(key)
    if tab is None:
        if len(_ptr_table_cache) > 64:
            _ptr_table_cache.clear()
        # a pageable host -> device copy with non_blocking=False: PyTorch synchronises the copy's stream before returning,
        # so the entry is complete for every stream that reads it afterwards (lookups run on several streams)
        tab = torch.tensor(key, dtype=torch.int64).to(tensors[0].device, non_blocking=False)
        _ptr_table_cache[key] = tab
    return tab


class _FAGather(Function):
    @staticmethod
    def forward(ctx, idx, offsets, *weights):
        require_device(idx, offsets, *weights)
        B, N = idx.shape
        if len(weights) != N:
            raise ValueError(f"need {N} tables, got {len(weights)}")
        V, E = weights[0].shape
        ws = [w.contiguous() for w in weights]
        for w in ws:
            if w.shape != (V, E) or w.dtype != ws[0].dtype:
                raise ValueError("field-aware tables must share shape and dtype")
        out = torch.empty(B, N * N, E, dtype=ws[0].dtype, device=ws[0].device)
        flag = _ErrFlag(out.device)
        call("trs_fa_gather_rows", ptr(_pointer_table(ws)), V, E, value_dtype_code(ws[0]), ptr(idx),
             index_dtype_code(idx), ptr(offsets), B, N, ptr(out), ptr(flag.t), stream_ptr())
        flag.check("fa_gather_rows")
        if any(ctx.needs_input_grad[2:]):
            prefetch_row_buckets(idx, offsets, V)
        ctx.save_for_backward(idx, offsets, *weights)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        idx, offsets, *weights = ctx.saved_tensors
        _adopt_grads(g)
        B, N = idx.shape
        V, E = weights[0].shape
        g = g.contiguous()
        rb = row_buckets(idx, offsets, V)
        grads = []
        for i, w in enumerate(weights):
            if ctx.needs_input_grad[2 + i]:
                grads.append(scatter_rows(rb, w, g_rows=g[:, i * N:(i + 1) * N], g_rows_batch_stride=N * N))
            else:
                grads.append(None)
        return (None, None, *grads)


_table_rows_cache = {}


def _tables_meta(weights: Sequence[torch.Tensor]):
    """(row counts, cumulative row offsets) of N tables as device int64 tensors, cached per shape tuple and device"""
    key = (tuple(int(w.shape[0]) for w in weights), weights[0].device)
    m = _table_rows_cache.get(key)
    if m is None:
        if len(_table_rows_cache) > 64:
            _table_rows_cache.clear()
        rows = torch.tensor(key[0], dtype=torch.int64)
        off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(rows, 0)[:-1]])
        m = _table_rows_cache[key] = (rows.to(key[1], non_blocking=False), off.to(key[1], non_blocking=False))  # blocking: see _pointer_table
    return m


class _GatherRowsTables(Function):
    """out[b,n,:] = weights[n][idx[b,n],:] for N SEPARATE tables of one width (a StackedInput of SingleIndexEmbeddings,
    stacked_inp.py:94-134) in one launch (trs_gather_rows_tables).  Backward: one row-bucket build over the concatenated
    row space and one bucket walk into a (sum V_n, E) gradient; every table's gradient is its slice of that tensor."""

    @staticmethod
    def forward(ctx, idx, *weights):
        require_device(idx, *weights)
        B, N = idx.shape
        E = weights[0].shape[1]
        if len(weights) != N:
            raise ValueError(f"gather_rows_tables: {len(weights)} tables for {N} index columns")
        ws = [w.contiguous() for w in weights]
        for w in ws:
            if w.dim() != 2 or w.shape[1] != E or w.dtype != ws[0].dtype:
                raise ValueError("gather_rows_tables: the tables must share embed size and dtype")
            if (E * w.element_size()) % 16 == 0 and w.data_ptr() % 16 != 0:
                raise ValueError("gather_rows_tables: every table must be 16-byte aligned")
        rows, offsets = _tables_meta(ws)
        out = torch.empty(B, N, E, dtype=ws[0].dtype, device=ws[0].device)
        flag = _ErrFlag(out.device)
        call("trs_gather_rows_tables", ptr(_pointer_table(ws)), ptr(rows), E, value_dtype_code(ws[0]), ptr(idx),
             index_dtype_code(idx), B, N, ptr(out), ptr(flag.t), stream_ptr())
        flag.check("gather_rows_tables")
        if any(ctx.needs_input_grad[1:]):
            prefetch_row_buckets(idx, offsets, int(sum(w.shape[0] for w in ws)))
        ctx.save_for_backward(idx, offsets)
        ctx.shapes = [tuple(w.shape) for w in ws]
        ctx.like = ws[0]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        idx, offsets = ctx.saved_tensors
        _adopt_grads(g)
        Vs = [s[0] for s in ctx.shapes]
        Vtot, E = sum(Vs), ctx.shapes[0][1]
        rb = row_buckets(idx, offsets, Vtot)
        gcat = scatter_rows(rb, _ShapeOnly(Vtot, E, ctx.like), g_rows=g.contiguous())
        grads, o = [], 0
        for i, v in enumerate(Vs):
            grads.append(gcat[o:o + v] if ctx.needs_input_grad[1 + i] else None)
            o += v
        return (None, *grads)


class _ShapeOnly:
    """what scatter_rows needs of its ``like_table`` when no (V,E) table exists: shape, dtype, device"""

    def __init__(self, V, E, like):
        self.shape, self.dtype, self.device, self._like = (V, E), like.dtype, like.device, like

    def element_size(self):
        return self._like.element_size()


def gather_rows_tables(weights: Sequence[torch.Tensor], idx: torch.Tensor) -> torch.Tensor:
    """(B,N) raw per-table indices -> (B,N,E) from N separate (V_n,E) tables; dense per-table gradients"""
    idx = _as_index(idx)
    if idx.dim() == 1:
        idx = idx.unsqueeze(-1)
    if idx.dim() != 2:
        raise ValueError(f"indices must be (B, N), got shape {tuple(idx.shape)}")
    return _GatherRowsTables.apply(idx, *weights)


def fa_gather_rows(weights: Sequence[torch.Tensor], idx: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    idx = _as_index(idx)
    return _FAGather.apply(idx, offsets, *weights)


# --------------------------------------------------------------------------------------------
# K7: inner-product network
# --------------------------------------------------------------------------------------------
class _PairDot(Function):
    @staticmethod
    def forward(ctx, x):
        require_device(x)
        x = x.contiguous()
        B, N, E = x.shape
        out = torch.empty(B, N * (N - 1) // 2, dtype=x.dtype, device=x.device)
        call("trs_pair_dot_fwd", ptr(x), B, N, E, value_dtype_code(x), ptr(out), stream_ptr())
        ctx.save_for_backward(x)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        B, N, E = x.shape
        dx = torch.empty_like(x)
        call("trs_pair_dot_bwd", ptr(x), ptr(g.contiguous()), B, N, E, value_dtype_code(x), ptr(dx), stream_ptr())
        return dx


def pair_dot(x: torch.Tensor) -> torch.Tensor:
    if x.dim() != 3:
        raise ValueError(f"inner-product input must be (B, N, E), got {tuple(x.shape)}")
    return _PairDot.apply(x)


def embed_ipn_supported(weight: torch.Tensor, N: int) -> bool:
    """the lookup + inner-product kernel covers bf16 tables whose rows the matrix-core pair kernel covers"""
    return (weight.is_cuda and weight.dtype == torch.bfloat16 and weight.dim() == 2 and weight.shape[1] in (32, 64, 128)
            and 2 <= N <= 64)


class _EmbedIPN(Function):
    """K7 fused with K1 (trs_embed_pair_dot): (emb (B,N,E), ipn (B,NC2)) in one pass over the table rows.  The block is
    written only when someone needs it: the caller (``want_emb``) or the backward (it is the ``x`` of trs_pair_dot_bwd);
    at inference with ``want_emb=False`` the (B,N,E) block never exists."""

    @staticmethod
    def forward(ctx, weight, idx, offsets, want_emb, opt=None):
        require_device(weight, idx, offsets)
        B, N = idx.shape
        V, E = weight.shape
        w = weight.contiguous()
        need_block = want_emb or ctx.needs_input_grad[0]
        emb = torch.empty(B, N, E, dtype=w.dtype, device=w.device) if need_block else None
        out = torch.empty(B, N * (N - 1) // 2, dtype=w.dtype, device=w.device)
        flag = _ErrFlag(w.device)
        call("trs_embed_pair_dot", ptr(w), V, E, value_dtype_code(w), ptr(idx), index_dtype_code(idx), ptr(offsets), B, N,
             ptr(emb), ptr(out), ptr(flag.t), stream_ptr())
        flag.check("embed_pair_dot")
        if ctx.needs_input_grad[0]:
            prefetch_row_buckets(idx, offsets, V)
        ctx.save_for_backward(idx, offsets, weight, emb if ctx.needs_input_grad[0] else None)
        ctx.want_emb = want_emb
        ctx.opt = opt
        ctx.set_materialize_grads(False)
        if not want_emb:
            blk = out.new_empty(0)
            ctx.mark_non_differentiable(blk)
            return blk, out
        return emb, out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_emb, g_out):
        idx, offsets, weight, emb = ctx.saved_tensors
        _adopt_grads(g_emb, g_out)
        V, E = weight.shape
        B, N = idx.shape
        g_rows = None
        if g_out is not None:
            g_rows = torch.empty_like(emb)
            call("trs_pair_dot_bwd", ptr(emb), ptr(g_out.contiguous()), B, N, E, value_dtype_code(emb), ptr(g_rows),
                 stream_ptr())
        if ctx.want_emb and g_emb is not None:
            g_rows = g_emb.contiguous() if g_rows is None else g_rows.add_(g_emb)
        if g_rows is None:
            return (torch.zeros_like(weight) if ctx.opt is None else None), None, None, None, None
        rb = row_buckets(idx, offsets, V)
        return _apply_or_grad(rb, weight, ctx.opt, g_rows=g_rows), None, None, None, None


def embed_ipn(weight: torch.Tensor, idx: torch.Tensor, offsets: Optional[torch.Tensor] = None, want_emb: bool = True,
              opt=None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """Lookup + inner-product network in one kernel: (emb (B,N,E) | None, ipn (B, N(N-1)/2))."""
    idx = _as_index(idx)
    if idx.dim() != 2:
        raise ValueError(f"indices must be (B, N), got shape {tuple(idx.shape)}")
    emb, out = _EmbedIPN.apply(weight, idx, offsets, want_emb, opt)
    return (emb if want_emb else None), out


# --------------------------------------------------------------------------------------------
# F4 glue: BatchNorm1d + ReLU + direct/hidden split + pooled sum on channels-last CIN activations
# --------------------------------------------------------------------------------------------
def cin_glue_supported(yT: torch.Tensor, D: int, Hs: int) -> bool:
    C = yT.shape[-1]
    vpr = C // 8
    return (yT.is_cuda and yT.dtype == torch.bfloat16 and yT.dim() == 3 and yT.is_contiguous() and C % 8 == 0
            and 1 <= vpr <= 256 and 256 % vpr == 0 and D % 8 == 0 and Hs % 8 == 0)


class _CINGlue(Function):
    """(hidden (B,E,C-Hs), pooled (B,D)) from the contraction output y (B,E,C): z = relu(bn(y)), hidden = z[..., Hs:],
    pooled = z[..., :D].sum(1).  BatchNorm1d semantics (batch statistics + running-stat update in training, running
    statistics in eval, affine optional) are reproduced here; see trs_cin_glue_*."""

    @staticmethod
    def forward(ctx, yT, gamma, beta, running_mean, running_var, training, momentum, eps, D, Hs):
        require_device(yT)
        B, E, C = yT.shape
        dev = yT.device
        R = B * E
        use_batch = bool(training) or running_mean is None
        if gamma is None and running_mean is None and not training and momentum is None and eps is None:
            use_batch = False                      # no BatchNorm module at all: identity statistics
        if eps is None:
            mean = torch.zeros(C, dtype=torch.float32, device=dev)
            invstd = torch.ones(C, dtype=torch.float32, device=dev)
            use_batch = False
        elif use_batch:
            nblk = size_query("trs_cin_glue_blocks", B)
            part = torch.empty(nblk, 2, C, dtype=torch.float32, device=dev)
            call("trs_cin_glue_stats", ptr(yT), B, E, C, value_dtype_code(yT), ptr(part), stream_ptr())
            tot = part.double().sum(0)
            mean64 = tot[0] / R
            var64 = (tot[1] / R - mean64 * mean64).clamp_min_(0.0)
            mean = mean64.float()
            invstd = (var64 + eps).rsqrt().float()
            if training and running_mean is not None:
                with torch.no_grad():
                    m = float(momentum)
                    running_mean.mul_(1.0 - m).add_(mean64.to(running_mean.dtype), alpha=m)
                    unbiased = var64 * (R / max(R - 1, 1))
                    running_var.mul_(1.0 - m).add_(unbiased.to(running_var.dtype), alpha=m)
        else:
            mean = running_mean.float()
            invstd = (running_var.double() + eps).rsqrt().float()
        g32 = gamma.float() if gamma is not None else torch.ones(C, dtype=torch.float32, device=dev)
        b32 = beta.float() if beta is not None else torch.zeros(C, dtype=torch.float32, device=dev)
        scale = (g32 * invstd).contiguous()
        shift = (b32 - mean * scale).contiguous()
        hidden = torch.empty(B, E, C - Hs, dtype=yT.dtype, device=dev)
        pooled = torch.empty(B, D, dtype=yT.dtype, device=dev)
        cf = C > Hs and bool(size_query("trs_cin_glue_cf_supported", E, C))
        if cf:
            # also emit the hidden half channels-first (B, C-Hs, E): the next layer's weight-gradient kernel reads
            # that layout (otherwise one transposing copy per layer and step); it rides on the returned tensor
            hidden_cf = torch.empty(B, C - Hs, E, dtype=yT.dtype, device=dev)
            call("trs_cin_glue_fwd_cf", ptr(yT), ptr(scale), ptr(shift), B, E, C, D, Hs, value_dtype_code(yT),
                 ptr(hidden), ptr(hidden_cf), ptr(pooled), stream_ptr())
        else:
            hidden_cf = yT.new_empty(0)
            call("trs_cin_glue_fwd", ptr(yT), ptr(scale), ptr(shift), B, E, C, D, Hs, value_dtype_code(yT), ptr(hidden),
                 ptr(pooled), stream_ptr())
        ctx.mark_non_differentiable(hidden_cf)
        ctx.save_for_backward(yT, scale, shift, mean.contiguous(), invstd.contiguous())
        ctx.meta = (use_batch, D, Hs, gamma is not None, beta is not None,
                    None if gamma is None else gamma.dtype)
        ctx.set_materialize_grads(False)
        return hidden, pooled, hidden_cf

    @staticmethod
    @once_differentiable
    def backward(ctx, g_hidden, g_pooled, _g_cf=None):
        yT, scale, shift, mean, invstd = ctx.saved_tensors
        use_batch, D, Hs, has_gamma, has_beta, pdtype = ctx.meta
        B, E, C = yT.shape
        dev = yT.device
        R = B * E
        gh = None if g_hidden is None else g_hidden.contiguous()
        gp = None if g_pooled is None else g_pooled.contiguous()
        nblk = size_query("trs_cin_glue_blocks", B)
        part = torch.empty(nblk, 2, C, dtype=torch.float32, device=dev)
        call("trs_cin_glue_bwd_reduce", ptr(yT), ptr(gh), ptr(gp), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), B, E, C,
             D, Hs, value_dtype_code(yT), ptr(part), stream_ptr())
        tot = part.double().sum(0)
        dbeta, dgamma = tot[0], tot[1]
        if use_batch:
            c1 = (dbeta / R).float().contiguous()
            c2 = (dgamma / R).float().contiguous()
        else:
            c1 = torch.zeros(C, dtype=torch.float32, device=dev)
            c2 = c1
        gy = torch.empty_like(yT)
        if size_query("trs_cin_glue_cf_supported", E, C):
            gy_cf = torch.empty(B, C, E, dtype=yT.dtype, device=dev)      # (B,C,E) copy for trs_cin_dw, see forward
            csum = torch.empty(nblk, C, dtype=torch.float32, device=dev)   # column sums of gy: the conv-bias gradient
            call("trs_cin_glue_bwd_apply_cf", ptr(yT), ptr(gh), ptr(gp), ptr(scale), ptr(shift), ptr(mean), ptr(invstd),
                 ptr(c1), ptr(c2), B, E, C, D, Hs, value_dtype_code(yT), ptr(gy), ptr(gy_cf), ptr(csum), stream_ptr())
            gy._trs_cf = gy_cf
            gy._trs_colsum = (csum, gy._version)
        else:
            call("trs_cin_glue_bwd_apply", ptr(yT), ptr(gh), ptr(gp), ptr(scale), ptr(shift), ptr(mean), ptr(invstd),
                 ptr(c1), ptr(c2), B, E, C, D, Hs, value_dtype_code(yT), ptr(gy), stream_ptr())
        ggamma = dgamma.to(pdtype) if has_gamma and ctx.needs_input_grad[1] else None
        gbeta = dbeta.to(pdtype) if has_beta and ctx.needs_input_grad[2] else None
        return gy, ggamma, gbeta, None, None, None, None, None, None, None


def cin_glue(yT, bn: Optional[torch.nn.Module], D: int, Hs: int):
    """BatchNorm1d ``bn`` (or None) + ReLU + split + pooled sum on yT (B,E,C) bf16 -> (hidden (B,E,C-Hs), pooled (B,D))."""
    if bn is None:
        return _glue_out(_CINGlue.apply(yT, None, None, None, None, False, None, None, D, Hs))
    momentum = bn.momentum
    if bn.training and bn.track_running_stats:
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
            if momentum is None:                              # cumulative moving average
                momentum = 1.0 / float(bn.num_batches_tracked)
    use_running = (not bn.training) and bn.track_running_stats
    return _glue_out(_CINGlue.apply(yT, bn.weight, bn.bias, bn.running_mean if bn.track_running_stats else None,
                                    bn.running_var if bn.track_running_stats else None,
                                    bn.training or not use_running, momentum if momentum is not None else 0.0, bn.eps,
                                    D, Hs))


def _glue_out(res):
    """(hidden, pooled, hidden_cf) -> (hidden, pooled); the channels-first copy rides on ``hidden`` as ``_trs_cf``"""
    hidden, pooled, hidden_cf = res
    if hidden_cf.numel() > 0:
        hidden._trs_cf = hidden_cf
    return hidden, pooled


# --------------------------------------------------------------------------------------------
# N3: outer-product network / bilinear interaction on the pair pattern
# --------------------------------------------------------------------------------------------
def _pair_start(i: int, N: int) -> int:
    return i * (2 * N - i - 1) // 2


class _OPNVec(Function):
    """out[b,p] = sum_e x_i x_j kern[p,e]  ('vec': kern (P,E); 'num': kern (P,))."""

    @staticmethod
    def forward(ctx, x, kern, is_num):
        require_device(x, kern)
        x = x.contiguous()
        kern = kern.contiguous().to(x.dtype)
        B, N, E = x.shape
        out = torch.empty(B, N * (N - 1) // 2, dtype=x.dtype, device=x.device)
        call("trs_opn_vec_fwd", ptr(x), ptr(kern), int(is_num), B, N, E, value_dtype_code(x), ptr(out), stream_ptr())
        ctx.save_for_backward(x, kern)
        ctx.is_num = bool(is_num)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, kern = ctx.saved_tensors
        B, N, E = x.shape
        P = N * (N - 1) // 2
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gk = torch.zeros(P, E, dtype=torch.float32, device=x.device) if ctx.needs_input_grad[1] else None
        ws_bytes = size_query("trs_opn_vec_bwd_workspace_bytes", B, N, E)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        call("trs_opn_vec_bwd", ptr(g.contiguous()), ptr(x), ptr(kern), int(ctx.is_num), B, N, E, value_dtype_code(x),
             ptr(gx), ptr(gk), ptr(ws), ws_bytes, stream_ptr())
        if gk is not None:
            gk = (gk.sum(-1) if ctx.is_num else gk).to(kern.dtype)
        return gx, gk, None


def opn_vec(x: torch.Tensor, kern: torch.Tensor, is_num: bool) -> torch.Tensor:
    if x.dim() != 3:
        raise ValueError(f"outer-product input must be (B, N, E), got {tuple(x.shape)}")
    return _OPNVec.apply(x, kern, is_num)


def _glue_colsum(t: torch.Tensor) -> torch.Tensor:
    """column sums (C,) fp64 of a contiguous bf16 (B, R, C) block that cin_glue_supported accepts: one bf16 read with fp32
    partials per workgroup (trs_cin_glue_stats) instead of a cast to fp32 plus a two-stage ATen reduction (three passes
    over a multi-GB tensor)."""
    B, R, C = t.shape
    nblk = size_query("trs_cin_glue_blocks", B)
    part = torch.empty(nblk, 2, C, dtype=torch.float32, device=t.device)
    call("trs_cin_glue_stats", ptr(t), B, R, C, value_dtype_code(t), ptr(part), stream_ptr())
    return part[:, 0].double().sum(0)


def _pair_bias_grad(g: torch.Tensor, per_pair: bool) -> torch.Tensor:
    """sum of a (B, P, E) gradient over b (per-pair bias) or over (b, p) (shared bias), fp32 accumulation."""
    E = g.shape[2]
    if not per_pair and cin_glue_supported(g, 0, 0):
        return _glue_colsum(g).to(g.dtype)        # column sums of the (B*P, E) matrix
    gb = g.sum(0, dtype=torch.float32) if per_pair else g.reshape(-1, E).sum(0, dtype=torch.float32)
    return gb.to(g.dtype)


class _PairMul(Function):
    """out[b,p,:] = a[b,i_p,:] * c[b,j_p,:] + bias."""

    @staticmethod
    def forward(ctx, a, c, bias, bias_per_pair):
        require_device(a, c, bias)
        a, c = a.contiguous(), c.contiguous()
        B, N, E = a.shape
        bias_c = None if bias is None else bias.contiguous().to(a.dtype)
        out = torch.empty(B, N * (N - 1) // 2, E, dtype=a.dtype, device=a.device)
        call("trs_pair_mul_fwd", ptr(a), ptr(c), ptr(bias_c), int(bool(bias_per_pair)), B, N, E, value_dtype_code(a),
             ptr(out), stream_ptr())
        ctx.save_for_backward(a, c)
        ctx.bias_per_pair = bool(bias_per_pair)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, c = ctx.saved_tensors
        B, N, E = a.shape
        g = g.contiguous()
        ga, gc = torch.empty_like(a), torch.empty_like(c)
        call("trs_pair_mul_bwd", ptr(g), ptr(a), ptr(c), B, N, E, value_dtype_code(a), ptr(ga), ptr(gc), stream_ptr())
        gb = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = _pair_bias_grad(g, ctx.bias_per_pair)
        return ga, gc, gb, None


def pair_mul(a: torch.Tensor, c: torch.Tensor, bias: Optional[torch.Tensor] = None, bias_per_pair: bool = False):
    if a.dim() != 3 or a.shape != c.shape:
        raise ValueError(f"pair_mul operands must both be (B, N, E), got {tuple(a.shape)} and {tuple(c.shape)}")
    return _PairMul.apply(a, c, bias, bias_per_pair)


class _RowsMulBias(Function):
    """out = a * c + bias on (B, P, E) operands that are already gathered per pair (trs_rows_mul_bias_fwd)."""

    @staticmethod
    def forward(ctx, a, c, bias, bias_per_pair):
        require_device(a, c, bias)
        B, P, E = a.shape
        a, c = a.contiguous(), c.contiguous()
        out = torch.empty_like(a)
        bias_c = None if bias is None else bias.to(a.dtype).contiguous()
        call("trs_rows_mul_bias_fwd", ptr(a), ptr(c), ptr(bias_c), int(bool(bias_per_pair)), B * P, P, E,
             value_dtype_code(a), ptr(out), stream_ptr())
        ctx.save_for_backward(a, c)
        ctx.bias_per_pair = bool(bias_per_pair)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, c = ctx.saved_tensors
        B, P, E = a.shape
        g = g.contiguous()
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        call("trs_rows_mul_bwd", ptr(g), ptr(a), ptr(c), B * P, E, value_dtype_code(a), ptr(ga), ptr(gc), stream_ptr())
        gb = _pair_bias_grad(g, ctx.bias_per_pair) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return ga, gc, gb, None


def rows_mul_bias(a: torch.Tensor, c: torch.Tensor, bias: Optional[torch.Tensor] = None, bias_per_pair: bool = False):
    """out = a * c + bias.  Operands (*, P, E) of equal shape -- any number of leading dimensions, as the reference's
    (N, *, H) contract allows (bilinear_interaction.py:11-79); they are folded into one batch axis for the kernel.
    bias: (E,) shared by every pair, or (P, E) with ``bias_per_pair``; its shape is checked here because the kernel
    indexes it without one."""
    if a.dim() < 2 or a.shape != c.shape:
        raise ValueError(f"rows_mul_bias operands must both be (*, P, E), got {tuple(a.shape)} and {tuple(c.shape)}")
    P, E = a.shape[-2], a.shape[-1]
    if bias is not None:
        want = (P, E) if bias_per_pair else (E,)
        if tuple(bias.shape) != want:
            raise ValueError(f"rows_mul_bias: bias must be {want} for operands {tuple(a.shape)}, got {tuple(bias.shape)}")
    if a.dim() == 3:
        return _RowsMulBias.apply(a, c, bias, bias_per_pair)
    lead = a.shape[:-2]
    out = _RowsMulBias.apply(a.reshape(-1, P, E), c.reshape(-1, P, E), bias, bias_per_pair)
    return out.reshape(*lead, P, E)


PAIR_GEMM_MIN_BATCH = 256      # below this the one-kernel path (weights streamed per sample group) is used


def _pair_gemm_route(x: torch.Tensor) -> bool:
    B, N, E = x.shape
    ve = 16 // x.element_size()
    vpr = E // ve if E % ve == 0 else 0
    return (B >= PAIR_GEMM_MIN_BATCH and vpr > 0 and (vpr & (vpr - 1)) == 0 and vpr <= 64
            and (N * E * 8 + N * N * 2 + 64) <= 64 * 1024)


def _pair_T(x: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
    """T[b,p,:] = x[b,i_p,:] @ W[p]: one plain GEMM per field i over its adjacent pairs (i, i+1..N-1)."""
    B, N, E = x.shape
    P = N * (N - 1) // 2
    T = torch.empty(B, P, E, dtype=x.dtype, device=x.device)
    T2 = T.view(B, P * E)
    for i in range(N - 1):
        p0, n_i = _pair_start(i, N), N - 1 - i
        Wcat = W[p0:p0 + n_i].permute(1, 0, 2).reshape(E, n_i * E)          # [e][(q,h)] = W[p0+q][e][h]
        torch.mm(x[:, i, :], Wcat, out=T2[:, p0 * E:(p0 + n_i) * E])
    return T


_pair_task_cache = {}


def _pair_tasks(N: int, device):
    """Task lists of the MFMA per-pair kernels, cached per (N, device):
    tasks_i (nti,3) = (i, j0, count <= 3): pairs (i, j0..j0+count-1);  seg_i (N+1): first task of field i;
    tasks_j (ntj,3) = (j, i0, count <= 3): pairs (i0..i0+count-1, j);  seg_j (N+1): first task of field j."""
    key = (N, str(device))
    t = _pair_task_cache.get(key)
    if t is None:
        ti, si, tj, sj = [], [0], [], [0]
        for i in range(N):
            ti += [(i, j0, min(3, N - j0)) for j0 in range(i + 1, N, 3)]
            si.append(len(ti))
        for j in range(N):
            tj += [(j, i0, min(3, j - i0)) for i0 in range(0, j, 3)]
            sj.append(len(tj))
        mk = lambda rows: torch.tensor(rows, dtype=torch.int32, device=device)
        t = _pair_task_cache[key] = (mk(ti), mk(si), mk(tj), mk(sj))
    return t


def _pair_mfma_fwd_ok(x: torch.Tensor) -> bool:
    return x.dtype == torch.bfloat16 and x.shape[2] in (32, 64) and x.shape[1] >= 2 and x.shape[0] >= 16


class _PairBilinear(Function):
    """T = x_i W_p;  mode 0: out[b,p] = sum_h T_h x_j[h]  |  mode 1: out[b,p,:] = T * x_j + bias_p.   W (P,E,E) [e][h].
    Two routes: one HIP kernel that streams W_p per group of samples (small batches, any shape), or -- at training
    batch sizes -- plain per-field GEMMs for T / dL/dx_i / dL/dW around HIP epilogue passes (trs_pair_epilogue_*)."""

    @staticmethod
    def forward(ctx, x, W, bias, mode):
        require_device(x, W, bias)
        x = x.contiguous()
        B, N, E = x.shape
        P = N * (N - 1) // 2
        if tuple(W.shape) != (P, E, E):
            raise ValueError(f"per-pair weights must be ({P}, {E}, {E}), got {tuple(W.shape)}")
        Wc = W.contiguous().to(x.dtype)
        bias_c = None if bias is None else bias.contiguous().to(x.dtype)
        ctx.gemm = _pair_gemm_route(x)
        if _pair_mfma_fwd_ok(x):
            # forward on the matrix cores in one kernel (W_p^T fragments resident per wave)
            Wt = Wc.transpose(1, 2).contiguous()
            tasks = _pair_tasks(N, x.device)[0]
            out = torch.empty((B, P) if mode == 0 else (B, P, E), dtype=x.dtype, device=x.device)
            call("trs_pair_bilinear_fwd_mfma", ptr(x), ptr(Wt), ptr(bias_c), ptr(tasks), tasks.shape[0], int(mode), B, N, E,
                 value_dtype_code(x), ptr(out), stream_ptr())
        elif ctx.gemm:
            T = _pair_T(x, Wc)
            out = torch.empty(B, P, dtype=x.dtype, device=x.device) if mode == 0 else None
            call("trs_pair_epilogue_fwd", ptr(T), ptr(x), ptr(bias_c), 1, int(mode), B, N, E, value_dtype_code(x),
                 ptr(out), stream_ptr())
            if mode == 1:
                out = T
        else:
            out = torch.empty((B, P) if mode == 0 else (B, P, E), dtype=x.dtype, device=x.device)
            call("trs_pair_bilinear_fwd", ptr(x), ptr(Wc), 1, ptr(bias_c), 1, int(mode), B, N, E, value_dtype_code(x),
                 ptr(out), stream_ptr())
        ctx.save_for_backward(x, Wc)
        ctx.mode = int(mode)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        B, N, E = x.shape
        P = N * (N - 1) // 2
        g = g.contiguous()
        need_w = ctx.needs_input_grad[1]
        if _pair_mfma_fwd_ok(x):
            # three MFMA kernels: dL/dx_i and dL/dx_j as per-task contribution rows + one reduction, dL/dW with K = batch
            ti, si, tj, sj = _pair_tasks(N, x.device)
            Wt = W.transpose(1, 2).contiguous()
            ci = torch.empty(B, ti.shape[0], E, dtype=x.dtype, device=x.device)
            cj = torch.empty(B, tj.shape[0], E, dtype=x.dtype, device=x.device)
            gx = torch.empty_like(x)
            call("trs_pair_bilinear_bwd_data_mfma", ptr(g), ptr(x), ptr(W), ptr(Wt), ptr(ti), ti.shape[0], ptr(si), ptr(tj),
                 tj.shape[0], ptr(sj), ctx.mode, B, N, E, value_dtype_code(x), ptr(ci), ptr(cj), ptr(gx), stream_ptr())
            gW = gb = None
            if need_w:
                gW = torch.empty(P, E, E, dtype=x.dtype, device=x.device)
                ws_bytes = size_query("trs_pair_bilinear_bwd_w_mfma_workspace_bytes", B, N, E)
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
                call("trs_pair_bilinear_bwd_w_mfma", ptr(g), ptr(x), ctx.mode, B, N, E, value_dtype_code(x), ptr(gW),
                     ptr(ws), ws_bytes, stream_ptr())
            if ctx.has_bias and ctx.needs_input_grad[2]:
                gb = _pair_bias_grad(g, True)
            return gx, gW, gb, None
        if ctx.gemm:
            gT = _pair_T(x, W)                                  # recomputed, then overwritten by dL/dT in place
            gx = torch.empty_like(x)
            call("trs_pair_epilogue_bwd", ptr(g), ptr(x), ptr(gT), ctx.mode, B, N, E, value_dtype_code(x), ptr(gx),
                 stream_ptr())
            gT2 = gT.view(B, P * E)
            gxi = torch.empty(B, E, dtype=x.dtype, device=x.device)
            for i in range(N - 1):                              # dL/dx_i = dL/dT[:, pairs of i] @ Wcat_i^T
                p0, n_i = _pair_start(i, N), N - 1 - i
                Wcat = W[p0:p0 + n_i].permute(1, 0, 2).reshape(E, n_i * E)
                torch.mm(gT2[:, p0 * E:(p0 + n_i) * E], Wcat.t(), out=gxi)
                gx[:, i, :] += gxi
        else:
            gx = torch.empty_like(x)
            gT = torch.empty(B, P, E, dtype=x.dtype, device=x.device) if need_w else None
            call("trs_pair_bilinear_bwd_data", ptr(g), ptr(x), ptr(W), 1, ctx.mode, B, N, E, value_dtype_code(x), ptr(gx),
                 ptr(gT), stream_ptr())
        gW = gb = None
        if need_w:
            # dW[p] = sum_b x[b,i_p,:]^T gT[b,p,:]: for field i the pairs (i, i+1..N-1) are adjacent, so one plain GEMM
            # (E x B) @ (B x n_i*E) per field covers them (K = the batch; hipBLASLt)
            gW = torch.empty(P, E, E, dtype=x.dtype, device=x.device)
            gT2 = gT.view(B, P * E)
            for i in range(N - 1):
                p0, n_i = _pair_start(i, N), N - 1 - i
                blk = x[:, i, :].t() @ gT2[:, p0 * E:(p0 + n_i) * E]              # (E, n_i*E)
                gW[p0:p0 + n_i] = blk.view(E, n_i, E).permute(1, 0, 2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = _pair_bias_grad(g, True)
        return gx, gW, gb, None


def pair_bilinear(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], mode: int) -> torch.Tensor:
    if x.dim() != 3:
        raise ValueError(f"pair-bilinear input must be (B, N, E), got {tuple(x.shape)}")
    return _PairBilinear.apply(x, W, bias, mode)


class _AFM(Function):
    """(out (B,E), attn (B,NC2)) = attention-weighted sum of the pair products; see trs_afm_fwd_dropout.  With a ``keep``
    mask (uint8 (B,NC2)) the reference's dropout on the scores (attentional_factorization_machine.py:82) happens inside
    the pass: ``attn`` is then the dropped scores (what the reference returns) and the sum uses them."""

    @staticmethod
    def forward(ctx, x, W1, b1, w2, b2, keep=None, keep_scale=1.0):
        require_device(x, W1, b1, w2, b2, keep)
        x = x.contiguous()
        B, N, E = x.shape
        A = W1.shape[0]
        P = N * (N - 1) // 2
        ps = [t.contiguous().to(x.dtype) for t in (W1, b1, w2.reshape(-1), b2.reshape(-1))]
        out = torch.empty(B, E, dtype=x.dtype, device=x.device)
        attn = torch.empty(B, P, dtype=x.dtype, device=x.device)
        attn_drop = None
        if keep is not None:
            if keep.dtype != torch.uint8 or tuple(keep.shape) != (B, P):
                raise ValueError(f"keep mask must be uint8 of shape {(B, P)}, got {keep.dtype} {tuple(keep.shape)}")
            keep = keep.contiguous()
            attn_drop = torch.empty_like(attn)
        call("trs_afm_fwd_dropout", ptr(x), ptr(ps[0]), ptr(ps[1]), ptr(ps[2]), ptr(ps[3]), ptr(keep), float(keep_scale),
             B, N, E, A, value_dtype_code(x), ptr(out), ptr(attn), ptr(attn_drop), stream_ptr())
        ctx.save_for_backward(x, attn, keep, *ps)
        ctx.keep_scale = float(keep_scale)
        ctx.set_materialize_grads(False)
        ctx.w2_shape, ctx.b2_shape = tuple(w2.shape), tuple(b2.shape)
        return out, (attn if keep is None else attn_drop)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_attn):
        x, attn, keep, W1, b1, w2, b2 = ctx.saved_tensors
        if g_out is None and g_attn is None:
            return None, None, None, None, None, None, None
        B, N, E = x.shape
        A = W1.shape[0]
        dev = x.device
        gx = torch.empty_like(x)
        gW1 = torch.zeros(A, E, dtype=torch.float32, device=dev)
        gv = torch.zeros(2 * A + 1, dtype=torch.float32, device=dev)
        ws_bytes = size_query("trs_afm_bwd_workspace_bytes", B, N, E, A)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        go = None if g_out is None else g_out.contiguous()
        ga = None if g_attn is None else g_attn.contiguous()
        call("trs_afm_bwd_dropout", ptr(go), ptr(ga), ptr(x), ptr(attn), ptr(keep), ctx.keep_scale, ptr(W1), ptr(b1),
             ptr(w2), B, N, E, A, value_dtype_code(x), ptr(gx), ptr(gW1), ptr(gv[:A]), ptr(gv[A:2 * A]), ptr(gv[2 * A:]),
             ptr(ws), ws_bytes, stream_ptr())
        dt = x.dtype
        return (gx, gW1.to(dt), gv[:A].to(dt), gv[A:2 * A].to(dt).reshape(ctx.w2_shape),
                gv[2 * A:].to(dt).reshape(ctx.b2_shape), None, None)


def afm(x: torch.Tensor, W1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
        keep: Optional[torch.Tensor] = None, keep_scale: float = 1.0):
    """``keep`` (uint8 (B,NC2), nonzero = kept) / ``keep_scale`` (1/(1-p)): dropout on the attention scores."""
    if x.dim() != 3:
        raise ValueError(f"AFM input must be (B, N, E), got {tuple(x.shape)}")
    return _AFM.apply(x, W1, b1, w2, b2, keep, keep_scale)


# --------------------------------------------------------------------------------------------
# SENET / compose-excitation gate: out[b,m,:] = x[b,m,:] * a[b,m],  a = relu(W2 relu(W1 mean_E(x[b]) + b1) + b2)
# --------------------------------------------------------------------------------------------
def senet_fused_supported(x: torch.Tensor, W1: torch.Tensor, b1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor) -> bool:
    """True when the one-kernel family serves these operands (ReLU excitation is the caller's side of the rule): a HIP
    (B, M, E) block and four parameters of ONE dtype (fp32 / bf16), M <= 64, 1 <= H <= M, rows of whole 16-byte vectors,
    a sample of at most 16 KiB.  Decided from shapes and dtypes alone."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3 and x.dtype in (torch.float32, torch.bfloat16)):
        return False
    if any(p is None or not p.is_cuda or p.dtype != x.dtype for p in (W1, b1, W2, b2)):
        return False
    M, E = int(x.shape[1]), int(x.shape[2])
    H = int(W1.shape[0]) if W1.dim() == 2 else -1
    if tuple(W1.shape) != (H, M) or tuple(W2.shape) != (M, H) or tuple(b1.shape) != (H,) or tuple(b2.shape) != (M,):
        return False
    return bool(size_query("trs_senet_fused_supported", M, H, E, value_dtype_code(x)))


class _SENet(Function):
    """The fused family: trs_senet_fwd / trs_senet_bwd.  The gates (B,M) and hidden activations (B,H) are kept in fp32
    when a backward can follow, and not written at all otherwise."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2):
        require_device(x, W1, b1, W2, b2)
        x = x.contiguous()
        W1, b1, W2, b2 = (t.contiguous() for t in (W1, b1, W2, b2))
        B, M, E = x.shape
        H = W1.shape[0]
        out = torch.empty_like(x)
        a = h = None
        if any(ctx.needs_input_grad):
            a = torch.empty(B, M, dtype=torch.float32, device=x.device)
            h = torch.empty(B, H, dtype=torch.float32, device=x.device)
            ctx.save_for_backward(x, a, h, W1, W2)
        call("trs_senet_fwd", ptr(x), ptr(W1), ptr(b1), ptr(W2), ptr(b2), B, M, H, E, value_dtype_code(x), ptr(out),
             ptr(a), ptr(h), stream_ptr())
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, a, h, W1, W2 = ctx.saved_tensors
        B, M, E = x.shape
        H = W1.shape[0]
        need = ctx.needs_input_grad
        dev, dt = x.device, x.dtype
        dx = torch.empty_like(x) if need[0] else None
        gW1 = torch.empty(H, M, dtype=dt, device=dev) if need[1] else None
        gb1 = torch.empty(H, dtype=dt, device=dev) if need[2] else None
        gW2 = torch.empty(M, H, dtype=dt, device=dev) if need[3] else None
        gb2 = torch.empty(M, dtype=dt, device=dev) if need[4] else None
        ws, ws_bytes = None, 0
        if any(need[1:]):
            ws_bytes = size_query("trs_senet_bwd_workspace_bytes", B, M, H)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        call("trs_senet_bwd", ptr(x), ptr(g.contiguous()), ptr(a), ptr(h), ptr(W1), ptr(W2), B, M, H, E,
             value_dtype_code(x), ptr(dx), ptr(gW1), ptr(gb1), ptr(gW2), ptr(gb2), ptr(ws), ws_bytes, stream_ptr())
        return dx, gW1, gb1, gW2, gb2


def senet(x: torch.Tensor, W1: torch.Tensor, b1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """(B, M, E) -> (B, M, E): squeeze, ReLU excitation (W1 (H,M), b1 (H), W2 (M,H), b2 (M): nn.Linear layouts) and
    re-weighting in one pass.  Raises when ``senet_fused_supported`` does not hold (no fallback)."""
    x = x.rename(None) if x.has_names() else x
    if x.dim() != 3:
        raise ValueError(f"SENET input must be (B, M, E), got {tuple(x.shape)}")
    require_device(x, W1, b1, W2, b2)
    if not senet_fused_supported(x, W1, b1, W2, b2):
        raise ValueError(f"senet: shapes / dtypes outside the fused family (x {tuple(x.shape)} {x.dtype}, W1 "
                         f"{tuple(W1.shape)} {W1.dtype}); compose senet_squeeze / senet_scale instead")
    return _SENet.apply(x, W1, b1, W2, b2)


class SENetLink:
    """Ties the two ends of the general family together in the backward.  dx = g * a + gz / E needs the output gradient g
    and the gates a (known to ``senet_scale``) and gz (known to ``senet_squeeze`` once the excitation's backward has
    run): with a link, ``senet_scale``'s backward hands g and a over instead of writing g * a, and ``senet_squeeze``'s
    backward writes dx once -- no second (B, M, E) tensor and no accumulation of two input gradients.  Both calls of a
    layer's forward must use the same link, and the gates must be computed from the squeezed means."""
    __slots__ = ("z_needs_grad", "defer", "g", "a")

    def __init__(self):
        self.z_needs_grad = self.defer = False
        self.g = self.a = None


class _SENetSqueeze(Function):
    @staticmethod
    def forward(ctx, x, link):
        require_device(x)
        x = x.contiguous()
        B, M, E = x.shape
        z = torch.empty(B, M, dtype=torch.float32, device=x.device)
        call("trs_senet_squeeze", ptr(x), B, M, E, value_dtype_code(x), ptr(z), stream_ptr())
        ctx.shape, ctx.dtype, ctx.link = (B, M, E), x.dtype, link
        if link is not None:
            link.z_needs_grad = bool(ctx.needs_input_grad[0])
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        B, M, E = ctx.shape
        gz = gz.contiguous().float()
        g = a = None
        link = ctx.link
        if link is not None and link.g is not None:
            g, a, link.g, link.a = link.g, link.a, None, None
        dx = torch.empty(B, M, E, dtype=ctx.dtype, device=gz.device)
        code = _abi.TRS_F32 if ctx.dtype == torch.float32 else _abi.TRS_BF16
        call("trs_senet_scale_bwd", None, ptr(g), ptr(a), ptr(gz), B, M, E, code, None, ptr(dx), stream_ptr())
        return dx, None


class _SENetScale(Function):
    @staticmethod
    def forward(ctx, x, a, link):
        require_device(x, a)
        x = x.contiguous()
        B, M, E = x.shape
        a = a.contiguous()
        out = torch.empty_like(x)
        call("trs_senet_scale_fwd", ptr(x), ptr(a), B, M, E, value_dtype_code(x), ptr(out), stream_ptr())
        ctx.save_for_backward(x, a)
        ctx.link = link
        if link is not None:
            link.defer = bool(link.z_needs_grad and ctx.needs_input_grad[0] and ctx.needs_input_grad[1])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, a = ctx.saved_tensors
        B, M, E = x.shape
        g = g.contiguous()
        code = value_dtype_code(x)
        ga = dx = None
        if ctx.needs_input_grad[1]:
            ga = torch.empty(B, M, dtype=torch.float32, device=x.device)
            call("trs_senet_scale_bwd", ptr(x), ptr(g), None, None, B, M, E, code, ptr(ga), None, stream_ptr())
        if ctx.needs_input_grad[0]:
            link = ctx.link
            if link is not None and link.defer:
                link.g, link.a = g, a            # senet_squeeze's backward writes dx = g * a + gz / E
            else:
                dx = torch.empty_like(x)
                call("trs_senet_scale_bwd", None, ptr(g), ptr(a), None, B, M, E, code, None, ptr(dx), stream_ptr())
        return dx, ga, None


def senet_squeeze(x: torch.Tensor, link: Optional[SENetLink] = None) -> torch.Tensor:
    """(B, M, E) -> (B, M) fp32 means over E, one pass (any M, any E)."""
    x = x.rename(None) if x.has_names() else x
    if x.dim() != 3:
        raise ValueError(f"SENET input must be (B, M, E), got {tuple(x.shape)}")
    return _SENetSqueeze.apply(x, link)


def senet_scale(x: torch.Tensor, a: torch.Tensor, link: Optional[SENetLink] = None) -> torch.Tensor:
    """out[b,m,:] = x[b,m,:] * a[b,m] with fp32 gates a (B, M), one pass; the gradient of a is sum_e g * x (fp32)."""
    x = x.rename(None) if x.has_names() else x
    a = a.rename(None) if a.has_names() else a
    if x.dim() != 3 or tuple(a.shape) != tuple(x.shape[:2]) or a.dtype != torch.float32:
        raise ValueError(f"senet_scale: x (B, M, E) and fp32 gates (B, M) expected, got {tuple(x.shape)} and "
                         f"{tuple(a.shape)} {a.dtype}")
    return _SENetScale.apply(x, a, link)


# --------------------------------------------------------------------------------------------
# Mixture-of-experts gating: out[b,g,k] = softmax_k(x W_g^T + b_g)[b,k] * experts[b,k]
# --------------------------------------------------------------------------------------------
MOE_GATE_MAX_K = 1024      # widest row of the kernels' vector path (moe.hip: 64 lanes x 16 columns); wider rows take the element path


MOE_PATH_VECTOR, MOE_PATH_ELEMENT = 1, 2


def moe_gate_last_path() -> int:
    """The branch the last trs_moe_gate_fwd / _bwd launch of this thread took, as the library recorded it where it
    launched: MOE_PATH_VECTOR, MOE_PATH_ELEMENT, or 0 before the first launch (tests and diagnostics)."""
    return size_query("trs_moe_gate_last_path")


def _moe_gate_operands(logits, bias, experts, gout=None):
    for name, t in (("logits", logits), ("bias", bias), ("experts", experts), ("gout", gout)):
        if t is not None and not t.is_contiguous():      # the entries read dense rows: a strided operand would be misread
            raise ValueError(f"moe_gate: {name} must be contiguous, got strides {tuple(t.stride())} for {tuple(t.shape)}")
    require_device(logits, bias, experts, gout)
    if logits.dim() != 2 or experts.dim() != 2 or logits.dtype != torch.float32 or logits.shape[0] != experts.shape[0]:
        raise ValueError(f"moe_gate: fp32 logits (B, G*K) and experts (B, K) expected, got {tuple(logits.shape)} "
                         f"{logits.dtype} and {tuple(experts.shape)}")
    B, K = experts.shape
    if K < 1 or logits.shape[1] < K or logits.shape[1] % K != 0:
        raise ValueError(f"moe_gate: logits of width {logits.shape[1]} are not G rows of K = {K} expert outputs")
    G = logits.shape[1] // K
    if bias is not None and (tuple(bias.shape) != (G * K,) or bias.dtype != experts.dtype):
        raise ValueError(f"moe_gate: bias ({G * K},) of {experts.dtype} expected, got {tuple(bias.shape)} {bias.dtype}")
    if gout is not None and (tuple(gout.shape) != (B, G, K) or gout.dtype != experts.dtype):
        raise ValueError(f"moe_gate: output gradient ({B}, {G}, {K}) of {experts.dtype} expected, got "
                         f"{tuple(gout.shape)} {gout.dtype}")
    return B, G, K


def moe_gate_forward_raw(logits: torch.Tensor, bias: Optional[torch.Tensor], experts: torch.Tensor) -> torch.Tensor:
    """trs_moe_gate_fwd as it is (no autograd): fp32 logits (B, G*K) WITHOUT bias, bias (G*K) or None, experts (B, K)
    -> (B, G, K) of the experts' dtype.  A non-contiguous operand raises ValueError."""
    B, G, K = _moe_gate_operands(logits, bias, experts)
    out = torch.empty(B, G, K, dtype=experts.dtype, device=experts.device)
    call("trs_moe_gate_fwd", ptr(logits), ptr(bias), ptr(experts), B, G, K, value_dtype_code(experts), ptr(out),
         stream_ptr())
    return out


def moe_gate_backward_raw(logits: torch.Tensor, bias: Optional[torch.Tensor], experts: torch.Tensor,
                          gout: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """trs_moe_gate_bwd as it is: -> glogits (B, G*K), gexperts (B, K), both of the experts' dtype."""
    B, G, K = _moe_gate_operands(logits, bias, experts, gout)
    glogits = torch.empty(B, G * K, dtype=experts.dtype, device=experts.device)
    gexperts = torch.empty_like(experts)
    call("trs_moe_gate_bwd", ptr(logits), ptr(bias), ptr(experts), ptr(gout), B, G, K, value_dtype_code(experts),
         ptr(glogits), ptr(gexperts), stream_ptr())
    return glogits, gexperts


class _MoEGate(Function):
    """The gate GEMM stays inside the node: its result is fp32 (logits rounded to bf16 cost 0.5-2e-2 of the output), while
    the gradient of the logits has to be of the value dtype for the two gradient GEMMs."""

    @staticmethod
    def forward(ctx, x, weight, bias, experts):
        experts = experts.contiguous()
        weight = weight.contiguous()
        bias = bias.contiguous() if bias is not None else None
        if x.dtype == torch.float32:
            logits = torch.mm(x, weight.t())
        else:
            logits = torch.mm(x, weight.t(), out_dtype=torch.float32)
        out = moe_gate_forward_raw(logits, bias, experts)
        ctx.save_for_backward(x, weight, bias, logits, experts)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, weight, bias, logits, experts = ctx.saved_tensors
        need = ctx.needs_input_grad
        glogits, gexperts = moe_gate_backward_raw(logits, bias, experts, g.contiguous())
        gx = torch.mm(glogits, weight) if need[0] else None
        gw = torch.mm(glogits.t(), x) if need[1] else None
        gb = glogits.sum(dim=0, dtype=torch.float32).to(bias.dtype) if bias is not None and need[2] else None
        return gx, gw, gb, gexperts if need[3] else None


def moe_gate(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], experts: torch.Tensor) -> torch.Tensor:
    """(B, D) input, stacked gate weights (G*K, D) and biases (G*K) or None (nn.Linear layouts, gate after gate), experts
    (B, K) -> (B, G, K):  out[b,g,:] = softmax(x W_g^T + b_g) * experts[b].  One GEMM with an fp32 result, then one kernel;
    the backward is one kernel, two GEMMs and the bias sum.  All operands of one dtype (fp32 / bf16)."""
    x, weight, experts = (t.rename(None) if t.has_names() else t for t in (x, weight, experts))
    require_device(x, weight, bias, experts)
    if x.dim() != 2 or weight.dim() != 2 or experts.dim() != 2 or weight.shape[1] != x.shape[1]:
        raise ValueError(f"moe_gate: x (B, D), weight (G*K, D) and experts (B, K) expected, got {tuple(x.shape)}, "
                         f"{tuple(weight.shape)} and {tuple(experts.shape)}")
    K = experts.shape[1]
    if K < 1 or weight.shape[0] < K or weight.shape[0] % K != 0 or experts.shape[0] != x.shape[0]:
        raise ValueError(f"moe_gate: weight of {weight.shape[0]} rows is not G gates over the K = {K} expert outputs of "
                         f"{experts.shape[0]} samples (x has {x.shape[0]})")
    if weight.dtype != x.dtype or experts.dtype != x.dtype or (bias is not None and bias.dtype != x.dtype):
        raise TypeError(f"moe_gate: operands of one dtype expected, got x {x.dtype}, weight {weight.dtype}, bias "
                        f"{None if bias is None else bias.dtype}, experts {experts.dtype}")
    value_dtype_code(x)
    return _MoEGate.apply(x, weight, bias, experts)


# --------------------------------------------------------------------------------------------
# Behaviour-to-interest dynamic routing (MIND): out = squash(sum_n softmax_k(noise + c) (x @ S))
# --------------------------------------------------------------------------------------------
ROUTING_PATH_VECTOR, ROUTING_PATH_ELEMENT = 1, 2


def dynamic_routing_path(N: int, R: int, K: int, dtype: torch.dtype) -> int:
    """0: no fused kernel for this shape (callers keep the ATen composition), ROUTING_PATH_VECTOR: rows of whole 16-byte
    vectors, ROUTING_PATH_ELEMENT: element loads (trs_dynamic_routing_path; a pure function, callable without a device).
    Covered: 1 <= N <= 128, 1 <= R <= 128, 1 <= K <= 8, fp32 / bf16."""
    if dtype not in (torch.float32, torch.bfloat16):
        return 0
    code = _abi.TRS_F32 if dtype == torch.float32 else _abi.TRS_BF16
    return size_query("trs_dynamic_routing_path", int(N), int(R), int(K), code)


def _routing_operands(noise, priors=None, c=None, z=None, gout=None):
    for name, t in (("priors", priors), ("noise", noise), ("c", c), ("z", z), ("gout", gout)):
        if t is not None and not t.is_contiguous():      # the entries read dense rows: a strided operand would be misread
            raise ValueError(f"dynamic_routing: {name} must be contiguous, got strides {tuple(t.stride())} for "
                             f"{tuple(t.shape)}")
    require_device(noise, priors, c, z, gout)
    if noise.dim() != 4:
        raise ValueError(f"dynamic_routing: noise (B, K, N, R) expected, got {tuple(noise.shape)}")
    B, K, N, R = noise.shape
    for name, t, shape, dtype in (("priors", priors, (B, N, R), torch.float32), ("c", c, (B, K, N), torch.float32),
                                  ("z", z, (B, K, R), torch.float32), ("gout", gout, (B, K, R), noise.dtype)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype):
            raise ValueError(f"dynamic_routing: {name} {shape} of {dtype} expected, got {tuple(t.shape)} {t.dtype}")
    code = value_dtype_code(noise)
    if dynamic_routing_path(N, R, K, noise.dtype) == 0:
        raise NotImplementedError(f"torecsys_amd: dynamic_routing does not cover N={N}, R={R}, K={K} "
                                  f"(1 <= N <= 128, 1 <= R <= 128, 1 <= K <= 8)")
    return B, K, N, R, code


def dynamic_routing_forward_raw(priors: torch.Tensor, noise: torch.Tensor, num_iter: int, save: bool = False):
    """trs_dynamic_routing_fwd as it is (no autograd): fp32 priors (B, N, R), noise (B, K, N, R) of the value dtype ->
    out (B, K, R) of the value dtype; with ``save`` also the fp32 routing sum c (B, K, N) and z (B, K, R) the backward
    reads.  A non-contiguous operand raises ValueError."""
    B, K, N, R, code = _routing_operands(noise, priors=priors)
    if int(num_iter) < 1:
        raise ValueError(f"dynamic_routing: num_iter >= 1 expected, got {num_iter}")
    out = torch.empty(B, K, R, dtype=noise.dtype, device=noise.device)
    c = torch.empty(B, K, N, dtype=torch.float32, device=noise.device) if save else None
    z = torch.empty(B, K, R, dtype=torch.float32, device=noise.device) if save else None
    call("trs_dynamic_routing_fwd", ptr(priors), ptr(noise), B, N, R, K, int(num_iter), code, ptr(out), ptr(c), ptr(z),
         stream_ptr())
    return (out, c, z) if save else out


def dynamic_routing_backward_raw(noise: torch.Tensor, c: torch.Tensor, z: torch.Tensor, gout: torch.Tensor) -> torch.Tensor:
    """trs_dynamic_routing_bwd as it is: noise, the forward's c and z, gout (B, K, R) -> dpri (B, N, R) of the value
    dtype."""
    B, K, N, R, code = _routing_operands(noise, c=c, z=z, gout=gout)
    dpri = torch.empty(B, N, R, dtype=noise.dtype, device=noise.device)
    call("trs_dynamic_routing_bwd", ptr(noise), ptr(c), ptr(z), ptr(gout), B, N, R, K, code, ptr(dpri), stream_ptr())
    return dpri


class _DynamicRouting(Function):
    """The projection stays inside the node, as the gate GEMM of _MoEGate: the priors are the GEMM's fp32 result (rounded
    to bf16 they move the output by 1e-2 at 3 iterations and 5e-2 at 5), and the gradient of the priors is of the value
    dtype for the two gradient GEMMs.  Saved: x, S, the noise, c (B, K, N) and z (B, K, R) -- no priors."""

    @staticmethod
    def forward(ctx, x, S, noise, num_iter):
        B, N, E = x.shape
        x2 = x.reshape(B * N, E)
        S = S.contiguous()
        if x.dtype == torch.float32:
            priors = torch.mm(x2, S)
        else:
            priors = torch.mm(x2, S, out_dtype=torch.float32)
        out, c, z = dynamic_routing_forward_raw(priors.view(B, N, S.shape[1]), noise.contiguous(), num_iter, save=True)
        ctx.save_for_backward(x, S, noise, c, z)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, S, noise, c, z = ctx.saved_tensors
        need = ctx.needs_input_grad
        B, N, E = x.shape
        dpri = dynamic_routing_backward_raw(noise.contiguous(), c, z, g.contiguous()).view(B * N, S.shape[1])
        gx = torch.mm(dpri, S.t()).view(B, N, E) if need[0] else None
        gS = torch.mm(x.reshape(B * N, E).t(), dpri) if need[1] else None
        return gx, gS, None, None


def dynamic_routing(x: torch.Tensor, S: torch.Tensor, noise: torch.Tensor, num_iter: int) -> torch.Tensor:
    """(B, N, E) behaviours, projection S (E, R), coupling noise (B, K', N, R) -> (B, K', R) interest capsules after
    ``num_iter`` rounds of MIND's behaviour-to-interest routing (K' is the noise's; the routing loop runs on detached
    priors, the noise receives no gradient).  One GEMM with an fp32 result and one kernel; the backward is one kernel and
    two GEMMs.  All operands of one dtype (fp32 / bf16); raises for shapes ``dynamic_routing_path`` refuses."""
    x, S, noise = (t.rename(None) if t.has_names() else t for t in (x, S, noise))
    if x.dim() != 3 or S.dim() != 2 or noise.dim() != 4 or S.shape[0] != x.shape[2]:
        raise ValueError(f"dynamic_routing: x (B, N, E), S (E, R) and noise (B, K, N, R) expected, got {tuple(x.shape)}, "
                         f"{tuple(S.shape)} and {tuple(noise.shape)}")
    B, N, _ = x.shape
    if noise.shape[0] != B or noise.shape[2] != N or noise.shape[3] != S.shape[1]:
        raise ValueError(f"dynamic_routing: noise ({B}, K, {N}, {S.shape[1]}) expected, got {tuple(noise.shape)}")
    if S.dtype != x.dtype or noise.dtype != x.dtype:
        raise TypeError(f"dynamic_routing: operands of one dtype expected, got x {x.dtype}, S {S.dtype}, noise "
                        f"{noise.dtype}")
    if int(num_iter) < 1:
        raise ValueError(f"dynamic_routing: num_iter >= 1 expected, got {num_iter}")
    require_device(x, S, noise)
    value_dtype_code(x)
    if dynamic_routing_path(N, S.shape[1], noise.shape[1], x.dtype) == 0:
        raise NotImplementedError(f"torecsys_amd: dynamic_routing does not cover N={N}, R={S.shape[1]}, "
                                  f"K={noise.shape[1]} (1 <= N <= 128, 1 <= R <= 128, 1 <= K <= 8)")
    return _DynamicRouting.apply(x, S, noise, int(num_iter))


# --------------------------------------------------------------------------------------------
# An ordered (B, L) list of ids through a one-layer RNN / LSTM / GRU, pooled over the live steps
# --------------------------------------------------------------------------------------------
SEQ_RNN_CELLS = {"rnn": 0, "lstm": 1, "gru": 2}
SEQ_RNN_GATES = {0: 1, 1: 4, 2: 3}
SEQ_RNN_MODES = {"avg": (0, 1), "sum": (0, 0), "none": (1, 0)}      # name -> (kernel mode, average)
SEQ_RNN_PATH_VECTOR, SEQ_RNN_PATH_MATRIX = 1, 2


def _seq_cell_code(cell) -> int:
    if isinstance(cell, str):
        if cell not in SEQ_RNN_CELLS:
            raise ValueError(f'seq_rnn: cell must be one of {sorted(SEQ_RNN_CELLS)}, got {cell!r}')
        return SEQ_RNN_CELLS[cell]
    return int(cell)


def seq_rnn_path(cell, L: int, E: int, dtype: torch.dtype) -> int:
    """0: no fused kernel for this cell / shape / dtype (callers keep the composition); SEQ_RNN_PATH_VECTOR: the fp32-FMA
    kernels (fp32 or bf16 operands, 1 <= E <= 128, any L >= 1); SEQ_RNN_PATH_MATRIX: the matrix-core kernels (bf16, E in
    {16, 32, 64}, any L >= 1).  trs_seq_rnn_path; a pure function, callable without a device.  ``cell``: 'rnn' | 'lstm' |
    'gru' or its code."""
    if dtype not in (torch.float32, torch.bfloat16):
        return 0
    code = _abi.TRS_F32 if dtype == torch.float32 else _abi.TRS_BF16
    return size_query("trs_seq_rnn_path", _seq_cell_code(cell), int(L), int(E), code)


def _seq_operands(weight, idx, lengths, w_ih, w_hh, b_ih, b_hh, cell, **more):
    named = dict(weight=weight, idx=idx, lengths=lengths, w_ih=w_ih, w_hh=w_hh, b_ih=b_ih, b_hh=b_hh, **more)
    for name, t in named.items():
        if t is not None and not t.is_contiguous():      # the entries read dense rows: a strided operand would be misread
            raise ValueError(f"seq_rnn: {name} must be contiguous, got strides {tuple(t.stride())} for {tuple(t.shape)}")
    require_device(*named.values())
    if weight.dim() != 2 or idx.dim() != 2 or idx.shape[1] < 1:
        raise ValueError(f"seq_rnn: weight (V, E) and idx (B, L >= 1) expected, got {tuple(weight.shape)} and "
                         f"{tuple(idx.shape)}")
    (V, E), (B, L) = weight.shape, idx.shape
    cell = _seq_cell_code(cell)
    if cell not in SEQ_RNN_GATES:
        raise ValueError(f"seq_rnn: bad cell code {cell}")
    GE = SEQ_RNN_GATES[cell] * E
    if tuple(lengths.shape) != (B,):
        raise ValueError(f"seq_rnn: lengths ({B},) expected, got {tuple(lengths.shape)}")
    for name, t, shape in (("w_ih", w_ih, (GE, E)), ("w_hh", w_hh, (GE, E)), ("b_ih", b_ih, (GE,)), ("b_hh", b_hh, (GE,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"seq_rnn: {name} {shape} expected, got {tuple(t.shape)}")
        if t.dtype != weight.dtype:
            raise TypeError(f"seq_rnn: {name} must have the table's dtype {weight.dtype}, got {t.dtype}")
    code = value_dtype_code(weight)
    if seq_rnn_path(cell, L, E, weight.dtype) == 0:
        raise NotImplementedError(f"torecsys_amd: seq_rnn does not cover L={L}, E={E}, {weight.dtype} (L >= 1, 1 <= E <= 128, "
                                  f"fp32 / bf16)")
    return V, E, B, L, GE, cell, code


def _seq_workspace(cell: int, E: int, dev) -> Tuple[torch.Tensor, int]:
    ws_bytes = size_query("trs_seq_rnn_workspace_bytes", cell, E)
    return torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev), ws_bytes


def seq_rnn_forward_raw(weight: torch.Tensor, idx: torch.Tensor, lengths: torch.Tensor, w_ih: torch.Tensor,
                        w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor, cell, mode: int, average: bool = True,
                        save: bool = False, flag: Optional[_ErrFlag] = None):
    """trs_seq_rnn_fwd as it is (no autograd).  ``mode`` 0: (B, E) = scale * sum of the live h_t, 1: (B, L, E) every h_t.
    Returns ``(out, scale, h_save, c_save)``: the one-float device scale (1 / max(lengths) with ``average``, else 1) and,
    with ``save``, what the backward reads -- h (B, L, E) of the value dtype (``out`` itself in mode 1) and the LSTM's fp32
    c (B, L, E), else None.  A non-contiguous operand raises ValueError."""
    V, E, B, L, GE, cell, code = _seq_operands(weight, idx, lengths, w_ih, w_hh, b_ih, b_hh, cell)
    if mode not in (0, 1):
        raise ValueError(f"seq_rnn: mode 0 or 1 expected, got {mode}")
    dev = weight.device
    out = torch.empty((B, E) if mode == 0 else (B, L, E), dtype=weight.dtype, device=dev)
    scale = torch.empty(1, dtype=torch.float32, device=dev)
    h = torch.empty(B, L, E, dtype=weight.dtype, device=dev) if save and mode == 0 else None
    c = torch.empty(B, L, E, dtype=torch.float32, device=dev) if save and cell == SEQ_RNN_CELLS["lstm"] else None
    ws, ws_bytes = _seq_workspace(cell, E, dev)
    call("trs_seq_rnn_fwd", ptr(weight), V, E, code, ptr(idx), index_dtype_code(idx), ptr(lengths),
         index_dtype_code(lengths), B, L, ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), cell, mode, int(bool(average)),
         ptr(scale), ptr(out), ptr(h), ptr(c), ptr(ws), ws_bytes, ptr(flag.t if flag is not None else None), stream_ptr())
    return out, scale, (out if save and mode == 1 else h), c


def seq_rnn_backward_raw(weight: torch.Tensor, idx: torch.Tensor, lengths: torch.Tensor, w_ih: torch.Tensor,
                         w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor, cell, mode: int, scale: torch.Tensor,
                         h: torch.Tensor, c: Optional[torch.Tensor], gout: torch.Tensor):
    """trs_seq_rnn_bwd as it is: the forward's operands, scale and saved state, gout (B, E) for mode 0 / (B, L, E) for
    mode 1 -> ``(dgates, dgates_h)``, both (B, L, G E) of the value dtype; ``dgates_h`` is ``dgates`` itself except for the
    GRU (whose n block differs on the hidden side)."""
    V, E, B, L, GE, cell, code = _seq_operands(weight, idx, lengths, w_ih, w_hh, b_ih, b_hh, cell, scale=scale, h=h, c=c,
                                               gout=gout)
    if mode not in (0, 1):
        raise ValueError(f"seq_rnn: mode 0 or 1 expected, got {mode}")
    lstm, gru = cell == SEQ_RNN_CELLS["lstm"], cell == SEQ_RNN_CELLS["gru"]
    for name, t, shape, dtype in (("scale", scale, (1,), torch.float32), ("h", h, (B, L, E), weight.dtype),
                                  ("c", c, (B, L, E), torch.float32),
                                  ("gout", gout, (B, E) if mode == 0 else (B, L, E), weight.dtype)):
        if t is None and (name != "c" or lstm):
            raise ValueError(f"seq_rnn: {name} is required")
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype):
            raise ValueError(f"seq_rnn: {name} {shape} of {dtype} expected, got {tuple(t.shape)} {t.dtype}")
    dev = weight.device
    dgates = torch.empty(B, L, GE, dtype=weight.dtype, device=dev)
    dgates_h = torch.empty(B, L, GE, dtype=weight.dtype, device=dev) if gru else None
    ws, ws_bytes = _seq_workspace(cell, E, dev)
    call("trs_seq_rnn_bwd", ptr(weight), V, E, code, ptr(idx), index_dtype_code(idx), ptr(lengths),
         index_dtype_code(lengths), B, L, ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), cell, mode, ptr(scale), ptr(h),
         ptr(c if lstm else None), ptr(gout), ptr(dgates), ptr(dgates_h), ptr(ws), ws_bytes, stream_ptr())
    return dgates, (dgates_h if gru else dgates)


class _SeqRNN(Function):
    """One kernel per direction for the chain; the sums over the batch are GEMMs here, as in _DynamicRouting and _MoEGate:
    dX = dgates W_ih (-> the row-bucket walk), dW_ih = dgates^T X with X gathered again (the forward never formed it),
    dW_hh = dgates_h^T H_prev with H_prev the saved h shifted by one step, the biases as column sums.  The list positions
    from a sample's length on are masked to the padding id for the gather and the walk: their dgates rows are zero, and
    whatever ids sit there are never looked up."""

    @staticmethod
    def forward(ctx, weight, idx, lengths, w_ih, w_hh, b_ih, b_hh, cell, mode, average, padding_idx):
        w, wi, wh, bi, bh = (t.contiguous() for t in (weight, w_ih, w_hh, b_ih, b_hh))
        V, E = w.shape
        L = idx.shape[1]
        need = ctx.needs_input_grad
        ctx.empty = idx.shape[0] == 0
        save = any(need) and not ctx.empty
        flag = _ErrFlag(w.device)
        out, scale, h, c = seq_rnn_forward_raw(w, idx, lengths, wi, wh, bi, bh, cell, mode, average, save=save, flag=flag)
        flag.check("seq_rnn")
        ctx.cell, ctx.mode = cell, mode
        ctx.padding_idx = -1 if padding_idx is None else int(padding_idx)
        ctx.skip = _skip_row(ctx.padding_idx, V)
        if save:
            idx_m = None
            if need[0] or need[3]:
                live = torch.arange(L, device=idx.device).unsqueeze(0) < lengths.unsqueeze(1)
                idx_m = torch.where(live, idx, torch.full_like(idx, ctx.skip if ctx.skip is not None else 0))
                if need[0] and not torch.cuda.is_current_stream_capturing():
                    # (a capture stays one chain on one stream: the backward then builds the buckets in line)
                    prefetch_row_buckets(idx_m, None, V, skip_row=ctx.skip)
            ctx.has_idx_m, ctx.has_c = idx_m is not None, c is not None
            extra = [t for t in (idx_m, c) if t is not None]
            ctx.save_for_backward(idx, lengths, weight, w_ih, w_hh, b_ih, b_hh, scale, h, *extra)
        elif ctx.empty:
            ctx.save_for_backward(weight, w_ih, w_hh, b_ih, b_hh)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if ctx.empty:      # no sample: zero gradients
            zeros = [torch.zeros_like(t) if n else None
                     for t, n in zip(ctx.saved_tensors, (ctx.needs_input_grad[0],) + tuple(ctx.needs_input_grad[3:7]))]
            return (zeros[0], None, None, *zeros[1:], None, None, None, None)
        idx, lengths, weight, w_ih, w_hh, b_ih, b_hh, scale, h = ctx.saved_tensors[:9]
        extra = list(ctx.saved_tensors[9:])
        idx_m = extra.pop(0) if ctx.has_idx_m else None
        c = extra.pop(0) if ctx.has_c else None
        _adopt_grads(g)
        need = ctx.needs_input_grad
        V, E = weight.shape
        B, L = idx.shape
        w, wi, wh, bi, bh = (t.contiguous() for t in (weight, w_ih, w_hh, b_ih, b_hh))
        dgates, dgates_h = seq_rnn_backward_raw(w, idx, lengths, wi, wh, bi, bh, ctx.cell, ctx.mode, scale, h, c,
                                                g.contiguous())
        GE = dgates.shape[2]
        dg, dgh = dgates.view(B * L, GE), dgates_h.view(B * L, GE)
        g_w = g_wih = g_whh = g_bih = g_bhh = None
        if need[3]:
            x = torch.empty(B, L, E, dtype=w.dtype, device=w.device)
            # the gather range-checks only when it is handed a flag (rows out of range then read as zeros, as in the
            # forward, which has reported them already: this one is not read back)
            call("trs_gather_rows", ptr(w), V, E, value_dtype_code(w), ptr(idx_m), index_dtype_code(idx_m), None, B, L,
                 ptr(x), ptr(_ErrFlag(w.device).t), stream_ptr())
            g_wih = torch.mm(dg.t(), x.view(B * L, E))
        if need[4]:
            h_prev = torch.cat([h.new_zeros(B, 1, E), h[:, :-1]], dim=1)
            g_whh = torch.mm(dgh.t(), h_prev.view(B * L, E))
        if need[5]:
            g_bih = dg.sum(0)
        if need[6]:
            g_bhh = dgh.sum(0)
        if need[0]:
            dx = torch.mm(dg, wi).view(B, L, E)
            rb = row_buckets(idx_m, None, V, skip_row=ctx.skip)
            g_w = scatter_rows(rb, weight, g_rows=dx, padding_row=ctx.padding_idx)
        return g_w, None, None, g_wih, g_whh, g_bih, g_bhh, None, None, None, None


def seq_rnn(weight: torch.Tensor, idx: torch.Tensor, lengths: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor,
            b_ih: torch.Tensor, b_hh: torch.Tensor, cell: str = "lstm", mode: str = "avg",
            padding_idx: Optional[int] = None) -> torch.Tensor:
    """The looked-up rows of an ordered, padded (B, L) list of ids through a one-layer ``cell`` ('rnn' | 'lstm' | 'gru',
    hidden size E, PyTorch's parameter layout) over the first ``lengths[b]`` steps of every sample, in one HIP pass per
    direction (csrc/seq_rnn.hip).  ``mode``: 'avg' -> (B, 1, E), the sum of the live h_t over ``max(lengths)`` (the
    divisor pad_packed_sequence leaves the reference's pooling with; read on the device); 'sum' -> (B, 1, E) unscaled;
    'none' -> (B, L, E), zeros from each sample's length on.  No sort, no packing and no host read of the lengths: the
    call can be captured in a graph.  ``padding_idx``: the table row that receives no gradient.  All parameters of the
    table's dtype (fp32 / bf16); raises NotImplementedError for what ``seq_rnn_path`` refuses."""
    if mode not in SEQ_RNN_MODES:
        raise ValueError(f'seq_rnn: mode must be one of {sorted(SEQ_RNN_MODES)}, got {mode!r}')
    code = _seq_cell_code(cell)
    idx = _as_index(idx)
    lengths = _as_index(lengths)
    w_ih, w_hh, b_ih, b_hh = (t.rename(None) if t.has_names() else t for t in (w_ih, w_hh, b_ih, b_hh))
    # shapes and dtypes are checked before the node is built (contiguity is the node's own business)
    _seq_operands(weight.contiguous(), idx, lengths, w_ih.contiguous(), w_hh.contiguous(), b_ih.contiguous(),
                  b_hh.contiguous(), code)
    if padding_idx is not None and padding_idx < 0:
        padding_idx = weight.shape[0] + padding_idx
    kmode, average = SEQ_RNN_MODES[mode]
    out = _SeqRNN.apply(weight, idx, lengths, w_ih, w_hh, b_ih, b_hh, code, kmode, bool(average), padding_idx)
    return out.unsqueeze(1) if kmode == 0 else out


# --------------------------------------------------------------------------------------------
# K3: field-aware FM pair products
# --------------------------------------------------------------------------------------------
class _FFM(Function):
    @staticmethod
    def forward(ctx, x, num_fields):
        require_device(x)
        x = x.contiguous()
        B, NN, E = x.shape
        N = num_fields
        out = torch.empty(B, N * (N - 1) // 2, E, dtype=x.dtype, device=x.device)
        call("trs_ffm_fwd", ptr(x), B, N, E, value_dtype_code(x), ptr(out), stream_ptr())
        ctx.save_for_backward(x)
        ctx.N = N
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        B, NN, E = x.shape
        dx = torch.empty_like(x)
        call("trs_ffm_bwd", ptr(x), ptr(g.contiguous()), B, ctx.N, E, value_dtype_code(x), ptr(dx), stream_ptr())
        return dx, None


def ffm_layer(x: torch.Tensor, num_fields: int) -> torch.Tensor:
    if x.dim() != 3 or x.shape[1] != num_fields * num_fields:
        raise ValueError(f"FFM input must be (B, N*N={num_fields * num_fields}, E), got {tuple(x.shape)}")
    return _FFM.apply(x, num_fields)


# --------------------------------------------------------------------------------------------
# K4: cross network
# --------------------------------------------------------------------------------------------
class _Cross(Function):
    @staticmethod
    def forward(ctx, x, W, b, detach_first):
        require_device(x, W, b)
        x = x.contiguous()
        L, E, _ = W.shape
        rows = x.numel() // E
        Wc = W.to(x.dtype).contiguous()
        bc = b.to(x.dtype).contiguous()
        out = torch.empty_like(x)
        ws_bytes = size_query("trs_cross_workspace_bytes", rows, E, L, value_dtype_code(x))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
        call("trs_cross_fwd", ptr(x), ptr(Wc), ptr(bc), rows, E, L, value_dtype_code(x), ptr(out), ptr(ws), ws_bytes,
             stream_ptr())
        ctx.save_for_backward(x, Wc, bc)
        ctx.detach_first = bool(detach_first)
        ctx.param_dtypes = (W.dtype, b.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, Wc, bc = ctx.saved_tensors
        L, E, _ = Wc.shape
        rows = x.numel() // E
        dx = torch.empty_like(x)
        dW = torch.zeros(L, E, E, dtype=torch.float32, device=x.device)
        db = torch.zeros(L, E, dtype=torch.float32, device=x.device)
        ws_bytes = size_query("trs_cross_workspace_bytes", rows, E, L, value_dtype_code(x))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
        call("trs_cross_bwd", ptr(x), ptr(Wc), ptr(bc), ptr(g.contiguous()), rows, E, L, value_dtype_code(x),
             1 if ctx.detach_first else 0, ptr(dx), ptr(dW), ptr(db), ptr(ws), ws_bytes, stream_ptr())
        return dx, dW.to(ctx.param_dtypes[0]), db.to(ctx.param_dtypes[1]), None


def cross_network(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, detach_first: bool = True) -> torch.Tensor:
    """x: (..., E); W: (L,E,E) stacked nn.Linear weights; b: (L,E)."""
    if W.dim() != 3 or W.shape[1] != W.shape[2] or x.shape[-1] != W.shape[1] or b.shape != W.shape[:2]:
        raise ValueError(f"cross_network: bad shapes x{tuple(x.shape)} W{tuple(W.shape)} b{tuple(b.shape)}")
    return _Cross.apply(x, W, b, detach_first)


# --------------------------------------------------------------------------------------------
# K5: CIN contraction  y[b,c,e] = bias[c] + sum_{n,h} Wc[c,n*H+h] x0[b,n,e] xk[b,h,e]
# --------------------------------------------------------------------------------------------
class _CINContract(Function):
    @staticmethod
    def forward(ctx, x0, xk, Wc, bias):
        require_device(x0, xk, Wc, bias)
        x0 = x0.contiguous()
        xk = xk.contiguous()
        B, N, E = x0.shape
        H = xk.shape[1]
        C = Wc.shape[0]
        w = Wc.to(x0.dtype).contiguous()
        bb = None if bias is None else bias.to(x0.dtype).contiguous()
        y = torch.empty(B, C, E, dtype=x0.dtype, device=x0.device)
        call("trs_cin_fwd", ptr(x0), ptr(xk), ptr(w), ptr(bb), B, N, H, C, E, value_dtype_code(x0), ptr(y), ptr(None),
             stream_ptr())
        ctx.save_for_backward(x0, xk, w)
        ctx.meta = (Wc.dtype, None if bias is None else bias.dtype)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x0, xk, w = ctx.saved_tensors
        B, N, E = x0.shape
        H, C = xk.shape[1], w.shape[0]
        gy = gy.contiguous()
        need_x0, need_xk, need_w, need_b = ctx.needs_input_grad
        dW = torch.zeros(C, N * H, dtype=torch.float32, device=x0.device) if need_w else None
        dx0 = torch.empty_like(x0) if need_x0 else None
        dxk = torch.empty_like(xk) if need_xk else None
        call("trs_cin_bwd", ptr(x0), ptr(xk), ptr(w), ptr(gy), B, N, H, C, E, value_dtype_code(x0), ptr(dW), ptr(dx0),
             ptr(dxk), 0, stream_ptr())
        db = gy.float().sum(dim=(0, 2)).to(ctx.meta[1]) if (need_b and ctx.meta[1] is not None) else None
        return dx0, dxk, (dW.to(ctx.meta[0]) if need_w else None), db


def cin_contract(x0: torch.Tensor, xk: torch.Tensor, Wc: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """x0 (B,N,E), xk (B,H,E), Wc (C,N*H) -> y (B,C,E); the (B,N*H,E) outer product is never materialised."""
    if x0.dim() != 3 or xk.dim() != 3 or x0.shape[0] != xk.shape[0] or x0.shape[2] != xk.shape[2]:
        raise ValueError(f"cin_contract: bad shapes x0{tuple(x0.shape)} xk{tuple(xk.shape)}")
    if Wc.dim() != 2 or Wc.shape[1] != x0.shape[1] * xk.shape[1]:
        raise ValueError(f"cin_contract: Wc must be (C, N*H={x0.shape[1] * xk.shape[1]}), got {tuple(Wc.shape)}")
    return _CINContract.apply(x0, xk, Wc, bias)


# --------------------------------------------------------------------------------------------
# K5, channels-last (MFMA) form: x0T (B,E,ld0), xkT (B,E,>=H) view, -> yT (B,E,C)
# --------------------------------------------------------------------------------------------
def cin_cl_supported(x: torch.Tensor, out_channels: Sequence[int], hidden_sizes: Sequence[int]) -> bool:
    """Whole-stack check for the channels-last MFMA path: bf16 on device, E % 16 == 0, every layer's
    C % 32 == 0, field count N <= 256, hidden widths multiples of 32 in {32,64,128,256}."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 16 == 0 and x.shape[1] <= 256):
        return False
    if any(c % 32 != 0 for c in out_channels):
        return False
    return all(h in (32, 64, 128, 256) for h in hidden_sizes)


# the last CIN layer's backward leaves out the output channels that provably carry no gradient (see _CINContractCL.forward)
CIN_SKIP_DEAD = os.environ.get("TRS_CIN_SKIP_DEAD", "1") != "0"


def cin_fold_symmetric(Wc: torch.Tensor, N: int) -> torch.Tensor:
    """First CIN layer (xk IS x0, compress_interaction_network.py:125-132 with H_0 = N): the products x0[n]*x0[h] are
    symmetric in (n, h), so the weight of the pair lives on h <= n as W[n,h] + W[h,n] (fp32 sum) and is 0 above the
    diagonal.  Wc (C, N*N) -> (C, N*N) fp32; sum_{n,h} W x0[n] x0[h] is unchanged."""
    C = Wc.shape[0]
    W3 = Wc.float().view(C, N, N)
    return (torch.tril(W3) + torch.triu(W3, 1).transpose(1, 2)).reshape(C, N * N)


def cin_cl_backward_route(C: int, E: int, live: Optional[int], tri: int) -> Tuple[int, bool, bool]:
    """Which kernels the channels-last backward of a layer with C output channels runs: (Cg, mfma_data, mfma_dw).
    mfma_data / mfma_dw: trs_cin_cl_bwd_data / trs_cin_dw cover the shape (else the generic trs_cin_bwd).  Cg: the channels
    both gradients contract over -- ``live`` (the leading channels that can receive a gradient) where leaving the dead ones
    out applies: not under the symmetric fold, both matrix-core kernels cover the full AND the live width; else C."""
    mfma_data = C in (32, 64, 128, 256)
    mfma_dw = C in (64, 128, 256) and E in (32, 64, 128)
    skip = bool(live) and not tri and live in (64, 128, 256) and mfma_data and mfma_dw
    return (int(live) if skip else C), mfma_data, mfma_dw


def _cin_cf_operand(cf: Optional[torch.Tensor], T: torch.Tensor, n: int) -> torch.Tensor:
    """channels-first (B,n,E) form of the first n channels of the channels-last T (B,E,>=n): the caller's copy ``cf`` when
    it has the right shape and is contiguous, else a transposing copy."""
    B, E, _ = T.shape
    if cf is not None and tuple(cf.shape) == (B, n, E) and cf.is_contiguous():
        return cf
    return T[:, :, :n].transpose(1, 2).contiguous()


class _CINContractCL(Function):
    @staticmethod
    def forward(ctx, x0T, xkT, Wc, bias, N, H, x0_cf=None, xk_cf=None, live=None):
        require_device(x0T, xkT, Wc, bias)
        B, E, ld0 = x0T.shape
        ldk = xkT.stride(1)
        C = Wc.shape[0]
        if xkT.stride(2) != 1 or xkT.stride(0) != E * ldk or x0T.stride() != (E * ld0, ld0, 1):
            raise ValueError("cin_contract_cl: x0T must be contiguous and xkT a (B,E,>=H) view with unit inner stride")
        # First layer (xk IS x0): the products x0[n]*x0[h] are symmetric in (n,h), so W[n,h] + W[h,n] folded onto h <= n
        # (one fp32 add, one bf16 rounding) gives the same sums from half the weights; the kernels skip the k-steps /
        # h tiles that then hold only zeros.  Pays once a field needs more than one 32-wide k-step.
        tri = int(xkT.data_ptr() == x0T.data_ptr() and ldk == ld0 and H == N and N > 32)
        if tri:
            w = cin_fold_symmetric(Wc.detach(), N).to(torch.bfloat16)
        else:
            w = Wc.to(torch.bfloat16).contiguous()
        bb = None if bias is None else bias.to(torch.bfloat16).contiguous()
        yT = torch.empty(B, E, C, dtype=torch.bfloat16, device=x0T.device)
        ws_bytes = size_query("trs_cin_cl_workspace_bytes", N, H, C)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x0T.device)
        call("trs_cin_cl_fwd", ptr(x0T), ld0, ptr(xkT), ldk, ptr(w), ptr(bb), B, N, H, C, E, _abi.TRS_BF16, tri, ptr(yT),
             ptr(ws), ws_bytes, stream_ptr())
        ctx.tri = tri
        # live: the caller's promise that the gradient of the output channels [live, C) is exactly zero (the LAST layer's
        # "hidden" half, which the reference computes, splits off and never uses -- compress_interaction_network.py:151-156,
        # 176-181): the backward then leaves their (zero) terms out of both contractions
        ctx.live = int(live) if (live is not None and 0 < int(live) < C and not tri and CIN_SKIP_DEAD) else None
        ctx.save_for_backward(x0T, xkT, w)
        ctx.x0_cf = x0_cf        # the caller's channels-first (B,N,E) input, if it has one (saves a transpose per layer)
        ctx.xk_cf = xk_cf        # likewise the hidden state (B,H,E), emitted by the glue pass of the previous layer
        ctx.meta = (N, H, Wc.dtype, None if bias is None else bias.dtype)
        return yT

    @staticmethod
    @once_differentiable
    def backward(ctx, gyT):
        x0T, xkT, w = ctx.saved_tensors
        N, H, wdt, bdt = ctx.meta
        B, E, ld0 = x0T.shape
        C = w.shape[0]
        tri = ctx.tri
        need_x0, need_xk, need_w, need_b = ctx.needs_input_grad[:4]
        gy_cf = getattr(gyT, '_trs_cf', None)      # (B,C,E) copy emitted by the glue backward, if any
        gyT = gyT.contiguous()
        dev = x0T.device
        db = None
        pre = getattr(gyT, '_trs_colsum', None)    # column sums emitted by the glue backward that produced gyT
        if need_b and bdt is not None:
            if pre is not None and pre[1] == gyT._version:
                db = pre[0].double().sum(0).to(bdt)
            elif cin_glue_supported(gyT, 0, 0):
                db = _glue_colsum(gyT).to(bdt)
            else:
                db = gyT.float().sum(dim=(0, 1)).to(bdt)
        # Cg < C: the channels [Cg, C) carry no gradient, both contractions run over the first Cg channels of the full
        # tensors (strides C and C*E) and the rest of dW stays zero
        Cg, mfma_data, mfma_dw = cin_cl_backward_route(C, E, ctx.live, tri)
        if gy_cf is not None and not gy_cf.is_contiguous():
            Cg = C
        generic_data = (need_x0 or need_xk) and not mfma_data
        dx0T = dxkT = dW = None
        if (need_x0 or need_xk) and mfma_data:
            ldo = ((H + 31) // 32) * 32
            dx0T = torch.empty_like(x0T)
            # tri: xkT is x0T, the kernel returns the sum of the two gradients (= the gradient of the quadratic form
            # under the folded weights = under the original ones) in dx0T and xkT's slot of this function stays None
            dxk_pad = None if tri else torch.empty(B, E, ldo, dtype=torch.bfloat16, device=dev)
            ws_bytes = size_query("trs_cin_cl_bwd_data_workspace_bytes", N, H, Cg)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            call("trs_cin_cl_bwd_data", ptr(x0T), ld0, ptr(xkT), xkT.stride(1), ptr(gyT), C, ptr(w), B, N, H, Cg, E,
                 _abi.TRS_BF16, tri, ptr(dx0T), ptr(dxk_pad), ldo, ptr(ws), ws_bytes, stream_ptr())
            if tri or tuple(dxk_pad.shape) == tuple(xkT.shape):     # already zero past H (zero weight fragments)
                dxkT = dxk_pad
            else:
                dxkT = torch.zeros(xkT.shape, dtype=xkT.dtype, device=dev)
                dxkT[:, :, :H] = dxk_pad[:, :, :H]
        if need_w or generic_data:
            # channels-first operands (pixels contiguous): the caller's copies where it has them
            x0 = _cin_cf_operand(ctx.x0_cf, x0T, N)
            xk = x0 if (xkT.data_ptr() == x0T.data_ptr() and H == N) else _cin_cf_operand(ctx.xk_cf, xkT, H)
            gy = _cin_cf_operand(gy_cf, gyT, C)
        if need_w:
            dW = torch.zeros(C, N * H, dtype=torch.float32, device=dev)
        if generic_data or (need_w and not mfma_dw):
            # generic channels-first kernels for shapes the MFMA kernels do not cover
            gx0 = torch.empty_like(x0) if generic_data else None
            gxk = torch.empty_like(xk) if generic_data else None
            call("trs_cin_bwd", ptr(x0), ptr(xk), ptr(w), ptr(gy), B, N, H, C, E, _abi.TRS_BF16,
                 ptr(None if mfma_dw else dW), ptr(gx0), ptr(gxk), 0, stream_ptr())
            if generic_data:
                dx0T = torch.zeros_like(x0T)
                dx0T[:, :, :N] = gx0.transpose(1, 2)
                dxkT = torch.zeros(xkT.shape, dtype=xkT.dtype, device=dev)
                dxkT[:, :, :H] = gxk.transpose(1, 2)
        if need_w and mfma_dw:
            ws_bytes = size_query("trs_cin_dw_workspace_bytes", B, N, H, Cg)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            call("trs_cin_dw", ptr(gy), C * E, ptr(x0), ptr(xk), B, N, H, Cg, E, _abi.TRS_BF16, tri, ptr(dW), ptr(ws),
                 ws_bytes, stream_ptr())
        return (dx0T if need_x0 else None, dxkT if need_xk else None, None if dW is None else dW.to(wdt), db, None, None,
                None, None, None)


def cin_contract_cl(x0T: torch.Tensor, xkT: torch.Tensor, Wc: torch.Tensor, bias: Optional[torch.Tensor], N: int,
                    H: int, x0_cf: Optional[torch.Tensor] = None, xk_cf: Optional[torch.Tensor] = None,
                    live: Optional[int] = None) -> torch.Tensor:
    """channels-last CIN contraction on the matrix cores: x0T (B,E,ld0>=N, zero padded), xkT (B,E,>=H view).
    ``x0_cf`` / ``xk_cf``: channels-first copies (B,N,E) / (B,H,E) of the same values when the caller has them.
    ``live``: the caller's promise that only the first ``live`` output channels can receive a gradient (the rest feed
    nothing downstream): the backward leaves the others' exactly-zero terms out."""
    return _CINContractCL.apply(x0T, xkT, Wc, bias, N, H, None if x0_cf is None else x0_cf.detach(),
                                None if xk_cf is None else xk_cf.detach(), live)


# --------------------------------------------------------------------------------------------
# K3 fused: field-aware lookup + pair products straight from the N tables
# --------------------------------------------------------------------------------------------
class _FFMFused(Function):
    @staticmethod
    def forward(ctx, idx, offsets, *weights):
        require_device(idx, offsets, *weights)
        B, N = idx.shape
        if len(weights) != N:
            raise ValueError(f"need {N} tables, got {len(weights)}")
        V, E = weights[0].shape
        ws = [w.contiguous() for w in weights]
        out = torch.empty(B, N * (N - 1) // 2, E, dtype=ws[0].dtype, device=ws[0].device)
        flag = _ErrFlag(out.device)
        call("trs_ffm_fused_fwd", ptr(_pointer_table(ws)), V, E, value_dtype_code(ws[0]), ptr(idx), index_dtype_code(idx),
             ptr(offsets), B, N, ptr(out), ptr(flag.t), stream_ptr())
        flag.check("ffm_fused_fwd")
        if any(ctx.needs_input_grad[2:]):
            prefetch_row_buckets(idx, offsets, V)
        ctx.save_for_backward(idx, offsets, *weights)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        idx, offsets, *weights = ctx.saved_tensors
        B, N = idx.shape
        V, E = weights[0].shape
        ws = [w.contiguous() for w in weights]
        rb = row_buckets(idx, offsets, V)
        grads = [torch.empty_like(w) for w in ws]
        # the global row ids transposed to (N, B) int32: table i's walk reads ONE 4 B-per-sample column (cache-resident)
        # instead of a random 8-byte load per lookup (9.5 -> see profiles/r05_kernels.md)
        rid_t = None
        if V < 2 ** 31 and B > 0:
            # range check BEFORE narrowing: an id such as 2^32 + 5 must stay out of range (-1: contributes nothing, as in
            # the forward), not wrap onto a foreign row
            rid = idx.long() if offsets is None else idx.long() + offsets
            rid = torch.where((rid >= 0) & (rid < V), rid, rid.new_full((), -1))
            rid_t = rid.t().contiguous().to(torch.int32)
        call("trs_ffm_fused_bwd", ptr(_pointer_table(ws)), V, E, value_dtype_code(ws[0]), ptr(idx), index_dtype_code(idx),
             ptr(offsets), ptr(g.contiguous()), ptr(rb.row_start), ptr(rb.perm), B, N, ptr(_pointer_table(grads)),
             ptr(rid_t), stream_ptr())
        return (None, None, *grads)


def ffm_fused(weights: Sequence[torch.Tensor], idx: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """(B,N) indices + N field-aware tables -> (B, N(N-1)/2, E) pair products; (B,N*N,E) is never materialised."""
    idx = _as_index(idx)
    return _FFMFused.apply(idx, offsets, *weights)


# --------------------------------------------------------------------------------------------
# MLP backward epilogue: relu backward + bias gradient in one pass (GEMMs stay on hipBLASLt)
# --------------------------------------------------------------------------------------------
def rowdot_supported(h2: torch.Tensor) -> bool:
    """one-output Linear as a row-wise dot product: rows of 16-byte vectors, a power of two of them, at most 64"""
    if not (h2.is_cuda and h2.dim() == 2 and h2.dtype in (torch.float32, torch.bfloat16) and h2.is_contiguous()):
        return False
    ve = 16 // h2.element_size()
    lpr = h2.shape[1] // ve if h2.shape[1] % ve == 0 else 0
    return 1 <= lpr <= 64 and (lpr & (lpr - 1)) == 0


def rowdot_width_supported(C: int, elem_size: int) -> bool:
    lpr = C * elem_size // 16 if (C * elem_size) % 16 == 0 else 0
    return 1 <= lpr <= 64 and (lpr & (lpr - 1)) == 0


class _RowDot(Function):
    """out (rows, 1) = h (rows, C) @ w (1, C)^T + b (1): trs_rowdot_fwd / trs_rowdot_bwd.  ``w_use`` / ``b_use`` are
    the (possibly zero-padded) tensors the kernels read; gradients are returned for ``weight`` / ``bias``."""

    @staticmethod
    def forward(ctx, h, weight, bias, w_use, b_use):
        W = (weight if w_use is None else w_use).reshape(-1).contiguous()
        Bv = bias if w_use is None else b_use
        h2 = h.reshape(-1, h.shape[-1])
        out = torch.empty(h2.shape[0], 1, dtype=h.dtype, device=h.device)
        call("trs_rowdot_fwd", ptr(h2), ptr(W), ptr(Bv), h2.shape[0], h2.shape[1], value_dtype_code(h2), ptr(out),
             stream_ptr())
        ctx.save_for_backward(h2, W)
        ctx.meta = (tuple(h.shape), tuple(weight.shape), weight.dtype, bias is not None)
        return out.reshape(*h.shape[:-1], 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        h2, W = ctx.saved_tensors
        hshape, wshape, wdt, has_bias = ctx.meta
        rows, C = h2.shape
        g2 = g.reshape(-1).contiguous()
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2])
        gh = torch.empty_like(h2) if need_h else None
        gw = torch.empty(C + 1, dtype=torch.float32, device=h2.device) if need_w else None
        ws_bytes = size_query("trs_rowdot_bwd_workspace_bytes", rows, C)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=h2.device) if need_w else None
        call("trs_rowdot_bwd", ptr(g2), ptr(h2), ptr(W), rows, C, value_dtype_code(h2), ptr(gh),
             ptr(gw), ptr(gw[C:]) if need_w else ptr(None), ptr(ws), ws_bytes if need_w else 0, stream_ptr())
        gq = gw.to(wdt) if need_w else None                      # one cast for weight row and bias
        g_weight = gq[:wshape[1]].reshape(wshape) if (need_w and ctx.needs_input_grad[1]) else None
        g_bias = gq[C:] if (need_w and has_bias and ctx.needs_input_grad[2]) else None
        return (gh.reshape(hshape) if need_h else None), g_weight, g_bias, None, None


def transpose_pad_supported(x: torch.Tensor, ld: int) -> bool:
    """(B, N, E) bf16 HIP tensor -> (B, E, ld) with zeros behind the N fields in one pass (trs_transpose_pad)"""
    return (x.is_cuda and x.dim() == 3 and x.dtype == torch.bfloat16 and x.shape[1] <= ld <= 64 and ld % 8 == 0
            and x.shape[2] <= 64 and x.shape[2] % 8 == 0)


class _TransposePad(Function):
    """x (B,N,E) -> (B,E,ld): out[b,e,n] = x[b,n,e], zeros for n >= N; the gradient is the transposition back.  What
    ``x.new_zeros(B,E,ld)[:, :, :N] = x.transpose(1,2)`` does in a fill + a strided copy forward and a clone + a slice
    clone backward (compress_interaction_network.py:105 keeps the activations as ('B','E','N'))."""

    @staticmethod
    def forward(ctx, x, ld):
        x = x.contiguous()
        B, N, E = x.shape
        out = torch.empty(B, E, ld, dtype=x.dtype, device=x.device)
        call("trs_transpose_pad", ptr(x), B, N, E, E, ptr(out), ld, value_dtype_code(x), stream_ptr())
        ctx.dims = (N, E, ld)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        N, E, ld = ctx.dims
        g = g.contiguous()
        gx = torch.empty(g.shape[0], N, E, dtype=g.dtype, device=g.device)
        call("trs_transpose_pad", ptr(g), g.shape[0], E, N, ld, ptr(gx), E, value_dtype_code(g), stream_ptr())
        return gx, None


def transpose_pad(x: torch.Tensor, ld: int) -> torch.Tensor:
    return _TransposePad.apply(x, ld)


def cat_head_supported(a: torch.Tensor, d: torch.Tensor, weight: torch.Tensor) -> bool:
    """one-output Linear over cat((a, d), dim=2).flatten(1) as one pass over the two blocks (trs_cat_head_fwd / _bwd):
    (B, N, Ea) and (B, N, Eb) HIP tensors of one dtype (bf16 / fp32) with rows of whole 16-byte vectors, at most 1024
    vectors per sample, weight (1, N * (Ea + Eb))"""
    if not (a.is_cuda and d.is_cuda and a.dim() == 3 and d.dim() == 3 and a.shape[:2] == d.shape[:2]
            and a.dtype == d.dtype == weight.dtype and a.dtype in (torch.float32, torch.bfloat16)):
        return False
    N, Ea, Eb = a.shape[1], a.shape[2], d.shape[2]
    ve = 16 // a.element_size()
    return (Ea % ve == 0 and Eb % ve == 0 and N * (Ea + Eb) // ve <= 1024
            and tuple(weight.shape) == (1, N * (Ea + Eb)))


class _CatHead(Function):
    """out (B, 1) = cat((a, d), dim=2).flatten(1) @ weight (1, N*(Ea+Eb))^T + bias: the head of the reference's
    DeepAndCrossNetworkModel (deep_and_cross_network.py:82-92) without the (B, N, Ea+Eb) concatenation, its slice
    copies in the backward and the 4992-wide GEMV / GEMMs around them."""

    @staticmethod
    def forward(ctx, a, d, weight, bias):
        a, d = a.contiguous(), d.contiguous()
        W = weight.reshape(-1).contiguous()
        B, N, Ea = a.shape
        Eb = d.shape[2]
        out = torch.empty(B, 1, dtype=a.dtype, device=a.device)
        call("trs_cat_head_fwd", ptr(a), ptr(d), ptr(W), ptr(bias), B, N, Ea, Eb, value_dtype_code(a), ptr(out),
             stream_ptr())
        ctx.save_for_backward(a, d, W)
        ctx.meta = (tuple(weight.shape), bias is not None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, d, W = ctx.saved_tensors
        wshape, has_bias = ctx.meta
        B, N, Ea = a.shape
        Eb = d.shape[2]
        C = N * (Ea + Eb)
        g2 = g.reshape(-1).contiguous()
        need_a, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_w = ctx.needs_input_grad[2] or (has_bias and ctx.needs_input_grad[3])
        ga = torch.empty_like(a) if need_a else None
        gd = torch.empty_like(d) if need_d else None
        gw = torch.empty(C + 1, dtype=torch.float32, device=a.device) if need_w else None
        ws_bytes = size_query("trs_cat_head_bwd_workspace_bytes", B, N, Ea, Eb) if need_w else 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device) if need_w else None
        call("trs_cat_head_bwd", ptr(g2), ptr(a), ptr(d), ptr(W), B, N, Ea, Eb, value_dtype_code(a), ptr(ga), ptr(gd),
             ptr(gw), ptr(gw[C:]) if need_w else ptr(None), ptr(ws), ws_bytes, stream_ptr())
        gq = gw.to(W.dtype) if need_w else None                  # one cast for the weight row and the bias
        g_weight = gq[:C].reshape(wshape) if (need_w and ctx.needs_input_grad[2]) else None
        g_bias = gq[C:] if (need_w and has_bias and ctx.needs_input_grad[3]) else None
        return ga, gd, g_weight, g_bias


def cat_head(a: torch.Tensor, d: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """``F.linear(torch.cat((a, d), dim=2).flatten(1), weight, bias)`` for a one-output Linear; see cat_head_supported"""
    return _CatHead.apply(a, d, weight, bias)


def relu_bwd_bias_supported(y: torch.Tensor) -> bool:
    row_bytes = y.shape[-1] * y.element_size()
    return (y.is_cuda and y.dtype in (torch.float32, torch.bfloat16) and y.is_contiguous()
            and row_bytes % 16 == 0 and row_bytes <= 4096)


def relu_bwd_bias(gy: torch.Tensor, y: torch.Tensor):
    """gz = gy * (y > 0), gb = gz.sum(0) (fp32) for y = relu(...) of shape (rows, C)."""
    rows, C = y.shape
    gy = gy.contiguous()
    gz = torch.empty_like(gy)
    gb = torch.empty(C, dtype=torch.float32, device=y.device)
    ws_bytes = size_query("trs_relu_bwd_bias_workspace_bytes", rows, C)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
    call("trs_relu_bwd_bias", ptr(gy), ptr(y), rows, C, value_dtype_code(y), ptr(gz), ptr(gb), ptr(ws), ws_bytes,
         stream_ptr())
    return gz, gb


# --------------------------------------------------------------------------------------------
# N4: per-field MLP (Linear -> ReLU ... -> Linear on every row of a (B,N,E) block) as one kernel per direction
# --------------------------------------------------------------------------------------------
FUSED_MLP = os.environ.get("TRS_FUSED_MLP", "1") not in ("", "0")
FUSED_MLP_MIN_ROWS = 4096


def _pad32(v: int) -> int:
    return (v + 31) // 32 * 32


def _i32_array(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[0 if t is None else t.data_ptr() for t in tensors])


_mlp_fused_verdicts = {}


def mlp_fused_supported_for(rows: int, dtype: torch.dtype, is_cuda: bool, widths: Sequence[int]) -> bool:
    """bf16 rows on the HIP device, every width a multiple of 8 and at most 512, enough rows to fill the chip.  Takes the
    row count / dtype / placement instead of a tensor (no throwaway allocation) and remembers the library's verdict per
    width list."""
    if not (FUSED_MLP and is_cuda and dtype == torch.bfloat16 and rows >= FUSED_MLP_MIN_ROWS):
        return False
    if len(widths) < 2 or len(widths) > 9 or any(w % 8 or w > 512 for w in widths):
        return False
    key = tuple(int(w) for w in widths)
    ok = _mlp_fused_verdicts.get(key)
    if ok is None:
        ok = _mlp_fused_verdicts[key] = bool(_abi.load().trs_mlp_fused_supported(len(widths) - 1, _i32_array(widths)))
    return ok


def mlp_fused_supported(x: torch.Tensor, widths: Sequence[int]) -> bool:
    return mlp_fused_supported_for(x.numel() // max(1, x.shape[-1]), x.dtype, x.is_cuda, widths)


MLP_FAMILY_AUTO, MLP_FAMILY_TILE, MLP_FAMILY_ROW_OWNER, MLP_FAMILY_MIXED = 0, 1, 2, 3
_mlp_family_request = MLP_FAMILY_AUTO


class mlp_family:
    """``with mlp_family(MLP_FAMILY_TILE | MLP_FAMILY_ROW_OWNER | MLP_FAMILY_AUTO):`` -- the kernel family the fused-MLP
    FORWARDS issued inside the block ask for (a request the library resolves per call, trs_mlp_fused_family; a family
    that does not cover a stack falls back to AUTO for it).  Backwards never look at this: every autograd node records the
    family its forward ran and hands that to trs_mlp_fused_bwd_data."""

    def __init__(self, request: int):
        self.request = int(request)

    def __enter__(self):
        global _mlp_family_request
        self.prev, _mlp_family_request = _mlp_family_request, self.request
        return self

    def __exit__(self, *exc):
        global _mlp_family_request
        _mlp_family_request = self.prev
        return False


def mlp_fused_family(widths: Sequence[int], rows: int, request: Optional[int] = None) -> int:
    """The kernel family (MLP_FAMILY_TILE / MLP_FAMILY_ROW_OWNER) a forward of this stack runs"""
    req = _mlp_family_request if request is None else int(request)
    wl = _i32_array(widths)
    fam = int(_abi.load().trs_mlp_fused_family(len(widths) - 1, wl, int(rows), req))
    if fam == 0 and req != MLP_FAMILY_AUTO:
        fam = int(_abi.load().trs_mlp_fused_family(len(widths) - 1, wl, int(rows), MLP_FAMILY_AUTO))
    if fam == 0:
        raise RuntimeError(f"torecsys_amd: no fused-MLP kernel family for widths {list(widths)}")
    return fam


def fused_mlp_forward_raw(x2: torch.Tensor, Ws: Sequence[torch.Tensor], bs: Sequence[torch.Tensor],
                          input_mask: bool = False, family: Optional[int] = None, x_stride: int = 0):
    """trs_mlp_fused_fwd on rows x2 (rows, widths[0]): returns (y (rows, widths[L]), hidden [(rows, pad32(w))] -- the
    ReLU outputs of the hidden layers, zero in the padding columns --, masks [the sign bits of the hidden layers in the
    kernel's own order: opaque bytes for trs_mlp_fused_bwd_data], [with ``input_mask`` (x2 is itself a ReLU output): the
    sign bits of x2 in the same form,] family -- the kernel family that ran, which the backward of THESE masks must be
    given (the two families lay the sign bits out differently)."""
    L = len(Ws)
    widths = [Ws[0].shape[1]] + [w.shape[0] for w in Ws]
    rows, dev = x2.shape[0], x2.device
    # ``x_stride`` (row-owner / mixed family): x2's rows are wider than the stack's input -- the first widths[0] columns
    # of every row are read
    if x_stride and (x_stride < widths[0] or x2.shape[1] != x_stride or not x2.is_contiguous()):
        raise ValueError(f"fused_mlp_forward_raw: x_stride {x_stride} does not describe x2 {tuple(x2.shape)}")
    fam = mlp_fused_family(widths, rows, family)
    hidden = [torch.empty(rows, _pad32(widths[l + 1]), dtype=torch.bfloat16, device=dev) for l in range(L - 1)]
    mask_bytes = size_query("trs_mlp_fused_mask_bytes", rows)
    masks = [torch.empty(mask_bytes, dtype=torch.uint8, device=dev) for _ in range(L - 1)]
    mask_in = torch.empty(mask_bytes, dtype=torch.uint8, device=dev) if input_mask else None
    y = torch.empty(rows, widths[L], dtype=torch.bfloat16, device=dev)
    wl = _i32_array(widths)
    ws_bytes = size_query("trs_mlp_fused_workspace_bytes", L, wl)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    call("trs_mlp_fused_fwd", ptr(x2), rows, L, wl, _ptr_array(Ws), _ptr_array(bs), _ptr_array(hidden),
         _ptr_array(masks), ptr(mask_in), ptr(y), _abi.TRS_BF16, fam, int(x_stride), ptr(ws), ws_bytes, stream_ptr())
    if input_mask:
        return y, hidden, masks, mask_in, fam
    return y, hidden, masks, fam


def mlp_bwd_wlast_bytes(widths: Sequence[int], rows: int, family: int, live: int) -> int:
    """Bytes of the partial buffer when the fused backward of this stack carries the output layer's weight gradient
    (trs_mlp_fused_bwd_wlast_part_bytes); 0: it does not -- the caller keeps the product of its own."""
    return size_query("trs_mlp_fused_bwd_wlast_part_bytes", len(widths) - 1, _i32_array(widths), int(rows), _abi.TRS_BF16,
                      int(family), int(live))


def fused_mlp_backward_raw(gy2: torch.Tensor, widths: Sequence[int], Ws: Sequence[torch.Tensor],
                           masks: Sequence[torch.Tensor], mask_in: Optional[torch.Tensor] = None, *, family: int,
                           h_last: Optional[torch.Tensor] = None, live: int = 0, parts: bool = False):
    """trs_mlp_fused_bwd_data: (gx, gz [d(pre-activation) of the hidden layers], gb [fp32 bias gradients, padded]) and,
    with ``mask_in``, gb_in: gx is then masked by the upstream ReLU and gb_in holds its column sums.  ``family``: what
    fused_mlp_forward_raw returned with these masks.
    With ``h_last`` (the last hidden activation) and ``live`` (the output layer's real columns) the kernel also sums the
    output layer's weight gradient (trs_mlp_fused_bwd_data_wlast; the caller asked mlp_bwd_wlast_bytes first): a fifth
    result, (live, pad32(widths[L-1])) fp32.  gy2 is then (rows, widths[L]) or the contiguous (rows, live) gradient.
    With ``parts`` (trs_mlp_fused_bwd_data_parts: tile and mixed family, rows > 0) the reduce launch behind the kernel is
    left out and every fp32 result is the set of per-workgroup partial rows instead, a strided view of the call's
    workspace that keeps it alive: gb[l] and gb_in (nparts, padded width), gw_last (nparts, live, padded width).
    _tail_grads folds such sets in its batched finish; colsum_parts_reduce sums them on its own."""
    if family not in (MLP_FAMILY_TILE, MLP_FAMILY_ROW_OWNER, MLP_FAMILY_MIXED):
        raise ValueError("fused_mlp_backward_raw: family must be the value the forward returned with these masks")
    L = len(Ws)
    rows, dev = gy2.shape[0], gy2.device
    gz = [torch.empty(rows, _pad32(widths[l + 1]), dtype=torch.bfloat16, device=dev) for l in range(L - 1)]
    gx = torch.empty(rows, widths[0], dtype=torch.bfloat16, device=dev)   # the kernel always writes dL/dx (its last GEMM)
    wl = _i32_array(widths)
    ws_bytes = size_query("trs_mlp_fused_workspace_bytes", L, wl)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    if parts:
        return _fused_mlp_backward_parts(gy2, widths, Ws, masks, mask_in, family, h_last, live, gz, gx, wl, ws)
    gb = [torch.empty(_pad32(widths[l + 1]), dtype=torch.float32, device=dev) for l in range(L)]
    gb_in = torch.empty(_pad32(widths[0]), dtype=torch.float32, device=dev) if mask_in is not None else None
    if h_last is not None:
        if not (gy2.is_contiguous() and h_last.is_contiguous() and h_last.shape[0] == rows):
            raise ValueError("fused_mlp_backward_raw: gy2 / h_last must be contiguous over the same rows")
        part_bytes = mlp_bwd_wlast_bytes(widths, max(rows, 1), family, live)
        part = torch.empty(max(part_bytes, 16), dtype=torch.uint8, device=dev)
        gw_last = torch.empty(live, _pad32(widths[L - 1]), dtype=torch.float32, device=dev)
        call("trs_mlp_fused_bwd_data_wlast", ptr(gy2), gy2.shape[1], rows, L, wl, _ptr_array(Ws), _ptr_array(masks),
             _ptr_array(gz), _ptr_array(gb), ptr(gx), ptr(mask_in), ptr(gb_in), ptr(h_last), h_last.shape[1], int(live),
             ptr(part), part_bytes, ptr(gw_last), _abi.TRS_BF16, int(family), ptr(ws), ws_bytes, stream_ptr())
        return gx, gz, gb, gb_in, gw_last
    call("trs_mlp_fused_bwd_data", ptr(gy2), rows, L, wl, _ptr_array(Ws), _ptr_array(masks), _ptr_array(gz),
         _ptr_array(gb), ptr(gx), ptr(mask_in), ptr(gb_in), _abi.TRS_BF16, int(family), ptr(ws), ws_bytes, stream_ptr())
    return gx, gz, gb, gb_in


def _fused_mlp_backward_parts(gy2, widths, Ws, masks, mask_in, family, h_last, live, gz, gx, wl, ws):
    """the ``parts`` form of fused_mlp_backward_raw: the entry reports addresses, the results are views of the buffers"""
    L, rows, dev = len(Ws), gy2.shape[0], gy2.device
    part, part_bytes = None, 0
    if h_last is not None:
        if not (gy2.is_contiguous() and h_last.is_contiguous() and h_last.shape[0] == rows):
            raise ValueError("fused_mlp_backward_raw: gy2 / h_last must be contiguous over the same rows")
        part_bytes = mlp_bwd_wlast_bytes(widths, max(rows, 1), family, live)
        part = torch.empty(max(part_bytes, 16), dtype=torch.uint8, device=dev)
    n = L + 4
    where, stride, nparts = (ctypes.c_void_p * n)(), (ctypes.c_int32 * n)(), ctypes.c_int32(0)
    call("trs_mlp_fused_bwd_data_parts", ptr(gy2), gy2.shape[1], rows, L, wl, _ptr_array(Ws), _ptr_array(masks),
         _ptr_array(gz), ptr(gx), ptr(mask_in), ptr(h_last), h_last.shape[1] if h_last is not None else 0, int(live),
         ptr(part), part_bytes, where, stride, ctypes.byref(nparts),
         _abi.TRS_BF16, int(family), ptr(ws), ws.numel(), stream_ptr())
    P = int(nparts.value)

    def view(base, k, shape, strides):
        f32 = base.view(torch.float32)
        off = (int(where[k] or 0) - base.data_ptr()) // 4
        last = off + sum((s - 1) * st for s, st in zip(shape, strides))
        if not (where[k] and 0 <= off and last < f32.numel()):
            raise RuntimeError("fused_mlp_backward_raw: a partial set lies outside its buffer")
        return torch.as_strided(f32, shape, strides, off)

    gb = [view(ws, l, (P, _pad32(widths[l + 1])), (int(stride[l]), 1)) for l in range(L)]
    gb_in = view(ws, L, (P, _pad32(widths[0])), (int(stride[L]), 1)) if mask_in is not None else None
    out = [gx, gz, gb, gb_in]
    if h_last is not None:
        Kh = _pad32(widths[L - 1])
        out.append(view(part, L + 1, (P, live, Kh), (int(stride[L + 1]), Kh, 1)))
    return tuple(out)


def colsum_parts_reduce(sets: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """The sums of 1 .. 8 partial sets (fp32 (nparts, n), rows a stride apart: fused_mlp_backward_raw with ``parts``) in
    one launch of the tile backward's own reduce kernel: the vectors trs_mlp_fused_bwd_data would have written."""
    outs = [torch.empty(t.shape[1], dtype=torch.float32, device=t.device) for t in sets]
    if len({t.shape[0] for t in sets}) != 1 or any(t.dim() != 2 or t.stride(1) != 1 for t in sets):
        raise ValueError("colsum_parts_reduce: sets of one launch share their partial count")
    call("trs_colsum_parts_reduce", len(sets), _ptr_array(sets), _i32_array([t.stride(0) for t in sets]),
         _i32_array([t.shape[1] for t in sets]), int(sets[0].shape[0]), _ptr_array(outs), stream_ptr())
    return outs


def _plain_sum(t):
    """a bias gradient as a summed vector: itself, or the sum of its partial rows"""
    return colsum_parts_reduce([t])[0] if t is not None and t.dim() == 2 else t


def wgrad_bias_rides(out_f: int, in_f: int) -> bool:
    """the bias cast of an (out_f, in_f) layer fits the one row of workgroups trs_wgrad_finish has for it"""
    return out_f <= (in_f + 255) // 256 * 256


def wgrad_finish(jobs, S: int, dtype_code: int, transposed: bool = False):
    """The finish of 1 .. 8 split-K weight gradients in one launch: trs_wgrad_finish, or trs_wgrad_finish_t for partial
    products stored transposed.  ``jobs`` = [(part, gw, gb_f32, gb, R, Cc, out_rows, out_cols)]: gw (out_rows, out_cols)
    out of part (S, R, Cc) -- (S, Cc, R) transposed --, gb = the cast of gb_f32 (both or neither).  A 2-D gb_f32 is a set
    of partial rows (fused_mlp_backward_raw with ``parts``), which the launch folds itself.  ``part`` None: a job without a
    product, gb[:out_cols] = the cast of gb_f32, nothing else of the job is read."""
    # The entry's ten arrays as two allocations, n entries per array: part, gw, gb_f32, gb | the partial's two dimensions in
    # the entry's order, out_rows, out_cols, gb_nparts, gb_stride.  (An array object per argument cost 6 us of host time
    # for one job, against 1 us for the scalar arguments the one-job entries used to take; this is 1.6.)
    n = len(jobs)
    ptrs, ints = (ctypes.c_void_p * (4 * n))(), (ctypes.c_int32 * (6 * n))()
    sets = False
    for k, (part, gw, gb_f32, gb, R, Cc, out_rows, out_cols) in enumerate(jobs):
        for f, t in enumerate((part, gw, gb_f32, gb)):
            if t is not None:
                ptrs[f * n + k] = t.data_ptr()
        if gb_f32 is not None and gb_f32.dim() == 2:
            sets, ints[4 * n + k], ints[5 * n + k] = True, gb_f32.shape[0], gb_f32.stride(0)
        ints[k], ints[n + k] = (Cc, R) if transposed else (R, Cc)
        ints[2 * n + k], ints[3 * n + k] = out_rows, out_cols
    p, i = ctypes.addressof(ptrs), ctypes.addressof(ints)
    call("trs_wgrad_finish_t" if transposed else "trs_wgrad_finish", n, p, S, i, i + 4 * n, i + 8 * n, i + 12 * n,
         dtype_code, p + 8 * n, p + 16 * n, p + 24 * n, i + 16 * n if sets else None, i + 20 * n if sets else None,
         stream_ptr())


class _FusedMLP(Function):
    """y = Linear_{L-1}(relu(... relu(Linear_0(x)))) on the rows of x (..., widths[0]); params = W0, b0, W1, b1, ...
    (nn.Linear layout).  Forward and the data gradient are one HIP kernel each (trs_mlp_fused_*); the weight gradients
    are GEMMs with K = rows on the tensors those kernels leave behind (hidden activations, pre-activation gradients)."""

    @staticmethod
    def forward(ctx, x, *params):
        require_device(x, *params)
        L = len(params) // 2
        Ws = [params[2 * l].contiguous() for l in range(L)]
        bs = [params[2 * l + 1].contiguous() for l in range(L)]
        widths = [Ws[0].shape[1]] + [w.shape[0] for w in Ws]
        x2 = x.reshape(-1, widths[0]).contiguous()
        y, hidden, masks, fam = fused_mlp_forward_raw(x2, Ws, bs)
        ctx.save_for_backward(x2, *Ws, *hidden, *masks)
        ctx.meta = (L, widths, tuple(x.shape), [p.dtype for p in params], fam)
        return y.reshape(*x.shape[:-1], widths[L])

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        L, widths, xshape, pdt, fam = ctx.meta
        saved = ctx.saved_tensors
        x2, Ws = saved[0], saved[1:1 + L]
        hidden, masks = saved[1 + L:L + L], saved[L + L:]
        rows, dev = x2.shape[0], x2.device
        gy2 = gy.reshape(rows, widths[L]).contiguous()
        same_dt = all(pdt[2 * l] == pdt[2 * l + 1] for l in range(L))
        gw_last = None
        if (same_dt and ctx.needs_input_grad[2 * L - 1] and gy2.dtype == torch.bfloat16
                and mlp_bwd_wlast_bytes(widths, rows, fam, widths[L]) > 0):
            gx, gz, gb, _, gw_last = fused_mlp_backward_raw(gy2, widths, Ws, masks, family=fam, h_last=hidden[L - 2],
                                                            live=widths[L])
        else:
            gx, gz, gb, _ = fused_mlp_backward_raw(gy2, widths, Ws, masks, family=fam)
        grads = []
        if same_dt:
            for gw, gbias in _tail_grads([(gy2 if l == L - 1 else gz[l], x2 if l == 0 else hidden[l - 1], widths[l + 1],
                                           widths[l], pdt[2 * l], gb[l], ctx.needs_input_grad[1 + 2 * l],
                                           ctx.needs_input_grad[2 + 2 * l]) for l in range(L)], gw_last):
                grads += [gw, gbias]
            return (gx.reshape(xshape) if ctx.needs_input_grad[0] else None, *grads)
        for l in range(L):
            inp = x2 if l == 0 else hidden[l - 1]               # (rows, widths[l] | pad32)
            g = gy2 if l == L - 1 else gz[l]                    # (rows, widths[l+1] | pad32)
            need_w, need_b = ctx.needs_input_grad[1 + 2 * l], ctx.needs_input_grad[2 + 2 * l]
            if pdt[2 * l] == pdt[2 * l + 1]:
                gw, gbias = _tail_layer_grads(g, inp, widths[l + 1], widths[l], pdt[2 * l], gb[l], need_w, need_b)
            else:                                               # (_tail_layer_grads casts both to the weight's dtype)
                gw = _wgrad_rows(g, inp, widths[l + 1], widths[l], pdt[2 * l]) if need_w else None
                gbias = gb[l][:widths[l + 1]].to(pdt[2 * l + 1]) if need_b else None
            grads += [gw, gbias]
        return (gx.reshape(xshape) if ctx.needs_input_grad[0] else None, *grads)


ROWS_GEMM = os.environ.get("TRS_ROWS_GEMM", "1") not in ("", "0")
ROWS_GEMM_MIN_COLS = 1024       # narrower outputs: the library GEMM is as fast


def rows_gemm_supported_for(rows: int, x_stride: int, W: torch.Tensor, out_f: int, in_f: int) -> bool:
    """rows_gemm_supported for a contiguous bf16 (rows, x_stride) gradient that does not exist yet"""
    if not (ROWS_GEMM and W.is_cuda and W.dtype == torch.bfloat16 and W.is_contiguous() and rows >= 4096
            and in_f >= ROWS_GEMM_MIN_COLS and W.shape[1] == in_f and W.shape[0] >= out_f):
        return False
    return bool(_abi.load().trs_rows_gemm_supported(int(out_f), int(in_f), int(x_stride)))


def rows_gemm_supported(g: torch.Tensor, W: torch.Tensor, out_f: int, in_f: int) -> bool:
    """dL/dx = g[:, :out_f] @ W[:out_f] by trs_rows_gemm: bf16 on the device, a short contraction (out_f <= 512) and a
    wide result (the 2496 embedding columns in front of a deep branch), enough rows to fill the chip"""
    if not (g.is_cuda and g.dtype == torch.bfloat16 and g.dim() == 2 and g.is_contiguous()):
        return False
    return rows_gemm_supported_for(g.shape[0], g.shape[1], W, out_f, in_f)


def rows_gemm(g: torch.Tensor, W: torch.Tensor, out_f: int, in_f: int) -> torch.Tensor:
    y = torch.empty(g.shape[0], in_f, dtype=torch.bfloat16, device=g.device)
    ws_bytes = size_query("trs_rows_gemm_workspace_bytes", out_f, in_f)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g.device)
    call("trs_rows_gemm", ptr(g), g.shape[0], g.shape[1], ptr(W), out_f, in_f, _abi.TRS_BF16, ptr(y), ptr(ws), ws_bytes,
         stream_ptr())
    return y


def _tail_layer_grads(g, inp, out_f, in_f, dtype, gb_f32, need_w, need_b):
    """(dW, db) of one layer behind the fused kernels: the bias cast rides in the weight gradient's finish launch"""
    if need_w and need_b:
        return _wgrad_rows(g, inp, out_f, in_f, dtype, gb_f32)
    gw = _wgrad_rows(g, inp, out_f, in_f, dtype) if need_w else None
    return gw, (gb_f32[:out_f].to(dtype) if need_b else None)


def _wgrad_many_splits(jobs) -> int:
    """Row ranges per job when the products ``jobs`` = [(g, inp, M, N)] over the same rows go out as ONE launch of the
    LDS-DMA kernel (trs_wgrad_rows_many_splits; 0: the caller keeps the per-layer calls)."""
    if not WGRAD_ROWS or len(jobs) < 2:
        return 0
    for g, inp, _, _ in jobs:
        if not (g.is_cuda and g.dtype == torch.bfloat16 and inp.dtype == torch.bfloat16 and g.is_contiguous()
                and inp.is_contiguous() and g.shape[0] == jobs[0][0].shape[0]):
            return 0
    return size_query("trs_wgrad_rows_many_splits", len(jobs), _i32_array([j[2] for j in jobs]),
                      _i32_array([j[3] for j in jobs]), _i32_array([j[0].shape[1] for j in jobs]),
                      _i32_array([j[1].shape[1] for j in jobs]), int(jobs[0][0].shape[0]))


# The deep branch's weight gradients as ONE product launch (trs_wgrad_wide_many) and one finish: measured against the
# two products and two finishes it replaces (profiles/wgrad_deep.md), product + finish in us: 8192 rows 66 against 100,
# 16 384 rows 92 against 120, 65 536 rows 200 against 237.  It is the faster pair at 8192 rows too, but the launches of
# the 2496-400-400-400-1 stack at exactly that row count are what tests/test_gpu_wgrad_many.py and
# tests/test_gpu_mlp_bwd_wlast.py pin (trs_wgrad_rows_many once per backward, the first layer bit-equal to
# trs_wgrad_wide's), so the stack takes the merged launch from the next measured row count on.
DEEP_WGRAD_MIN_ROWS = 16384


def _wgrad_deep_jobs(first, tail):
    """[(x, g, M_x, N_g, out_f, in_f, gb_f32 or None)] for trs_wgrad_wide_many from layer tuples (g, inp, out_f, in_f,
    dtype, gb_f32, need_w, need_b), the first layer in front: dW^T = inp^T g over whole 208-column blocks of inp and the
    16-column tiles of g that hold out_f; None where an operand is not a bf16 matrix of that width"""
    jobs = []
    for g, inp, out_f, in_f, dtype, gb_f32, _, need_b in [first] + tail:
        M_x, N_g = (in_f + 207) // 208 * 208, (out_f + 15) // 16 * 16
        if not (g.is_cuda and g.dtype == inp.dtype == dtype == torch.bfloat16 and g.dim() == inp.dim() == 2
                and g.is_contiguous() and inp.is_contiguous() and g.shape[0] == inp.shape[0] == first[0].shape[0]
                and M_x <= inp.shape[1] and N_g <= g.shape[1] and (not need_b or gb_f32 is not None)):
            return None
        jobs.append((inp, g, M_x, N_g, out_f, in_f, gb_f32 if need_b else None))
    return jobs


def _wgrad_deep_splits(jobs) -> int:
    """Row ranges when ``jobs`` (see _wgrad_deep_jobs) go out as one launch of the four-wave LDS-DMA kernel
    (trs_wgrad_wide_many_splits; 0: the caller keeps the launch per product)."""
    if not WGRAD_ROWS or jobs is None or not 2 <= len(jobs) <= 4 or jobs[0][0].shape[0] < DEEP_WGRAD_MIN_ROWS:
        return 0
    return size_query("trs_wgrad_wide_many_splits", len(jobs), _i32_array([j[2] for j in jobs]),
                      _i32_array([j[0].shape[1] for j in jobs]), _i32_array([j[3] for j in jobs]),
                      _i32_array([j[1].shape[1] for j in jobs]), int(jobs[0][0].shape[0]))


def wgrad_deep_splits_for(rows: int, dims) -> int:
    """_wgrad_deep_splits from shapes alone, for a backward that chooses its form before the gradients exist: ``dims`` =
    [(in_f, ldx, out_f, ldg)] of contiguous bf16 operands over ``rows`` rows, the wide first layer in front"""
    if not WGRAD_ROWS or not 2 <= len(dims) <= 4 or rows < DEEP_WGRAD_MIN_ROWS:
        return 0
    M_x, N_g = [(d[0] + 207) // 208 * 208 for d in dims], [(d[2] + 15) // 16 * 16 for d in dims]
    if any(m > d[1] or n > d[3] for m, n, d in zip(M_x, N_g, dims)):
        return 0
    return size_query("trs_wgrad_wide_many_splits", len(dims), _i32_array(M_x), _i32_array([d[1] for d in dims]),
                      _i32_array(N_g), _i32_array([d[3] for d in dims]), int(rows))


def _wgrad_deep(jobs, S, casts):
    """the merged product and its finish; ``casts``: jobs without a product (see wgrad_finish) that ride in it.  Returns [(dW, db or None)] per job."""
    dev, rows = jobs[0][0].device, int(jobs[0][0].shape[0])
    parts = [torch.empty(S, j[2], j[3], dtype=torch.float32, device=dev) for j in jobs]
    call("trs_wgrad_wide_many", len(jobs), _ptr_array([j[0] for j in jobs]), _i32_array([j[0].shape[1] for j in jobs]),
         _ptr_array([j[1] for j in jobs]), _i32_array([j[1].shape[1] for j in jobs]), rows,
         _i32_array([j[2] for j in jobs]), _i32_array([j[3] for j in jobs]), S, _ptr_array(parts), stream_ptr())
    gws = [torch.empty(j[4], j[5], dtype=torch.bfloat16, device=dev) for j in jobs]
    gbs = [torch.empty(j[4], dtype=torch.bfloat16, device=dev) if j[6] is not None else None for j in jobs]
    wgrad_finish([(p, gw, j[6], gb, j[3], j[2], j[4], j[5]) for p, gw, gb, j in zip(parts, gws, gbs, jobs)] + casts, S,
                 _abi.TRS_BF16, transposed=True)
    return list(zip(gws, gbs))


def _tail_grads(layers, gw_last=None, first=None):
    """(dW, db) of every layer behind the fused kernels, ``layers`` = [(g, inp, out_f, in_f, dtype, gb_f32, need_w,
    need_b)] in stack order with the output layer last.  The hidden layers whose weight gradient is needed go out as one
    batched product and one batched finish where trs_wgrad_rows_many_splits takes them (two 400 x 400 layers from 8192
    rows on); the output layer's few columns stay on their own kernel, and so does everything the query declines.
    ``gw_last``: the output layer's weight gradient as the fused backward summed it ((out_f, padded in_f) fp32, see
    fused_mlp_backward_raw): no product for that layer, the cast of its rows and of its bias gradient ride in the batched
    finish as jobs without a product (a finish launch of their own where there is no batch).
    ``first``: the same tuple for the wide layer in FRONT of the stack (_HybridMLP).  The result then has one more entry at
    its end: that layer's (dW, db) where trs_wgrad_wide_many_splits takes it together with the batch -- one product launch
    and one finish for all of them -- and None where it does not: the caller computes it as ever."""
    out = [None] * len(layers)
    batch = [k for k, t in enumerate(layers[:-1]) if t[6]]
    deep = _wgrad_deep_jobs(first, [layers[k] for k in batch]) if first is not None and first[6] and batch else None
    S_deep = _wgrad_deep_splits(deep)
    jobs = [(layers[k][0], layers[k][1], min(layers[k][0].shape[1], (layers[k][2] + 7) // 8 * 8),
             min(layers[k][1].shape[1], (layers[k][3] + 7) // 8 * 8)) for k in batch]
    S = _wgrad_many_splits(jobs) if S_deep == 0 and len({layers[k][4] for k in batch}) == 1 else 0
    # the output layer as cast-only jobs of the finish (part = gw = None, see wgrad_finish), one per row
    casts = []
    if gw_last is not None:
        _, _, out_f, in_f, dt, gb_f32, _, need_b = layers[-1]
        gw = torch.empty(out_f, in_f, dtype=dt, device=gw_last.device)
        gbias = torch.empty(out_f, dtype=dt, device=gw_last.device) if need_b else None
        # (gw_last as partial rows, (nparts, out_f, padded in_f): row r's set is gw_last[:, r])
        casts = [(None, None, gw_last[r] if gw_last.dim() == 2 else gw_last[:, r], gw[r], 0, 0, 0, in_f)
                 for r in range(out_f)] + ([(None, None, gb_f32, gbias, 0, 0, 0, out_f)] if need_b else [])
        out[-1] = (gw, gbias)

    # Any fp32 bias gradient (and gw_last) may be a set of partial rows (fused_mlp_backward_raw with ``parts``): the
    # batched finishes fold such a set themselves; whatever does not end in one is summed by colsum_parts_reduce first.
    first_out = None
    if S_deep > 0:
        ride_casts = casts if casts and layers[-1][4] == torch.bfloat16 and len(deep) + len(casts) <= 8 else []
        first_out, *rest = _wgrad_deep(deep, S_deep, ride_casts)
        if ride_casts:
            casts = []
        for k, gwb in zip(batch, rest):
            out[k] = gwb
    if S > 0:
        dev, dtype, rows = jobs[0][0].device, layers[batch[0]][4], jobs[0][0].shape[0]
        parts = [torch.empty(S, M, N, dtype=torch.float32, device=dev) for _, _, M, N in jobs]
        call("trs_wgrad_rows_many", len(jobs), _ptr_array([j[0] for j in jobs]), _i32_array([j[0].shape[1] for j in jobs]),
             _ptr_array([j[1] for j in jobs]), _i32_array([j[1].shape[1] for j in jobs]), rows,
             _i32_array([j[2] for j in jobs]), _i32_array([j[3] for j in jobs]), S, _ptr_array(parts), stream_ptr())
        gws, gbs, gbfs = [], [], []
        for k in batch:
            _, _, out_f, in_f, _, gb_f32, _, need_b = layers[k]
            gws.append(torch.empty(out_f, in_f, dtype=dtype, device=dev))
            ride = need_b and wgrad_bias_rides(out_f, in_f)      # the bias cast rides in the finish (see _wgrad_rows)
            gbs.append(torch.empty(out_f, dtype=dtype, device=dev) if ride else None)
            gbfs.append(gb_f32 if ride else None)
        ride_casts = casts if casts and layers[-1][4] == dtype and len(jobs) + len(casts) <= 8 else []
        wgrad_finish([(parts[n], gws[n], gbfs[n], gbs[n], jobs[n][2], jobs[n][3], layers[k][2], layers[k][3])
                      for n, k in enumerate(batch)] + ride_casts, S, value_dtype_code(gws[0]))
        if ride_casts:
            casts = []
        for n, k in enumerate(batch):
            gb = gbs[n]
            if gb is None and layers[k][7]:
                gb = _plain_sum(layers[k][5])[:layers[k][2]].to(dtype)
            out[k] = (gws[n], gb)
    if casts:      # no batched finish to ride in: a launch of their own
        wgrad_finish(casts, 1, value_dtype_code(casts[0][3]))
    for k, t in enumerate(layers):
        if out[k] is None:
            out[k] = _tail_layer_grads(*t[:5], _plain_sum(t[5]) if t[7] else None, *t[6:])
    return out if first is None else out + [first_out]


WGRAD_ROWS = os.environ.get("TRS_WGRAD_ROWS", "1") not in ("", "0")


def pad_cols(g: torch.Tensor, width: int) -> torch.Tensor:
    """(rows, c) bf16 -> (rows, width) with zeros behind the c columns, one launch (trs_pad_cols)"""
    g = g.contiguous()
    out = torch.empty(g.shape[0], width, dtype=g.dtype, device=g.device)
    call("trs_pad_cols", ptr(g), g.shape[1], ptr(out), width, g.shape[0], value_dtype_code(g), stream_ptr())
    return out


def _wgrad_rows(g: torch.Tensor, inp: torch.Tensor, out_f: int, in_f: int, dtype, gb_f32: Optional[torch.Tensor] = None):
    """dW = g^T @ inp over the rows (K = rows): split-K batched GEMM with fp32 partials, folded / sliced / cast by
    trs_wgrad_finish (the padding columns of g / inp are dropped there).  With ``gb_f32`` (the layer's fp32 bias
    gradient, at least out_f entries) returns (dW, db): the cast of the bias gradient rides in the same finish launch."""
    if gb_f32 is not None:
        gb = torch.empty(out_f, dtype=dtype, device=g.device)
        if wgrad_bias_rides(out_f, in_f):
            return _wgrad_rows_impl(g, inp, out_f, in_f, dtype, gb_f32, gb), gb
        gb.copy_(gb_f32[:out_f])
        return _wgrad_rows_impl(g, inp, out_f, in_f, dtype, None, None), gb
    return _wgrad_rows_impl(g, inp, out_f, in_f, dtype, None, None)


def _wgrad_rows_impl(g, inp, out_f, in_f, dtype, gb_f32, gb):
    rows = g.shape[0]
    if (WGRAD_ROWS and g.is_cuda and g.dtype == torch.bfloat16 and inp.dtype == torch.bfloat16 and g.is_contiguous()
            and inp.is_contiguous()):
        # only the columns that exist in the weight (rounded up to the kernel's 8): a 400-wide layer kept in 416-column
        # tensors is 25 x 25 output tiles instead of 26 x 26, and its 16 zero columns are not fetched
        M, N = min(g.shape[1], (out_f + 7) // 8 * 8), min(inp.shape[1], (in_f + 7) // 8 * 8)
        S = int(_abi.load().trs_wgrad_rows_splits(M, N, int(rows)))
        if S > 0:
            part = torch.empty(S, M, N, dtype=torch.float32, device=g.device)
            call("trs_wgrad_rows", ptr(g), g.shape[1], ptr(inp), inp.shape[1], rows, M, N,
                 _abi.TRS_BF16, S, ptr(part), stream_ptr())
            gw = torch.empty(out_f, in_f, dtype=dtype, device=g.device)
            wgrad_finish([(part, gw, gb_f32, gb, M, N, out_f, in_f)], S, value_dtype_code(gw))
            return gw
    S = 0
    # 192 batches measured best at 2.5 M rows (416 x 416: 1.33 ms against 1.48 at 384 and 1.53 at 96; 416 x 64: 0.49 against
    # 0.57 / 0.54): enough workgroups for the chip, partials still small against the operands
    for cand in (192, 128, 96, 64, 48, 32, 24, 16, 12, 8, 6, 4):
        if rows % cand == 0 and rows // cand >= 1024:
            S = cand
            break
    if S == 0:
        if gb is not None:
            gb.copy_(gb_f32[:out_f])
        return (g.t() @ inp)[:out_f, :in_f].contiguous().to(dtype)
    part = torch.bmm(g.view(S, rows // S, -1).transpose(1, 2), inp.view(S, rows // S, -1), out_dtype=torch.float32)
    gw = torch.empty(out_f, in_f, dtype=dtype, device=g.device)
    wgrad_finish([(part, gw, gb_f32, gb, part.shape[1], part.shape[2], out_f, in_f)], S, value_dtype_code(gw))
    return gw


def fused_mlp(x: torch.Tensor, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor]) -> torch.Tensor:
    params = []
    for w, b in zip(weights, biases):
        params += [w, b]
    return _FusedMLP.apply(x, *params)


# --------------------------------------------------------------------------------------------
# K8: the scalar head of the CTR models and its loss (csrc/head.hip)
# --------------------------------------------------------------------------------------------
class _CTRLogit(Function):
    """logit (B,1) = sum_e fm + sum_n feat + sum_k extra_k + bias in one pass; the gradient of every operand is the
    incoming column broadcast, returned as VIEWS (the lookups' backwards read a broadcast gradient as one value per
    sample: _fm_grad_operand, _GatherRows.backward) -- no kernel in the backward except the bias' batch sum."""

    @staticmethod
    def forward(ctx, fm, feat, bias, *extras):
        ref = fm if fm is not None else (feat if feat is not None else extras[0])
        require_device(ref, *[t for t in (fm, feat, bias, *extras) if t is not None])
        B = ref.shape[0]
        dt = ref.dtype
        for t in (fm, feat, bias, *extras):
            if t is not None and t.dtype != dt:
                raise ValueError("ctr_logit: every operand must have the same dtype")
        fmc = None if fm is None else fm.contiguous()
        ftc = None if feat is None else feat.reshape(B, -1).contiguous()
        E = 0 if fmc is None else fmc.shape[1]
        N = 0 if ftc is None else ftc.shape[1]
        cols, strides = [], []
        for t in extras:
            if t.dim() != 2 or t.shape[0] != B or t.shape[1] != 1:
                raise ValueError(f"ctr_logit: extra terms must be (B,1), got {tuple(t.shape)}")
            cols.append(t)
            strides.append(t.stride(0))          # a (B,1) slice of a wider row (the padded logit column of the fused MLP tail)
        out = torch.empty(B, 1, dtype=dt, device=ref.device)
        call("trs_ctr_logit_fwd", ptr(fmc), E, ptr(ftc), N, _ptr_array(cols), (ctypes.c_int64 * max(1, len(cols)))(*strides),
             len(cols), ptr(bias), B, value_dtype_code(out), ptr(out), stream_ptr())
        ctx.shapes = (None if fm is None else tuple(fm.shape), None if feat is None else tuple(feat.shape),
                      None if bias is None else tuple(bias.shape), len(extras))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        fm_shape, feat_shape, bias_shape, n_extras = ctx.shapes
        needs = ctx.needs_input_grad
        B = g.shape[0]
        g_fm = g.expand(fm_shape) if fm_shape is not None and needs[0] else None
        g_feat = None
        if feat_shape is not None and needs[1]:
            g_feat = g.reshape(B, *([1] * (len(feat_shape) - 1))).expand(feat_shape)
        g_bias = g.sum().reshape(bias_shape) if bias_shape is not None and needs[2] else None
        return (g_fm, g_feat, g_bias, *[g if needs[3 + k] else None for k in range(n_extras)])


def ctr_logit(fm: Optional[torch.Tensor] = None, feat: Optional[torch.Tensor] = None,
              extras: Sequence[torch.Tensor] = (), bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The scalar head the reference's CTR models end in, as one kernel: ``fm`` (B,E) second-order FM term (summed over
    E), ``feat`` (B,N,1) | (B,N) first-order weights of the looked-up rows (summed over N), ``extras`` up to four (B,1)
    columns (deep / CIN outputs), ``bias`` one value -> (B,1).  models/ctr/factorization_machine.py:55-66,
    deep_fm.py:75-104, xdeep_fm.py:117-121."""
    if fm is None and feat is None and not extras:
        raise ValueError("ctr_logit: nothing to sum")
    strip = lambda t: None if t is None else (t.rename(None) if t.has_names() else t)
    return _CTRLogit.apply(strip(fm), strip(feat), bias, *[strip(t) for t in extras])


class _BCEWithLogits(Function):
    @staticmethod
    def forward(ctx, logits, labels):
        require_device(logits, labels)
        x = logits.reshape(-1).contiguous()
        y = labels.reshape(-1).contiguous()
        if x.numel() != y.numel():
            raise ValueError(f"bce_with_logits: {tuple(logits.shape)} logits against {tuple(labels.shape)} labels")
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ws_bytes = size_query("trs_bce_logits_workspace_bytes", x.numel())
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        call("trs_bce_logits_fwd", ptr(x), value_dtype_code(x), ptr(y), value_dtype_code(y), x.numel(), ptr(loss), ptr(ws),
             ws_bytes, stream_ptr())
        ctx.save_for_backward(x, y)
        ctx.shape = tuple(logits.shape)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        gx = torch.empty_like(x)
        gf = g.float().contiguous()
        call("trs_bce_logits_bwd", ptr(x), value_dtype_code(x), ptr(y), value_dtype_code(y), ptr(gf), x.numel(), ptr(gx),
             stream_ptr())
        return gx.reshape(ctx.shape), None


def bce_with_logits(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """mean binary cross entropy of ``logits`` (fp32 / bf16, any shape) against ``labels`` (fp32 / bf16, same number of
    elements): an fp32 scalar.  ``F.binary_cross_entropy_with_logits(logits.float(), labels)`` in three launches
    (forward 2, backward 1) instead of ATen's cast + log-sigmoid chain + mean and their backwards."""
    return _BCEWithLogits.apply(logits, labels)


# --------------------------------------------------------------------------------------------
# Pair scores of the embedding models (MF / StarSpace) and the ranking losses over them (csrc/rank.hip)
# --------------------------------------------------------------------------------------------
PAIR_SIMS = {"dot": 0, "cosine": 1}
RANK_KINDS = {"pointwise": 0, "bpr": 1, "hinge": 2, "adaptive_hinge": 3}
RANK_REDUCTIONS = {"sum": 0, "mean": 1, "sample": 2}
# TRS_PAIR_SCORE=0: pair_scores keeps the composition (gather_rows + ATen multiply / cosine_similarity), for A/B runs
PAIR_SCORE = os.environ.get("TRS_PAIR_SCORE", "1") not in ("", "0")


def pair_score_path(E: int, dtype: torch.dtype) -> int:
    """1: the lane-group kernels (rows of 1, 2, 4 .. 64 whole 16-byte vectors), 0: one thread per (b, j) (any other E),
    -1: a dtype or E the kernels do not take.  trs_pair_score_path; a pure function, callable without a device."""
    if dtype not in (torch.float32, torch.bfloat16):
        return -1
    return size_query("trs_pair_score_path", int(E), _abi.TRS_F32 if dtype == torch.float32 else _abi.TRS_BF16)


def _sim_code(sim) -> int:
    if isinstance(sim, str):
        if sim not in PAIR_SIMS:
            raise ValueError(f"pair_scores: sim must be one of {sorted(PAIR_SIMS)}, got {sim!r}")
        return PAIR_SIMS[sim]
    if sim not in (0, 1):
        raise ValueError(f"pair_scores: bad sim code {sim!r}")
    return int(sim)


def _pair_operands(aw, a_idx, tw, t_idx, **more):
    named = dict(anchor_weight=aw, anchor_idx=a_idx, target_weight=tw, target_idx=t_idx, **more)
    for name, t in named.items():
        if t is not None and not t.is_contiguous():
            raise ValueError(f"pair_scores: {name} must be contiguous, got strides {tuple(t.stride())}")
    require_device(*named.values())
    if aw.dim() != 2 or tw.dim() != 2 or aw.shape[1] != tw.shape[1] or aw.dtype != tw.dtype:
        raise ValueError(f"pair_scores: two (V, E) tables of one dtype and width expected, got {tuple(aw.shape)} {aw.dtype} "
                         f"and {tuple(tw.shape)} {tw.dtype}")
    if a_idx.dim() != 1 or t_idx.dim() != 2 or t_idx.shape[0] != a_idx.shape[0] or t_idx.shape[1] < 1:
        raise ValueError(f"pair_scores: anchor ids (B,) and target ids (B, 1 + K) expected, got {tuple(a_idx.shape)} and "
                         f"{tuple(t_idx.shape)}")
    if a_idx.dtype != t_idx.dtype:
        raise TypeError(f"pair_scores: one index dtype expected, got {a_idx.dtype} and {t_idx.dtype}")
    return aw.shape[0], tw.shape[0], aw.shape[1], a_idx.shape[0], t_idx.shape[1] - 1, value_dtype_code(aw)


def pair_scores_forward_raw(anchor_weight: torch.Tensor, anchor_idx: torch.Tensor, target_weight: torch.Tensor,
                            target_idx: torch.Tensor, anchor_offset: int = 0, target_offset: int = 0, sim=0,
                            out_dtype: Optional[torch.dtype] = None, flag: Optional[_ErrFlag] = None) -> torch.Tensor:
    """trs_embed_pair_score_fwd as it is (no autograd): (B, 1 + K) scores of ``out_dtype`` (the tables' or fp32)."""
    Va, Vt, E, B, K, code = _pair_operands(anchor_weight, anchor_idx, target_weight, target_idx)
    out_dtype = out_dtype or anchor_weight.dtype
    if out_dtype not in (anchor_weight.dtype, torch.float32):
        raise TypeError(f"pair_scores: out_dtype must be the tables' dtype or float32, got {out_dtype}")
    out = torch.empty(B, 1 + K, dtype=out_dtype, device=anchor_weight.device)
    call("trs_embed_pair_score_fwd", ptr(anchor_weight), Va, ptr(anchor_idx), int(anchor_offset), ptr(target_weight), Vt,
         ptr(target_idx), int(target_offset), E, code, index_dtype_code(anchor_idx), B, K, _sim_code(sim), ptr(out),
         value_dtype_code(out), ptr(flag.t if flag is not None else None), stream_ptr())
    return out


def pair_scores_backward_raw(anchor_weight: torch.Tensor, anchor_idx: torch.Tensor, target_weight: torch.Tensor,
                             target_idx: torch.Tensor, g_scores: torch.Tensor, anchor_offset: int = 0,
                             target_offset: int = 0, sim=0) -> torch.Tensor:
    """trs_embed_pair_score_bwd as it is: the gradient rows (B, 2 + K, E) of the tables' dtype, ordered [anchor,
    positive, negatives], from ``g_scores`` (B, 1 + K) of the tables' dtype or fp32."""
    Va, Vt, E, B, K, code = _pair_operands(anchor_weight, anchor_idx, target_weight, target_idx, g_scores=g_scores)
    if tuple(g_scores.shape) != (B, 1 + K) or g_scores.dtype not in (anchor_weight.dtype, torch.float32):
        raise ValueError(f"pair_scores: g_scores ({B}, {1 + K}) of {anchor_weight.dtype} or float32 expected, got "
                         f"{tuple(g_scores.shape)} {g_scores.dtype}")
    dev = anchor_weight.device
    block = torch.empty(B, 2 + K, E, dtype=anchor_weight.dtype, device=dev)
    ws_bytes = size_query("trs_pair_score_bwd_workspace_bytes", B, K, E, code)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    call("trs_embed_pair_score_bwd", ptr(anchor_weight), Va, ptr(anchor_idx), int(anchor_offset), ptr(target_weight), Vt,
         ptr(target_idx), int(target_offset), E, code, index_dtype_code(anchor_idx), B, K, _sim_code(sim), ptr(g_scores),
         value_dtype_code(g_scores), ptr(block), ptr(ws), ws_bytes, stream_ptr())
    return block


_pair_offsets = {}        # (device, anchor offset, target offset, columns) -> the per-column offsets of the id matrix


def _pair_offset_columns(dev, a_off: int, t_off: int, na: int, nt: int) -> Optional[torch.Tensor]:
    if a_off == 0 and t_off == 0:
        return None
    key = (dev, a_off, t_off, na, nt)
    t = _pair_offsets.get(key)
    if t is None:
        t = _pair_offsets[key] = torch.tensor([a_off] * na + [t_off] * nt, dtype=torch.int64, device=dev)
    return t


class _PairScores(Function):
    """ids -> (B, 1 + K) scores in one kernel; nothing but the ids is saved.  The backward writes the gradient rows
    (B, 2 + K, E) and walks the row buckets of the (B, 2 + K) id matrix: ONE walk for a shared table (one gradient, or one
    fused optimizer step), two walks over its two column ranges for two tables."""

    @staticmethod
    def forward(ctx, aw, a_idx, tw, t_idx, a_off, t_off, sim, out_dtype, opt, track):
        shared = tw is None
        wa = aw.contiguous()
        wt = wa if shared else tw.contiguous()
        flag = _ErrFlag(wa.device)
        out = pair_scores_forward_raw(wa, a_idx, wt, t_idx, a_off, t_off, sim, out_dtype, flag)
        flag.check("pair_scores")
        ctx.args = (a_off, t_off, sim, opt, shared)
        K1 = t_idx.shape[1]
        dev = wa.device
        # ``track``: the caller's grad mode (needs_input_grad says True under torch.no_grad() too, and the forward itself
        # always runs with grad mode off): no backward, no id matrix, no buckets
        need = track and (ctx.needs_input_grad[0] or (not shared and ctx.needs_input_grad[2]))
        ids = ()
        if need and a_idx.shape[0] > 0:
            prefetch = not torch.cuda.is_current_stream_capturing()      # a capture stays one chain on one stream
            if shared:
                ids = (torch.cat([a_idx.unsqueeze(1), t_idx], dim=1),)
                if prefetch:
                    prefetch_row_buckets(ids[0], _pair_offset_columns(dev, a_off, t_off, 1, K1), wa.shape[0])
            else:
                ids = (a_idx.unsqueeze(1),)
                if prefetch and ctx.needs_input_grad[0]:
                    prefetch_row_buckets(ids[0], _pair_offset_columns(dev, a_off, 0, 1, 0), wa.shape[0])
                if prefetch and ctx.needs_input_grad[2]:
                    prefetch_row_buckets(t_idx, _pair_offset_columns(dev, 0, t_off, 0, K1), wt.shape[0])
        ctx.save_for_backward(aw, a_idx, tw, t_idx, *ids)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        aw, a_idx, tw, t_idx = ctx.saved_tensors[:4]
        a_off, t_off, sim, opt, shared = ctx.args
        need_a, need_t = ctx.needs_input_grad[0], (not shared and ctx.needs_input_grad[2])
        tail = (None,) * 6
        if not (need_a or need_t):
            return (None, None, None, None, *tail)
        if a_idx.shape[0] == 0:      # no sample: zero gradients
            za = torch.zeros_like(aw) if need_a and opt is None else None
            zt = torch.zeros_like(tw) if need_t and opt is None else None
            return (za, None, zt, None, *tail)
        _adopt_grads(g)
        ids = ctx.saved_tensors[4]
        wa = aw.contiguous()
        wt = wa if shared else tw.contiguous()
        K1 = t_idx.shape[1]
        dev = wa.device
        block = pair_scores_backward_raw(wa, a_idx, wt, t_idx, g.contiguous(), a_off, t_off, sim)
        if shared:
            rb = row_buckets(ids, _pair_offset_columns(dev, a_off, t_off, 1, K1), wa.shape[0])
            return (_apply_or_grad(rb, aw, opt, g_rows=block), None, None, None, *tail)
        g_a = g_t = None
        if need_a:
            rb = row_buckets(ids, _pair_offset_columns(dev, a_off, 0, 1, 0), wa.shape[0])
            g_a = _apply_or_grad(rb, aw, opt, g_rows=block, g_rows_batch_stride=K1 + 1)
        if need_t:
            rb = row_buckets(t_idx, _pair_offset_columns(dev, 0, t_off, 0, K1), wt.shape[0])
            g_t = _apply_or_grad(rb, tw, opt, g_rows=block[:, 1:], g_rows_batch_stride=K1 + 1)
        return (g_a, None, g_t, None, *tail)


def _pair_scores_composition(aw, a_idx, tw, t_idx, a_off, t_off, sim, out_dtype, opt):
    """gather_rows + ATen: the A/B baseline of pair_scores (TRS_PAIR_SCORE=0); forms the (B, 1 + K, E) block"""
    dev = aw.device
    a = gather_rows(aw, a_idx.unsqueeze(1), _pair_offset_columns(dev, a_off, 0, 1, 0), opt=opt)              # (B, 1, E)
    t = gather_rows(aw if tw is None else tw, t_idx, _pair_offset_columns(dev, 0, t_off, 0, t_idx.shape[1]), opt=opt)
    if out_dtype is not None and out_dtype != a.dtype:
        a, t = a.to(out_dtype), t.to(out_dtype)
    if sim == 0:
        return (a * t).sum(dim=2)
    return torch.nn.functional.cosine_similarity(a, t, dim=2)


def pair_scores(anchor_weight: torch.Tensor, anchor_idx: torch.Tensor, target_weight: Optional[torch.Tensor],
                target_idx: torch.Tensor, anchor_offset: Optional[int] = None, target_offset: Optional[int] = None,
                sim="dot", out_dtype: Optional[torch.dtype] = None, opt=None) -> torch.Tensor:
    """scores[b, j] = sim(anchor_weight[anchor_idx[b] + anchor_offset], target_weight[target_idx[b, j] + target_offset]):
    (B,) anchor ids and (B, 1 + K) target ids (column 0 the positive, the others sampled negatives; K >= 0) -> (B, 1 + K)
    in one HIP pass per direction (csrc/rank.hip).  ``sim``: 'dot' | 'cosine' (ATen's cosine_similarity, eps 1e-8).
    ``target_weight`` None or ``anchor_weight`` itself: ONE shared table, which then gets one gradient from one bucket walk
    (or one fused step with ``opt``).  ``out_dtype``: the tables' dtype (default) or float32.  The anchor row is read once
    per sample, no (B, 1 + K, E) block is formed, nothing but the ids is kept for the backward.  An id outside its table
    scores as a zero row, receives no gradient and raises the index flag."""
    sim = _sim_code(sim)
    a_idx, t_idx = _as_index(anchor_idx), _as_index(target_idx)
    if a_idx.dim() == 2 and a_idx.shape[1] == 1:
        a_idx = a_idx.reshape(-1)
    if t_idx.dim() == 1:
        t_idx = t_idx.unsqueeze(1)
    if a_idx.dtype != t_idx.dtype:
        a_idx, t_idx = a_idx.long(), t_idx.long()
    tw = None if target_weight is None or target_weight is anchor_weight else target_weight
    a_off, t_off = int(anchor_offset or 0), int(target_offset or 0)
    _pair_operands(anchor_weight.contiguous(), a_idx, (anchor_weight if tw is None else tw).contiguous(), t_idx)
    if pair_score_path(anchor_weight.shape[1], anchor_weight.dtype) < 0:
        raise TypeError(f"pair_scores: unsupported table dtype {anchor_weight.dtype}")
    if not PAIR_SCORE:
        return _pair_scores_composition(anchor_weight, a_idx, tw, t_idx, a_off, t_off, sim, out_dtype, opt)
    return _PairScores.apply(anchor_weight, a_idx, tw, t_idx, a_off, t_off, sim, out_dtype, opt, torch.is_grad_enabled())


_row_ids = {}       # (device, B) -> (2 b, 2 b + 1): the rows of a (B, 2, E) block seen as a (2 B, E) table


class _BlockPairScore(Function):
    """sim of the two rows of every sample of a (B, 2, E) block already in memory (the layers' input): the pair-score
    kernels over the block as a (2 B, E) table with ids (2 b, 2 b + 1); the (B, 2, E) gradient rows ARE the gradient."""

    @staticmethod
    def forward(ctx, x, sim):
        B = x.shape[0]
        key = (x.device, B)
        ids = _row_ids.get(key)
        if ids is None:
            if len(_row_ids) > 16:
                _row_ids.clear()
            even = torch.arange(0, 2 * B, 2, dtype=torch.int32, device=x.device)
            ids = _row_ids[key] = (even, (even + 1).unsqueeze(1).contiguous())
        xc = x.contiguous()
        ctx.save_for_backward(xc, *ids)
        ctx.sim = sim
        rows = xc.view(2 * B, xc.shape[2])
        return pair_scores_forward_raw(rows, ids[0], rows, ids[1], 0, 0, sim)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xc, a_idx, t_idx = ctx.saved_tensors
        rows = xc.view(-1, xc.shape[2])
        return pair_scores_backward_raw(rows, a_idx, rows, t_idx, g.contiguous(), 0, 0, ctx.sim), None


def block_pair_score(x: torch.Tensor, sim="dot") -> torch.Tensor:
    """(B, 2, E) -> (B, 1): sim(x[:, 0], x[:, 1]) in one kernel per direction (GeneralizedMatrixFactorizationLayer,
    StarSpaceLayer); 'dot' | 'cosine'."""
    x = x.rename(None) if x.has_names() else x
    if x.dim() != 3 or x.shape[1] != 2:
        raise ValueError(f"block_pair_score: (B, 2, E) expected, got {tuple(x.shape)}")
    require_device(x)
    if pair_score_path(x.shape[2], x.dtype) < 0:
        raise TypeError(f"block_pair_score: unsupported dtype {x.dtype}")
    return _BlockPairScore.apply(x, _sim_code(sim))


def _rank_kind_code(kind) -> int:
    if isinstance(kind, str):
        if kind not in RANK_KINDS:
            raise ValueError(f"rank_loss: kind must be one of {sorted(RANK_KINDS)}, got {kind!r}")
        return RANK_KINDS[kind]
    if kind not in (0, 1, 2, 3):
        raise ValueError(f"rank_loss: bad kind code {kind!r}")
    return int(kind)


def rank_reduction_code(reduction) -> int:
    """'sum' | torch.sum -> 0, 'mean' | torch.mean -> 1, 'sample' -> 2 (the sum over the kept samples' terms divided by the
    number of kept samples: the reference's apply_mask rule); anything else raises.  Callable without a device."""
    if isinstance(reduction, int) and not isinstance(reduction, bool) and reduction in (0, 1, 2):
        return reduction
    if reduction is torch.sum:
        return 0
    if reduction is torch.mean:
        return 1
    if isinstance(reduction, str) and reduction in RANK_REDUCTIONS:
        return RANK_REDUCTIONS[reduction]
    raise ValueError(f"rank_loss: reduction must be 'sum', 'mean', 'sample', torch.sum or torch.mean, got {reduction!r}")


def _rank_views(pos, neg):
    """(pos, pos row stride, neg, neg row stride, B, K) of a (B, 1 + K) score matrix (``neg`` None) or a (B[, 1]) /
    (B, K) pair"""
    if neg is None:
        if pos.dim() != 2 or pos.shape[1] < 2:
            raise ValueError(f"rank_loss: a (B, 1 + K) score matrix with K >= 1 expected, got {tuple(pos.shape)}")
        s = pos.contiguous()
        return s, s.shape[1], s[:, 1:], s.shape[1], s.shape[0], s.shape[1] - 1
    p = pos.reshape(-1).contiguous()
    if neg.dim() != 2 or neg.shape[0] != p.shape[0] or neg.shape[1] < 1 or neg.dtype != p.dtype:
        raise ValueError(f"rank_loss: pos (B,) | (B, 1) and neg (B, K >= 1) of one dtype expected, got {tuple(pos.shape)} "
                         f"{pos.dtype} and {tuple(neg.shape)} {neg.dtype}")
    n = neg.contiguous()
    return p, 1, n, n.shape[1], n.shape[0], n.shape[1]


def rank_loss_forward_raw(pos: torch.Tensor, neg: Optional[torch.Tensor], kind, margin: float = 1.0,
                          mask: Optional[torch.Tensor] = None, reduction="sum"):
    """trs_rank_loss_fwd as it is (no autograd): ``(loss, denom)``, two fp32 device scalars."""
    require_device(pos, neg, mask)
    p, ps, n, ns, B, K = _rank_views(pos, neg)
    if mask is not None and (mask.dtype != torch.bool or tuple(mask.shape) != (B,)):
        raise ValueError(f"rank_loss: mask ({B},) of torch.bool expected, got {tuple(mask.shape)} {mask.dtype}")
    mask = None if mask is None else mask.contiguous()
    loss = torch.zeros((), dtype=torch.float32, device=p.device) if B == 0 else \
        torch.empty((), dtype=torch.float32, device=p.device)
    denom = torch.empty((), dtype=torch.float32, device=p.device)
    ws_bytes = size_query("trs_rank_loss_workspace_bytes", B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=p.device)
    call("trs_rank_loss_fwd", ptr(p), ps, ptr(n), ns, value_dtype_code(p), ptr(mask), B, K, _rank_kind_code(kind),
         float(margin), rank_reduction_code(reduction), ptr(loss), ptr(denom), ptr(ws), ws_bytes, stream_ptr())
    return loss, denom


def rank_loss_backward_raw(pos: torch.Tensor, neg: Optional[torch.Tensor], kind, margin: float = 1.0,
                           mask: Optional[torch.Tensor] = None, reduction="sum", gout: Optional[torch.Tensor] = None,
                           denom: Optional[torch.Tensor] = None):
    """trs_rank_loss_bwd as it is: ``(g_pos, g_neg)`` shaped like the operands -- for a (B, 1 + K) score matrix
    (``neg`` None) ``g_pos`` is the whole (B, 1 + K) gradient and ``g_neg`` None."""
    require_device(pos, neg, mask, gout, denom)
    p, ps, n, ns, B, K = _rank_views(pos, neg)
    mask = None if mask is None else mask.contiguous()
    if neg is None:
        g = torch.empty_like(p)
        gp, gps, gn, gns = g, K + 1, g[:, 1:], K + 1
    else:
        gp, gn = torch.empty_like(p), torch.empty_like(n)
        gps, gns = 1, K
    call("trs_rank_loss_bwd", ptr(p), ps, ptr(n), ns, value_dtype_code(p), ptr(mask), B, K, _rank_kind_code(kind),
         float(margin), rank_reduction_code(reduction), ptr(gout), ptr(denom), ptr(gp), gps, ptr(gn), gns, stream_ptr())
    return (gp, None) if neg is None else (gp.reshape(pos.shape), gn)


class _RankLoss(Function):
    @staticmethod
    def forward(ctx, pos, neg, kind, margin, mask, reduction):
        loss, denom = rank_loss_forward_raw(pos, neg, kind, margin, mask, reduction)
        ctx.save_for_backward(pos, neg, mask, denom)
        ctx.args = (kind, margin, reduction)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pos, neg, mask, denom = ctx.saved_tensors
        kind, margin, reduction = ctx.args
        gp, gn = rank_loss_backward_raw(pos, neg, kind, margin, mask, reduction, g.float().contiguous(), denom)
        return gp, gn, None, None, None, None


def rank_loss(pos: torch.Tensor, neg: Optional[torch.Tensor], kind, margin: float = 1.0,
              mask: Optional[torch.Tensor] = None, reduction="sum") -> torch.Tensor:
    """Ranking loss of positive scores ``pos`` (B,) | (B, 1) against negative scores ``neg`` (B, K), fp32 or bf16 -> an
    fp32 scalar, forward two launches, backward one.  ``neg=None``: ``pos`` is the (B, 1 + K) score matrix of
    ``pair_scores`` (column 0 the positive), read in place, and its gradient is written as one matrix.
    ``kind``: 'pointwise' (1 - sigmoid(p)) + sigmoid(n) | 'bpr' softplus(-(p - n)) | 'hinge' max(0, margin - p + n) |
    'adaptive_hinge' max(0, margin - p + max_k n), one term per sample.  ``mask`` (B,) bool drops samples.
    ``reduction``: 'sum' | 'mean' (over the kept terms) | 'sample' (the sum over the number of kept SAMPLES: the
    reference's masked rule); torch.sum / torch.mean are accepted for the first two."""
    strip = lambda t: None if t is None else (t.rename(None) if t.has_names() else t)
    pos, neg, mask = strip(pos), strip(neg), strip(mask)
    value_dtype_code(pos)
    return _RankLoss.apply(pos, neg, _rank_kind_code(kind), float(margin), mask, rank_reduction_code(reduction))

"""Fused sparse optimizers for embedding tables.

The reference trains every parameter with a dense optimizer over a dense ``V x E`` gradient
(trainer/torecsys_pipeline.py:562-578).  For SGD and Adagrad (no momentum, no weight decay) the dense step only
changes rows that were looked up, so it can be applied by the kernel that reduces the bucketed gradient
(``FusedSparseAdam`` applies the lazy ``torch.optim.SparseAdam`` rule instead -- dense Adam also decays the moments
of rows nobody looked up, which is exactly the full-table sweep a 1 B-row table cannot afford):
``module.set_fused_optimizer(FusedSparseSGD(lr))`` makes the backward pass update the table rows in place --
bit-for-bit the same rows a dense ``torch.optim.SGD`` / ``Adagrad`` step would produce up to fp32 summation order --
without ever forming the dense gradient or sweeping the table.  The other parameters keep a normal optimizer.

State (Adagrad accumulators, Adam moments and step counts) is kept per table, keyed by the ``nn.Parameter`` object, so
it follows ``module.to(...)`` (the state tensors move to the table's device on the next step) and can be saved /
restored with ``state_dict(named_parameters)`` / ``load_state_dict(sd, named_parameters)``.

``capturable=True`` keeps what changes from step to step on the DEVICE, so a step captured into a hipGraph
(``graph.GraphedStep``) stays correct over its replays: the learning rate is a one-element fp32 tensor that ``set_lr()``
writes (replays see the new value, no ``recapture()``), and Adam keeps a per-table step counter (int64) and its
bias-corrected step size there, advanced by a one-thread kernel in front of every update.  Eager and replayed steps of a
capturable optimizer run the same kernels.  The default (``capturable=False``) passes these scalars by value, as before.

``FusedSparseRowWiseAdagrad`` is the rule for tables whose ``V x E`` fp32 of Adagrad / Adam state does not fit beside them:
ONE fp32 accumulator per table row (``(V,)``: 0.5 GB for a 125 M-row x 64 bf16 shard of 16 GB, where Adagrad keeps 32 GB
and Adam 64 GB -- sizes by arithmetic), advanced by the mean square of the row's summed gradient.  It lives in the
lane-group walk only: tables whose rows are not 1, 2, 4 .. 64 whole 16-byte vectors are refused (``E == 1`` excepted,
where the rule IS element-wise Adagrad and runs as such).

``stochastic_rounding=True`` (every optimizer here; off by default) is for bf16 tables, which are trained in place with no
fp32 master copy: the new weight of a touched row exists in fp32 only inside the kernel, and stored round-to-nearest an
update below half a bf16 ulp of the weight (2^-9 at 1.0) is dropped, at every step.  With the option the store rounds up or
down with the probability that makes its expectation the fp32 value.  The random bits are a counter-based hash of
``(seed, update number of the table, element position)`` (Philox4x32-10; the rule is spelled out in include/trs_abi.h), so
a run is reproducible, two lookups of one table in one backward draw different bits, and a checkpointed run resumes the
same bit stream: ``state_dict`` carries the seed and every table's update counter.  A ``capturable`` optimizer keeps the
counter on the device, advanced by a one-thread kernel in front of every update, so hipGraph replays draw fresh bits.
fp32 tables ignore the option: there is nothing to round.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Tuple

import torch


class _FusedSparse:
    kind = 0
    _buffers: Tuple[str, ...] = ()          # names of the per-table fp32 state tensors

    def __init__(self, lr: float, eps: float = 0.0, capturable: bool = False, stochastic_rounding: bool = False,
                 seed: int = 0):
        if lr < 0:
            raise ValueError(f"invalid learning rate {lr}")
        if not isinstance(capturable, bool):
            raise TypeError(f"capturable must be a bool, got {type(capturable).__name__}")
        if not isinstance(stochastic_rounding, bool):
            raise TypeError(f"stochastic_rounding must be a bool, got {type(stochastic_rounding).__name__}")
        self.lr, self.eps = float(lr), float(eps)
        self._capturable = capturable
        # (flag, seed) in one tuple: 'hyper' of state_dict() collects the plain numbers of __dict__
        self._sr: Tuple[bool, int] = (stochastic_rounding, self._check_seed(seed))
        self._lr_dev: Dict[torch.device, torch.Tensor] = {}      # capturable: the learning rate, one fp32 per device
        self._state: Dict[object, dict] = {}

    @property
    def capturable(self) -> bool:
        return self._capturable

    # ---- stochastic rounding ---------------------------------------------------------------------------
    @staticmethod
    def _check_seed(seed) -> int:
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise TypeError(f"seed must be an int, got {type(seed).__name__}")
        if not 0 <= seed < 1 << 64:
            raise ValueError(f"seed {seed} outside [0, 2^64)")
        return seed

    @property
    def stochastic_rounding(self) -> bool:
        return self._sr[0]

    @property
    def seed(self) -> int:
        return self._sr[1]

    def next_update(self, table: torch.Tensor, key=None) -> Tuple[int, Optional[torch.Tensor]]:
        """The number of the update of ``table`` that starts now (the first is 1), as the stochastic-rounding entries take
        it: ``(t, None)`` counted on the host, or ``(0, counter)`` for a capturable optimizer, whose int64 counter lives
        on the device and is advanced by the caller (trs_sr_advance) on the stream of the update."""
        if not self._sr[0]:
            raise RuntimeError("next_update: the optimizer was not built with stochastic_rounding=True")
        st = self._entry(table, key)
        if self._capturable:
            return 0, st["sr_t_dev"]
        if table.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            # the update number is passed by value: a captured launch would draw the capture-time bits at every replay
            raise RuntimeError("torecsys_amd: stochastic rounding inside a hipGraph capture needs a fused optimizer built "
                               "with capturable=True (the update counter must live on the device)")
        st["sr_t"] = st.get("sr_t", 0) + 1
        return st["sr_t"], None

    @staticmethod
    def _sr_t_of(st: dict) -> int:
        # a capturable optimizer counts on the device: one host read per table, at checkpoint time only
        return int(st["sr_t_dev"].item()) if "sr_t_dev" in st else int(st.get("sr_t", 0))

    # ---- learning rate ---------------------------------------------------------------------------------
    def set_lr(self, lr: float) -> None:
        """Change the learning rate.  Capturable optimizers write it into their device scalar (a ``fill_`` on the
        current stream: call it between replays, not inside a capture); captured steps read the new value."""
        if isinstance(lr, bool) or not isinstance(lr, (int, float)):
            raise TypeError(f"learning rate must be a number, got {type(lr).__name__}")
        if not lr >= 0:
            raise ValueError(f"invalid learning rate {lr}")
        self.lr = float(lr)
        for t in self._lr_dev.values():
            t.fill_(self.lr)

    def lr_tensor(self, device) -> torch.Tensor:
        """the device-resident learning rate of a capturable optimizer (created on first use, outside any capture)"""
        if not self._capturable:
            raise RuntimeError("lr_tensor: the optimizer was not built with capturable=True")
        device = torch.device(device)
        t = self._lr_dev.get(device)
        if t is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("torecsys_amd: a capturable fused optimizer met a table on a new device inside a "
                                   "capture; run one eager step first (GraphedStep's warm-up does)")
            t = self._lr_dev[device] = torch.full((1,), self.lr, dtype=torch.float32, device=device)
        return t

    # ---- per-table state -------------------------------------------------------------------------------
    def _init_value(self, name: str) -> float:
        return 0.0

    def _state_shape(self, table: torch.Tensor) -> tuple:
        """shape of every per-table state tensor in ``_buffers``"""
        return tuple(table.shape)

    def _entry(self, table: torch.Tensor, key=None) -> dict:
        """state of one table.  ``key`` is the nn.Parameter the rows belong to (falls back to the storage address for
        bare tensors); tensors follow the table's device and are rebuilt if its shape changed."""
        k = id(key) if key is not None else (table.data_ptr(), tuple(table.shape))
        st = self._state.get(k)
        if st is None:
            st = self._state[k] = {"step": 0, "ref": key}
        for name in self._buffers:
            t = st.get(name)
            if t is None or tuple(t.shape) != self._state_shape(table):
                st[name] = torch.full(self._state_shape(table), self._init_value(name), dtype=torch.float32,
                                      device=table.device)
            elif t.device != table.device:
                st[name] = t.to(table.device)
        for name, dtype in self._all_scalars:
            t = st.get(name)
            if t is None:
                if name == "sr_t_dev" and table.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                    # as lr_tensor(): a counter created inside a capture would be reset by every replay
                    raise RuntimeError("torecsys_amd: a capturable fused optimizer with stochastic rounding met a new "
                                       "table inside a capture; run one eager step first (GraphedStep's warm-up does)")
                first = {"step_dev": st["step"], "sr_t_dev": st.get("sr_t", 0)}.get(name, 0)
                st[name] = torch.full((1,), first, dtype=dtype, device=table.device)
            elif t.device != table.device:
                st[name] = t.to(table.device)
        return st

    @property
    def _scalars(self) -> Tuple[tuple, ...]:
        """(name, dtype) of the per-table one-element device tensors of a capturable optimizer"""
        return ()

    @property
    def _all_scalars(self) -> Tuple[tuple, ...]:
        sr = (("sr_t_dev", torch.int64),) if self._capturable and self._sr[0] else ()
        return tuple(self._scalars) + sr

    @staticmethod
    def _step_of(st: dict) -> int:
        # a capturable Adam counts on the device: one host read per table, at checkpoint time only
        return int(st["step_dev"].item()) if "step_dev" in st else int(st["step"])

    def state_for(self, table: torch.Tensor, key=None):
        return None

    # ---- checkpointing ---------------------------------------------------------------------------------
    def state_dict(self, named_parameters: Optional[Iterable] = None) -> dict:
        """{'hyper': {...}, 'tables': {name: {'step': int, <buffer>: tensor}}}; ``named_parameters`` (e.g.
        ``model.named_parameters()``) gives the tables their names -- tables it does not cover are 'table<i>'.  With
        ``stochastic_rounding`` also 'stochastic_rounding': {'seed': int} and, per table, 'sr_t': its update counter."""
        names = {id(p): n for n, p in (named_parameters or [])}
        tables = {}
        for i, (k, st) in enumerate(self._state.items()):
            name = names.get(k if isinstance(k, int) else None, f"table{i}")
            tables[name] = {"step": self._step_of(st), **{b: st[b].detach().clone() for b in self._buffers if b in st}}
            if self._sr[0]:
                tables[name]["sr_t"] = self._sr_t_of(st)
        sd = {"hyper": {k: v for k, v in self.__dict__.items()
                        if isinstance(v, (int, float)) and not isinstance(v, bool)}, "tables": tables}
        if self._sr[0]:
            sd["stochastic_rounding"] = {"seed": self._sr[1]}
        return sd

    def load_state_dict(self, sd: dict, named_parameters: Iterable) -> None:
        """State tensors (a capturable Adam's device step counter included) are re-created: a graph captured before the
        load still points at the old ones and must be ``recapture()``d."""
        params = dict(named_parameters)
        for k, v in sd.get("hyper", {}).items():
            setattr(self, k, v)
        self.set_lr(self.lr)          # a capturable optimizer's device scalar follows the loaded learning rate
        if "stochastic_rounding" in sd:      # the checkpointed run rounded stochastically: continue its bit stream
            self._sr = (True, self._check_seed(sd["stochastic_rounding"]["seed"]))
        for name, entry in sd.get("tables", {}).items():
            if name not in params:
                raise KeyError(f"load_state_dict: no parameter named {name!r}")
            p = params[name]
            st = self._state[id(p)] = {"step": int(entry.get("step", 0)), "ref": p}
            if "sr_t" in entry:
                st["sr_t"] = int(entry["sr_t"])
            for b in self._buffers:
                if b in entry:
                    if tuple(entry[b].shape) != self._state_shape(p):
                        raise ValueError(f"load_state_dict: state {b!r} of {name!r} has shape {tuple(entry[b].shape)}, "
                                         f"the parameter has {tuple(p.shape)}"
                                         + ("" if self._state_shape(p) == tuple(p.shape)
                                            else f" and wants {self._state_shape(p)}"))
                    st[b] = entry[b].to(device=p.device, dtype=torch.float32).clone()


class FusedSparseSGD(_FusedSparse):
    """w[r] -= lr * g[r] for every looked-up row r (== torch.optim.SGD(lr) without momentum / weight decay)."""
    kind = 1


class FusedSparseAdagrad(_FusedSparse):
    """state[r] += g[r]^2 ; w[r] -= lr * g[r] / (sqrt(state[r]) + eps)   (== torch.optim.Adagrad(lr, eps=eps))."""
    kind = 2
    _buffers = ("sum",)

    def __init__(self, lr: float = 1e-2, eps: float = 1e-10, initial_accumulator_value: float = 0.0,
                 capturable: bool = False, stochastic_rounding: bool = False, seed: int = 0):
        super().__init__(lr, eps, capturable, stochastic_rounding, seed)
        self.initial = float(initial_accumulator_value)

    def _init_value(self, name: str) -> float:
        return self.initial

    def state_for(self, table: torch.Tensor, key=None):
        return self._entry(table, key)["sum"]


class FusedSparseRowWiseAdagrad(FusedSparseAdagrad):
    """G[r,:] = summed gradient of row r;  s[r] += mean_e(G[r,e]^2);  w[r,e] -= lr * G[r,e] / (sqrt(s[r]) + eps) for
    every looked-up row r (the "exact row-wise Adagrad" of embedding libraries): state ``"sum"`` is ``(V,)`` fp32, one
    accumulator per table row.  The mean is taken in a fixed order (include/trs_abi.h, TRS_OPT_ROWWISE)."""
    rowwise = True

    def _state_shape(self, table: torch.Tensor) -> tuple:
        return (int(table.shape[0]),)


class FusedSparseAdam(_FusedSparse):
    """Lazy Adam on the looked-up rows, == ``torch.optim.SparseAdam(lr, betas, eps)`` on the coalesced sparse gradient:
    m[r] += (g[r]-m[r])(1-b1);  v[r] += (g[r]^2-v[r])(1-b2);  w[r] -= lr*sqrt(1-b2^t)/(1-b1^t) * m[r]/(sqrt(v[r])+eps).
    ``t`` counts the steps applied to each table (one per backward pass through it)."""
    kind = 3
    _buffers = ("exp_avg", "exp_avg_sq")

    def __init__(self, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, capturable: bool = False,
                 stochastic_rounding: bool = False, seed: int = 0):
        super().__init__(lr, eps, capturable, stochastic_rounding, seed)
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas {betas}")
        self.beta1, self.beta2 = float(betas[0]), float(betas[1])

    def state_for(self, table: torch.Tensor, key=None):
        st = self._entry(table, key)
        return st["exp_avg"], st["exp_avg_sq"]

    @property
    def _scalars(self):
        return (("step_dev", torch.int64), ("step_size_dev", torch.float32)) if self._capturable else ()

    def step_tensors(self, table: torch.Tensor, key=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """capturable: the table's device step counter (int64) and bias-corrected step size (fp32), one element each"""
        st = self._entry(table, key)
        return st["step_dev"], st["step_size_dev"]

    def next_step_size(self, table: torch.Tensor, key=None) -> float:
        if self._capturable:
            raise RuntimeError("next_step_size: a capturable FusedSparseAdam steps on the device (trs_adam_step_size)")
        st = self._entry(table, key)
        st["step"] += 1
        t = st["step"]
        return self.lr * (1.0 - self.beta2 ** t) ** 0.5 / (1.0 - self.beta1 ** t)

"""Weight gradients of the two 400 x 400 tail layers of the deep branch (gz[0] (rows, 416) against h1 (rows, 512) and
gz[1] (rows, 416) against hidden[0] (rows, 416)): trs_wgrad_rows_many + one trs_wgrad_finish against the per-layer calls
(two trs_wgrad_rows + two trs_wgrad_finish), stand-alone with events at 65 536 rows, interleaved in one process.
usage (GPU box): python tools/wgrad_many_probe.py [--rows R]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from torecsys_amd import _abi
from torecsys_amd import functional as F_

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--iters", type=int, default=30)
args = ap.parse_args()

lib = _abi.load()
dev = torch.device("cuda:0")
torch.manual_seed(0)
rows, M, N = args.rows, 400, 400
gs = [torch.randn(rows, 416, device=dev).bfloat16() for _ in range(2)]
xs = [(torch.randn(rows, 512, device=dev) * 0.5).bfloat16(), (torch.randn(rows, 416, device=dev) * 0.5).bfloat16()]
gbf = [torch.randn(416, device=dev) for _ in range(2)]
refs = [g[:, :M].float().t() @ x[:, :N].float() for g, x in zip(gs, xs)]
ia = F_._i32_array
Ms, Ns, ldg, ldx = ia([M, M]), ia([N, N]), ia([g.shape[1] for g in gs]), ia([x.shape[1] for x in xs])

S1 = int(lib.trs_wgrad_rows_splits(M, N, rows))
S = int(lib.trs_wgrad_rows_many_splits(2, Ms, Ns, ldg, ldx, rows))
assert S1 > 0 and S > 0, (S1, S)
part1 = [torch.empty(S1, M, N, dtype=torch.float32, device=dev) for _ in range(2)]
part = [torch.empty(S, M, N, dtype=torch.float32, device=dev) for _ in range(2)]
gw1 = [torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(2)]
gw = [torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(2)]
gb = [torch.empty(M, dtype=torch.bfloat16, device=dev) for _ in range(2)]
pa = F_._ptr_array


def per_layer():
    for k in range(2):
        _abi.call("trs_wgrad_rows", _abi.ptr(gs[k]), gs[k].shape[1], _abi.ptr(xs[k]), xs[k].shape[1], rows, M, N, _abi.TRS_BF16,
                  S1, _abi.ptr(part1[k]), _abi.stream_ptr())
        F_.wgrad_finish([(part1[k], gw1[k], gbf[k], gb[k], M, N, M, N)], S1, _abi.TRS_BF16)


def many_kernel():
    _abi.call("trs_wgrad_rows_many", 2, pa(gs), ldg, pa(xs), ldx, rows, Ms, Ns, S, pa(part), _abi.stream_ptr())


def many_finish():
    F_.wgrad_finish([(part[k], gw[k], gbf[k], gb[k], M, N, M, N) for k in range(2)], S, _abi.TRS_BF16)


def many():
    many_kernel()
    many_finish()


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


arms = {"per-layer (2 x rows + 2 x finish)": per_layer, "many + one finish": many, "many, product only": many_kernel,
        "many, finish only": many_finish}
for fn in arms.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
ts = {k: [] for k in arms}
for _ in range(args.iters):      # interleaved rounds, one event pair per call
    for k, fn in arms.items():
        ts[k].append(once(fn))
print(f"rows {rows}: per-layer S={S1}, batched S={S} per job")
for k, v in ts.items():
    print(f"  {k:36s} med {statistics.median(v):7.1f} min {min(v):7.1f} us")
for k in range(2):
    e1 = float((gw1[k].float() - refs[k]).abs().max() / refs[k].abs().max())
    e = float((gw[k].float() - refs[k]).abs().max() / refs[k].abs().max())
    d = float((gw[k].float() - gw1[k].float()).abs().max() / gw1[k].float().abs().max())
    print(f"  job {k}: rel err against the fp32 product per-layer {e1:.2e}, batched {e:.2e}; batched against per-layer {d:.2e}")

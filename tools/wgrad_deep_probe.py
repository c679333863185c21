"""Weight gradients of the DeepFM / xDeepFM deep branch (2496-400-400-400): the first layer's cur (rows, 2496) against g1
(rows, 512) and the two tail layers' h1 (rows, 512) / hidden[0] (rows, 416) against gz[0] / gz[1] (rows, 416).  Today's
two products with their two finishes (trs_wgrad_rows_many + trs_wgrad_finish, trs_wgrad_wide + trs_wgrad_finish_t)
against the merged pair (trs_wgrad_wide_many + one trs_wgrad_finish_t), stand-alone with events, interleaved in one
process.
usage (GPU box): python tools/wgrad_deep_probe.py [--rows R [R ...]]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from torecsys_amd import _abi
from torecsys_amd import functional as F_

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[65536])
ap.add_argument("--iters", type=int, default=30)
args = ap.parse_args()

lib = _abi.load()
dev = torch.device("cuda:0")
ia, pa = F_._i32_array, F_._ptr_array
BF = _abi.TRS_BF16


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def probe(rows):
    torch.manual_seed(0)
    xs = [(torch.randn(rows, w, device=dev) * 0.5).bfloat16() for w in (2496, 512, 416)]
    gs = [torch.randn(rows, w, device=dev).bfloat16() for w in (512, 416, 416)]
    gbf = [torch.randn(512, device=dev) for _ in range(3)]
    in_f = [2496, 400, 400]
    # today: tail layers as g^T x in one launch, first layer as x^T g
    Ms, Ns, ldg, ldx = ia([400, 400]), ia([400, 400]), ia([416, 416]), ia([512, 416])
    St = int(lib.trs_wgrad_rows_many_splits(2, Ms, Ns, ldg, ldx, rows))
    Sw = int(lib.trs_wgrad_wide_splits(2496, 400, 512, rows))
    # merged: x^T g for all three
    Mx, Ng, lx, lg = ia([2496, 416, 416]), ia([400, 400, 400]), ia([2496, 512, 416]), ia([512, 416, 416])
    S = int(lib.trs_wgrad_wide_many_splits(3, Mx, lx, Ng, lg, rows))
    assert St > 0 and Sw > 0 and S > 0, (St, Sw, S)
    part_t = [torch.empty(St, 400, 400, dtype=torch.float32, device=dev) for _ in range(2)]
    part_w = torch.empty(Sw, 2496, 400, dtype=torch.float32, device=dev)
    part = [torch.empty(S, m, 400, dtype=torch.float32, device=dev) for m in (2496, 416, 416)]
    gw_old = [torch.empty(400, c, dtype=torch.bfloat16, device=dev) for c in in_f]
    gw_new = [torch.empty(400, c, dtype=torch.bfloat16, device=dev) for c in in_f]
    gb = [torch.empty(400, dtype=torch.bfloat16, device=dev) for _ in range(3)]

    def tail_product():
        _abi.call("trs_wgrad_rows_many", 2, pa(gs[1:]), ldg, pa(xs[1:]), ldx, rows, Ms, Ns, St, pa(part_t), _abi.stream_ptr())

    def tail_finish():
        F_.wgrad_finish([(part_t[k], gw_old[1 + k], gbf[1 + k], gb[1 + k], 400, 400, 400, 400) for k in range(2)], St, BF)

    def first_product():
        _abi.call("trs_wgrad_wide", _abi.ptr(xs[0]), 2496, _abi.ptr(gs[0]), 512, rows, 2496, 400, Sw, _abi.ptr(part_w),
                  _abi.stream_ptr())

    def first_finish():
        F_.wgrad_finish([(part_w, gw_old[0], gbf[0], gb[0], 400, 2496, 400, 2496)], Sw, BF, transposed=True)

    def today():
        tail_product()
        tail_finish()
        first_product()
        first_finish()

    def merged_product():
        _abi.call("trs_wgrad_wide_many", 3, pa(xs), lx, pa(gs), lg, rows, Mx, Ng, S, pa(part), _abi.stream_ptr())

    def merged_finish():
        F_.wgrad_finish([(part[k], gw_new[k], gbf[k], gb[k], 400, part[k].shape[1], 400, in_f[k]) for k in range(3)], S, BF,
                        transposed=True)

    def merged():
        merged_product()
        merged_finish()

    arms = {"today: 2 products + 2 finishes": today, "merged product + finish": merged,
            "today, tail product": tail_product, "today, tail finish": tail_finish,
            "today, first product": first_product, "today, first finish": first_finish,
            "merged, product only": merged_product, "merged, finish only": merged_finish}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(args.iters):      # interleaved rounds, one event pair per call
        for k, fn in arms.items():
            ts[k].append(once(fn))
    print(f"rows {rows}: today S = {St} (tail, per job) and {Sw} (first layer); merged S = {S}")
    for k, v in ts.items():
        print(f"  {k:34s} med {statistics.median(v):7.1f} min {min(v):7.1f} us")
    flop = 2.0 * rows * 400 * (2496 + 400 + 400)
    t = statistics.median(ts["merged, product only"])
    print(f"  merged product: {flop / 1e9:.1f} GFLOP from the shapes, {flop / t / 1e9:.3f} PFLOP/s at the median")
    for k in range(3):
        ref = gs[k][:, :400].float().t() @ xs[k][:, :in_f[k]].float()
        e_old = float((gw_old[k].float() - ref).abs().max() / ref.abs().max())
        e_new = float((gw_new[k].float() - ref).abs().max() / ref.abs().max())
        d = float((gw_new[k].float() - gw_old[k].float()).abs().max() / gw_old[k].float().abs().max())
        print(f"  layer {k}: rel err against the fp32 product today {e_old:.2e}, merged {e_new:.2e}; merged against today {d:.2e}")


for r in args.rows:
    probe(r)

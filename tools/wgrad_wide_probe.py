"""First-layer weight gradient of the deep branch (dW1^T = x^T g1, x 2496 wide, g1 400 live columns in 512-wide rows):
trs_wgrad_wide + trs_wgrad_finish_t against the library path it replaces (torch.bmm over 16 row slices of x^T g1 with the
padding columns + trs_wgrad_finish_t), stand-alone with events at 65 536 rows; then the layer's weight gradient
(layers._dense_layer_grads) with and without the kernel at smaller row counts -- the figures behind
layers.WIDE_WGRAD_MIN_ROWS.
usage (GPU box): python tools/wgrad_wide_probe.py"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from torecsys_amd import _abi, layers
from torecsys_amd import functional as F_

lib = _abi.load()
dev = torch.device("cuda:0")
torch.manual_seed(0)


def timeit(fn, iters=20, warm=3):
    """(median, min) in us, one event pair per call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


rows, M, N, ldg = 65536, 2496, 400, 512
x = (torch.randn(rows, M, device=dev) * 0.5).bfloat16()
g = torch.randn(rows, ldg, device=dev).bfloat16()
gbf = torch.randn(ldg, device=dev)
ref = g[:, :N].float().t() @ x.float()

S = int(lib.trs_wgrad_wide_splits(M, N, ldg, rows))
part = torch.empty(S, M, N, dtype=torch.float32, device=dev)
gw = torch.empty(N, M, dtype=torch.bfloat16, device=dev)
gb = torch.empty(N, dtype=torch.bfloat16, device=dev)


def kernel():
    _abi.call("trs_wgrad_wide", _abi.ptr(x), M, _abi.ptr(g), ldg, rows, M, N, S, _abi.ptr(part), _abi.stream_ptr())


def finish():
    F_.wgrad_finish([(part, gw, gbf, gb, N, M, N, M)], S, _abi.TRS_BF16, transposed=True)


kernel()
finish()
err = float((gw.float() - ref).abs().max() / ref.abs().max())
tk, tf, tb = timeit(kernel), timeit(finish), timeit(lambda: (kernel(), finish()))
print(f"trs_wgrad_wide S={S}: kernel med {tk[0]:.1f} min {tk[1]:.1f} us | finish_t med {tf[0]:.1f} min {tf[1]:.1f} | "
      f"both med {tb[0]:.1f} min {tb[1]:.1f} | rel err against the fp32 product {err:.2e}")


def library():
    p = torch.bmm(x.view(16, rows // 16, -1).transpose(1, 2), g.view(16, rows // 16, -1), out_dtype=torch.float32)
    F_.wgrad_finish([(p, gw, gbf, gb, ldg, M, N, M)], 16, _abi.TRS_BF16, transposed=True)


tl = timeit(library)
print(f"library path (bmm of 16 slices + finish_t): med {tl[0]:.1f} min {tl[1]:.1f} us")

W = torch.randn(ldg, M, device=dev).bfloat16()
layers.WIDE_WGRAD_MIN_ROWS = 0
routed = layers._wide_wgrad_splits
for r in (2688, 3072, 4096, 6144, 8192, 16384, 65536):
    xs, gs = x[:r], g[:r]
    assert routed(gs, xs, N, M)
    t1 = timeit(lambda: layers._dense_layer_grads(gs, gbf, xs, W, N, M, torch.bfloat16, False, True, True))
    layers._wide_wgrad_splits = lambda *a: 0
    t0 = timeit(lambda: layers._dense_layer_grads(gs, gbf, xs, W, N, M, torch.bfloat16, False, True, True))
    layers._wide_wgrad_splits = routed
    print(f"rows {r}: wide {t1[0]:.1f} (min {t1[1]:.1f}) us, library {t0[0]:.1f} (min {t0[1]:.1f}) us")

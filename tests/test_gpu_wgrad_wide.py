"""trs_wgrad_wide: the weight gradient of a wide-input layer, dW^T = x^T g over row slices, on the four-wave LDS-DMA
kernel of csrc/wgrad_rows.hip (x in 13-tile blocks of 208 columns, g in two blocks of 12 | 13 tiles), folded by
trs_wgrad_finish_t.

Exact sums: operands are integers of magnitude <= 2 in bf16 and rows <= 8192, so every product is an integer of at most
4, every fp32 partial and the sum of the partials is an integer below 2**24 whatever the order of summation, and the fp32
output of the finish must equal the int64 product computed on the CPU.

Two row thresholds: the C entry takes every multiple of 128 rows that gives each of its S slices one 128-row quad (the
exact-sum cases start there); the layer routes to it from layers.WIDE_WGRAD_MIN_ROWS on, the measured row count from
which it beats the library GEMM (profiles/wgrad_wide.md).  trs_wgrad_wide_splits sees no pointers: a misaligned row
stride makes it answer 0, a misaligned base pointer is refused by trs_wgrad_wide itself (and never reaches it from the
layer, which checks before it asks)."""
import copy

import pytest
import torch

import exact_ref as X
from conftest import rel_err

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
# (x columns, live g columns, g row stride): the benchmark's first layer (12 blocks; g padded to 512 columns) and an
# odd block count against an unpadded g of two 13-tile blocks
SHAPES = [(2496, 400, 512), (624, 416, 416)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _splits(M, N, ldg, rows):
    from torecsys_amd import _abi
    return int(_abi.load().trs_wgrad_wide_splits(M, N, ldg, rows))


def _slices(M, N, ldg):
    """S of a shape: the same for every row count that is taken"""
    S = _splits(M, N, ldg, 1 << 16)
    assert S > 0
    return S


def _row_counts(S):
    return [128 * S, 128 * (S + 5), 8192]


@pytest.fixture(scope="module")
def operands():
    """per shape: integer operands of 8192 rows (the row counts of a shape are prefixes of them) and the int64 products
    of every row count, computed once"""
    out = {}
    for M, N, ldg in SHAPES:
        g_ = X.gen(M, N, ldg)
        x = torch.randint(-2, 3, (8192, M), generator=g_)
        g = torch.randint(-2, 3, (8192, ldg), generator=g_)      # columns N.. hold junk that must not reach the result
        if ldg > N:
            g[:, N:] = torch.randint(1, 3, (8192, ldg - N), generator=g_)
        out[(M, N, ldg)] = (x, g, {})
    return out


def _reference(operands, shape, rows):
    x, g, memo = operands[shape]
    if rows not in memo:
        N = shape[1]
        memo[rows] = (g[:rows, :N].t().to(torch.float64) @ x[:rows].to(torch.float64)).to(torch.int64)
        assert int(memo[rows].abs().max()) < 2 ** 24
    return memo[rows]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["one_quad_per_slice", "ragged", "8192"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_wide_exact_sums(dev, operands, shape, which):
    """offset operand views (16-byte aligned, not at the start of their allocations), sentinels around the partials,
    the fp32 output of trs_wgrad_finish_t equal to the int64 product"""
    from torecsys_amd import _abi, functional as F_
    M, N, ldg = shape
    S = _slices(M, N, ldg)
    rows = _row_counts(S)[which]
    assert rows <= 8192 and rows % 128 == 0
    assert _splits(M, N, ldg, rows) == S
    x_cpu, g_cpu, _ = operands[shape]
    off_x, off_g, guard = 8 * 5, 8 * 3, 4096
    xbuf = torch.full((off_x + rows * M + 64,), 2.0, dtype=BF16, device=dev)
    gbuf = torch.full((off_g + rows * ldg + 64,), 2.0, dtype=BF16, device=dev)
    x = xbuf[off_x:off_x + rows * M].view(rows, M)
    g = gbuf[off_g:off_g + rows * ldg].view(rows, ldg)
    x.copy_(x_cpu[:rows].to(BF16))
    g.copy_(g_cpu[:rows].to(BF16))
    assert x.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and x.data_ptr() != xbuf.data_ptr()
    pbuf = torch.full((guard + S * M * N + guard,), -12345.0, dtype=torch.float32, device=dev)
    part = pbuf[guard:guard + S * M * N]
    _abi.call("trs_wgrad_wide", _abi.ptr(x), M, _abi.ptr(g), ldg, rows, M, N, S, _abi.ptr(part), _abi.stream_ptr())
    gw = torch.empty(N, M, dtype=torch.float32, device=dev)
    F_.wgrad_finish([(part, gw, None, None, N, M, N, M)], S, _abi.value_dtype_code(gw), transposed=True)
    torch.cuda.synchronize()
    assert bool((pbuf[:guard] == -12345.0).all()) and bool((pbuf[guard + S * M * N:] == -12345.0).all()), \
        "a sentinel next to the partials was overwritten"
    want = _reference(operands, shape, rows).to(torch.float32)
    m = X.mismatch(f"wgrad_wide {shape} rows={rows} S={S}", gw, want)
    assert m is None, m
    # every partial is written (no slice keeps the fill value), and is itself an integer
    p = part.view(S, M, N)
    assert not bool((p == -12345.0).all(dim=(1, 2)).any())
    assert torch.equal(p, p.round())


def test_wgrad_wide_refusals(dev):
    """shapes trs_wgrad_wide_splits does not take, and what trs_wgrad_wide itself refuses"""
    from torecsys_amd import _abi
    M, N, ldg = 2496, 400, 512
    S = _slices(M, N, ldg)
    assert _splits(M, N, ldg, 8192 + 37) == 0                 # rows not a multiple of 128
    assert _splits(M, N, ldg, 128 * S) == S
    assert _splits(M, N, ldg, 128 * (S - 1)) == 0             # fewer rows than one quad per slice
    assert _splits(M + 16, N, ldg, 8192) == 0                 # x columns not a multiple of 208
    assert _splits(208, N, ldg, 8192) == 0                    # a single block
    assert _splits(M, 416, 408, 8192) == 0                    # the second 208-column image of g would pass ldg
    assert _splits(M, 400, 392, 8192) == 0
    assert _splits(M, 512, 512, 8192) == 0                    # not two blocks of 12 | 13 tiles
    assert _splits(M, N, 516, 8192) == 0                      # rows of g not 16-byte aligned
    rows = 128 * S
    xbuf = torch.zeros(rows * M + 64, dtype=BF16, device=dev)
    gbuf = torch.zeros(rows * ldg + 64, dtype=BF16, device=dev)
    part = torch.zeros(S * M * N, dtype=torch.float32, device=dev)

    def run(x, g, rows_, S_, ldg_=ldg):
        _abi.call("trs_wgrad_wide", _abi.ptr(x), M, _abi.ptr(g), ldg_, rows_, M, N, S_, _abi.ptr(part), _abi.stream_ptr())

    run(xbuf, gbuf, rows, S)
    for S_bad in (S - 1, S + 1, 0):
        with pytest.raises(RuntimeError, match="code"):
            run(xbuf, gbuf, rows, S_bad)
    with pytest.raises(RuntimeError, match="code"):
        run(xbuf, gbuf, 128 * (S - 1), S)                     # under the threshold, whatever S says
    with pytest.raises(RuntimeError, match="aligned"):
        run(xbuf[4:], gbuf, rows, S)                          # 8 bytes off
    with pytest.raises(RuntimeError, match="aligned"):
        run(xbuf, gbuf[4:], rows, S)
    torch.cuda.synchronize()


def _smallest_layer_rows():
    """the fewest rows at which the LAYER routes its first weight gradient to the kernel: what trs_wgrad_wide_splits
    takes, but no fewer than layers.WIDE_WGRAD_MIN_ROWS, the measured row count from which the kernel is the faster path"""
    from torecsys_amd.layers import WIDE_WGRAD_MIN_ROWS
    rows = max(128 * _slices(2496, 400, 512), WIDE_WGRAD_MIN_ROWS)
    return (rows + 127) // 128 * 128


def _layer_pair(dev, rows):
    from torecsys_amd.layers import MultilayerPerceptionLayer
    torch.manual_seed(23)
    mlp = MultilayerPerceptionLayer(2496, 1, [400, 400, 400]).to(dev).bfloat16()
    ref = copy.deepcopy(mlp.model)
    x = (torch.randn(rows, 2496, device=dev) * 0.5).bfloat16()
    return mlp, ref, x


@pytest.mark.parametrize("rows,launches", [(None, 1), (8192 + 37, 0)], ids=["smallest", "8229"])
def test_mlp_first_layer_takes_the_wide_kernel(dev, rows, launches):
    """MultilayerPerceptionLayer(2496, 1, [400, 400, 400]) in bf16 against the plain nn.Linear stack: trs_wgrad_wide runs
    once at the smallest row count at which the layer takes it and not at all at a row count that is no multiple of 128"""
    from torecsys_amd import _abi
    if rows is None:
        rows = _smallest_layer_rows()
    mlp, ref, x = _layer_pair(dev, rows)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya, yb = mlp(xa).rename(None), ref(xb)
    g = torch.randn_like(yb)
    _abi.time_kernel("trs_wgrad_wide", True)
    try:
        ya.backward(g)
        assert len(_abi.kernel_times_ms("trs_wgrad_wide")) == launches
    finally:
        _abi.time_kernel("trs_wgrad_wide", False)
    yb.backward(g)
    assert rel_err(ya.detach().float().cpu(), yb.detach().float().cpu()) <= 1e-2
    assert rel_err(xa.grad.float().cpu(), xb.grad.float().cpu()) <= 1e-2
    for (n, pa), (_, pb) in zip(mlp.model.named_parameters(), ref.named_parameters()):
        assert pa.grad.shape == pb.grad.shape == pa.shape, n
        assert rel_err(pa.grad.float().cpu(), pb.grad.float().cpu()) <= 1e-2, n


def test_mlp_wide_first_layer_replays_from_a_graph(dev):
    """forward + backward captured after one eager step: both replays give the eager weight gradients"""
    rows = _smallest_layer_rows()
    mlp, _, x = _layer_pair(dev, rows)
    x.requires_grad_()
    gout = torch.randn(rows, 1, device=dev).bfloat16()
    params = list(mlp.model.parameters())

    def step():
        for p in params:
            p.grad = None
        mlp(x).rename(None).backward(gout)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                # eager: one-time attributes, workspaces
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [p.grad.clone() for p in params]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    static = [p.grad for p in params]
    for _ in range(2):
        for t in static:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for (n, _), got, want in zip(mlp.model.named_parameters(), static, eager):
            if n.endswith("weight"):
                assert torch.equal(got, want), n

"""trs_wgrad_wide_many + one trs_wgrad_finish_t: the weight gradients of a deep branch's wide first layer and of the
400 x 400 layers behind it as ONE launch of the four-wave LDS-DMA kernel (csrc/wgrad_rows.hip) and one finish
(csrc/mlp_epilogue.hip).  16 blocks of 208 x-columns per row range, 16 ranges, 256 workgroups.

Exact sums, as in test_gpu_wgrad_wide.py: operands are integers of magnitude <= 2 in bf16 and rows <= 8192, so every
product is an integer of at most 4, every fp32 partial and every sum of partials an integer below 2**24 whatever the
order, and the fp32 output of the finish must equal the int64 product computed on the CPU.

Against today's entries (trs_wgrad_wide + trs_wgrad_finish_t, trs_wgrad_rows_many + trs_wgrad_finish) on Gaussian
operands the two paths group the fp32 sum differently (16 row ranges against 21 and 32) and round it once to bf16: the
project's bound for that is 2**-7 of the largest entry."""
import ctypes

import pytest
import torch

import exact_ref as X

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TOL = 2.0 ** -7
EINVAL, ESHAPE = -1, -3
# (M_x, ldx, N_g, ldg) per job.  DEEP: the benchmark's three -- cur, h1 (416 of its 512 columns) and hidden[0] against
# g1 (512-wide rows), gz[0] and gz[1].  FOUR: a four-block job behind the first layer (a job boundary inside an XCD)
DEEP = [(2496, 2496, 400, 512), (416, 512, 400, 416), (416, 416, 400, 416)]
FOUR = [(2496, 2496, 400, 512), (832, 832, 400, 416)]
SETS = {"2496+416+416": DEEP, "2496+832": FOUR}
S16 = 16
ROWS = [128 * S16, 128 * (S16 + 5), 8192]      # one quad per range; ranges of one and two quads; 8192


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ia(v):
    return (ctypes.c_int32 * len(v))(*[int(t) for t in v])


def _pa(ts):
    return (ctypes.c_void_p * len(ts))(*[0 if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in ts])


def _splits(jobs, rows):
    from torecsys_amd import _abi
    return int(_abi.load().trs_wgrad_wide_many_splits(len(jobs), _ia([j[0] for j in jobs]), _ia([j[1] for j in jobs]),
                                                       _ia([j[2] for j in jobs]), _ia([j[3] for j in jobs]), rows))


def _product(jobs, xs, gs, rows, S, parts, rc_only=False):
    from torecsys_amd import _abi
    args = (len(jobs), _pa(xs), _ia([j[1] for j in jobs]), _pa(gs), _ia([j[3] for j in jobs]), rows,
            _ia([j[0] for j in jobs]), _ia([j[2] for j in jobs]), S, _pa(parts), _abi.stream_ptr())
    if rc_only:
        return int(_abi.load().trs_wgrad_wide_many(*args))
    _abi.call("trs_wgrad_wide_many", *args)


def _finish(jobs, parts, S, dtype, dev, gbf=None, out_rows=None, out_cols=None):
    """gw[k] (out_rows, out_cols) = sum over the ranges of part[k] (S, M_x, N_g), transposed; the whole product by default"""
    from torecsys_amd import _abi
    J = len(jobs)
    orows, ocols = out_rows or [j[2] for j in jobs], out_cols or [j[0] for j in jobs]
    gw = [torch.empty(r, c, dtype=dtype, device=dev) for r, c in zip(orows, ocols)]
    gb = [torch.empty(r, dtype=dtype, device=dev) if gbf is not None else None for r in orows]
    _abi.call("trs_wgrad_finish_t", J, _pa(parts), S, _ia([j[0] for j in jobs]), _ia([j[2] for j in jobs]), _ia(orows),
              _ia(ocols), _abi.value_dtype_code(gw[0]), _pa(gw), _pa(gbf if gbf is not None else [None] * J), _pa(gb),
              None, None, _abi.stream_ptr())
    return gw, gb


@pytest.fixture(scope="module")
def operands():
    """per job set and job: integer operands of 8192 rows (every row count is a prefix) with junk behind the live columns
    of both operands, and a memo of the int64 products per row count"""
    out = {}
    for name, jobs in SETS.items():
        per_job = []
        for k, (M, ldx, N, ldg) in enumerate(jobs):
            g_ = X.gen(41, k, M, ldx, N, ldg)
            x = torch.randint(-2, 3, (8192, ldx), generator=g_)
            g = torch.randint(-2, 3, (8192, ldg), generator=g_)
            if ldx > M:
                x[:, M:] = torch.randint(1, 3, (8192, ldx - M), generator=g_)
            if ldg > N:
                g[:, N:] = torch.randint(1, 3, (8192, ldg - N), generator=g_)
            per_job.append((x, g, {}))
        out[name] = per_job
    return out


def _reference(operands, name, k, rows):
    x, g, memo = operands[name][k]
    if rows not in memo:
        M, _, N, _ = SETS[name][k]
        memo[rows] = (g[:rows, :N].t().to(torch.float64) @ x[:rows, :M].to(torch.float64)).to(torch.int64)
        assert int(memo[rows].abs().max()) < 2 ** 24
    return memo[rows]


@pytest.mark.parametrize("rows", ROWS, ids=["one_quad_per_range", "ragged", "8192"])
@pytest.mark.parametrize("name", list(SETS))
def test_wgrad_deep_exact_sums(dev, operands, name, rows):
    """offset operand views (16-byte aligned, not at the start of their allocations), sentinels around every job's
    partials, the fp32 output of the finish equal to the int64 product of every job"""
    jobs = SETS[name]
    assert _splits(jobs, rows) == S16 and rows % 128 == 0
    xs, gs, keep, pbufs, parts = [], [], [], [], []
    guard = 4096
    for k, (M, ldx, N, ldg) in enumerate(jobs):
        x_cpu, g_cpu, _ = operands[name][k]
        off_x, off_g = 8 * (5 + k), 8 * (3 + k)
        xbuf = torch.full((off_x + rows * ldx + 64,), 2.0, dtype=BF16, device=dev)
        gbuf = torch.full((off_g + rows * ldg + 64,), 2.0, dtype=BF16, device=dev)
        x, g = xbuf[off_x:off_x + rows * ldx].view(rows, ldx), gbuf[off_g:off_g + rows * ldg].view(rows, ldg)
        x.copy_(x_cpu[:rows].to(BF16))
        g.copy_(g_cpu[:rows].to(BF16))
        assert x.data_ptr() % 16 == 0 and g.data_ptr() % 16 == 0 and x.data_ptr() != xbuf.data_ptr()
        pbuf = torch.full((guard + S16 * M * N + guard,), -12345.0, dtype=torch.float32, device=dev)
        xs.append(x), gs.append(g), keep.append((xbuf, gbuf)), pbufs.append(pbuf)
        parts.append(pbuf[guard:guard + S16 * M * N])
    _product(jobs, xs, gs, rows, S16, parts)
    gw, _ = _finish(jobs, parts, S16, torch.float32, dev)
    torch.cuda.synchronize()
    for k, (M, ldx, N, ldg) in enumerate(jobs):
        n = S16 * M * N
        assert bool((pbufs[k][:guard] == -12345.0).all()) and bool((pbufs[k][guard + n:] == -12345.0).all()), \
            f"a sentinel next to the partials of job {k} was overwritten"
        m = X.mismatch(f"wgrad_deep {name} job {k} rows={rows}", gw[k], _reference(operands, name, k, rows).to(torch.float32))
        assert m is None, m
        p = parts[k].view(S16, M, N)
        assert not bool((p == -12345.0).any()), f"job {k}: a partial was not written"
        assert torch.equal(p, p.round())


def test_wgrad_deep_against_todays_entries(dev):
    """Gaussian operands at 8192 rows, the benchmark's three jobs: every weight gradient within 2**-7 of its maximum of
    what today's two products and two finishes give, bias gradients bit-equal, and two merged runs give identical bits.
    Measured: see profiles/wgrad_deep.md."""
    from torecsys_amd import _abi
    rows, jobs = 8192, DEEP
    S = _splits(jobs, rows)
    assert S == S16
    torch.manual_seed(7)
    xs = [(torch.randn(rows, j[1], device=dev) * 0.5).to(BF16) for j in jobs]
    gs = [torch.randn(rows, j[3], device=dev).to(BF16) for j in jobs]
    gbf = [torch.randn(512, device=dev) for _ in jobs]
    orows, ocols = [400] * 3, [2496, 400, 400]
    runs = []
    for _ in range(2):
        parts = [torch.full((S, j[0], j[2]), float("nan"), dtype=torch.float32, device=dev) for j in jobs]
        _product(jobs, xs, gs, rows, S, parts)
        runs.append(_finish(jobs, parts, S, BF16, dev, gbf, orows, ocols))
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(runs[0][0][k], runs[1][0][k]) and torch.equal(runs[0][1][k], runs[1][1][k]), k
    gw, gb = runs[0]
    # today: the first layer on trs_wgrad_wide + trs_wgrad_finish_t
    S1 = int(_abi.load().trs_wgrad_wide_splits(2496, 400, 512, rows))
    assert S1 > 0
    part = torch.empty(S1, 2496, 400, dtype=torch.float32, device=dev)
    _abi.call("trs_wgrad_wide", _abi.ptr(xs[0]), 2496, _abi.ptr(gs[0]), 512, rows, 2496, 400, S1, _abi.ptr(part), _abi.stream_ptr())
    gw1 = torch.empty(400, 2496, dtype=BF16, device=dev)
    gb1 = torch.empty(400, dtype=BF16, device=dev)
    _abi.call("trs_wgrad_finish_t", 1, _pa([part]), S1, _ia([2496]), _ia([400]), _ia([400]), _ia([2496]), _abi.TRS_BF16,
              _pa([gw1]), _pa([gbf[0]]), _pa([gb1]), None, None, _abi.stream_ptr())
    # ... and the two tail layers on trs_wgrad_rows_many + one trs_wgrad_finish (g^T x)
    Ms, Ns, ldg, ldx = _ia([400, 400]), _ia([400, 400]), _ia([416, 416]), _ia([512, 416])
    S2 = int(_abi.load().trs_wgrad_rows_many_splits(2, Ms, Ns, ldg, ldx, rows))
    assert S2 > 0
    parts2 = [torch.empty(S2, 400, 400, dtype=torch.float32, device=dev) for _ in range(2)]
    _abi.call("trs_wgrad_rows_many", 2, _pa(gs[1:]), ldg, _pa(xs[1:]), ldx, rows, Ms, Ns, S2, _pa(parts2), _abi.stream_ptr())
    gw2 = [torch.empty(400, 400, dtype=BF16, device=dev) for _ in range(2)]
    gb2 = [torch.empty(400, dtype=BF16, device=dev) for _ in range(2)]
    _abi.call("trs_wgrad_finish", 2, _pa(parts2), S2, Ms, Ns, Ms, Ns, _abi.TRS_BF16, _pa(gw2), _pa(gbf[1:]), _pa(gb2),
              None, None, _abi.stream_ptr())
    torch.cuda.synchronize()
    for k, (old_w, old_b, S_old) in enumerate([(gw1, gb1, S1), (gw2[0], gb2[0], S2), (gw2[1], gb2[1], S2)]):
        diff = float((gw[k].float() - old_w.float()).abs().max()) / float(old_w.float().abs().max())
        print(f"job {k} (S {S} against {S_old}): max difference {diff:.3e} of the maximum")
        assert diff <= TOL, (k, diff)
        assert torch.equal(gb[k], old_b), k
        f32 = gs[k][:, :400].float().t() @ xs[k][:, :ocols[k]].float()
        assert float((gw[k].float() - f32).abs().max() / f32.abs().max()) <= TOL, k


@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "f32"])
def test_finish_t_many_bias_and_cast_only_jobs(dev, dtype):
    """three products of different sizes with bias gradients and three jobs without a product (1, 400 and 70 000 values:
    more than one plane of workgroups) in one launch; integer partials, so the sums are exact: gw = part.sum(0)^T cut to
    (out_rows, out_cols) and cast once, every bias and cast-only job a plain cast; nothing behind the outputs is written"""
    from torecsys_amd import _abi
    g_ = X.gen(43)
    S = 5
    shapes = [(416, 400, 400, 400), (70, 45, 33, 65), (32, 32, 32, 32)]      # (Cc, R, out_rows, out_cols)
    parts = [torch.randint(-300, 301, (S, Cc, R), generator=g_).float().to(dev) for Cc, R, _, _ in shapes]
    gbf = [(torch.randn(R, generator=g_) * 3).to(dev) for _, R, _, _ in shapes]
    casts = [(torch.randn(n, generator=g_) * 3).to(dev) for n in (1, 400, 70000)]
    gw = [torch.full((r * c + 64,), 7.0, dtype=dtype, device=dev) for _, _, r, c in shapes]
    gb = [torch.full((r + 64,), 7.0, dtype=dtype, device=dev) for _, _, r, _ in shapes]
    cout = [torch.full((c.numel() + 64,), 7.0, dtype=dtype, device=dev) for c in casts]
    n = len(casts)
    _abi.call("trs_wgrad_finish_t", 3 + n, _pa(parts + [None] * n), S, _ia([s[0] for s in shapes] + [0] * n),
              _ia([s[1] for s in shapes] + [0] * n), _ia([s[2] for s in shapes] + [0] * n),
              _ia([s[3] for s in shapes] + [c.numel() for c in casts]), _abi.value_dtype_code(gw[0]), _pa(gw + [None] * n),
              _pa(gbf + casts), _pa(gb + cout), None, None, _abi.stream_ptr())
    torch.cuda.synchronize()
    for k, (Cc, R, r, c) in enumerate(shapes):
        want = parts[k].sum(0).t()[:r, :c].contiguous().to(dtype)
        assert torch.equal(gw[k][:r * c].view(r, c), want), k
        assert torch.equal(gb[k][:r], gbf[k][:r].to(dtype)), k
        assert bool((gw[k][r * c:] == 7.0).all()) and bool((gb[k][r:] == 7.0).all()), k
    for k, c in enumerate(casts):
        assert torch.equal(cout[k][:c.numel()], c.to(dtype)), k
        assert bool((cout[k][c.numel():] == 7.0).all()), k


def test_wgrad_deep_refusals(dev):
    """what the entries return an error code for on device operands; nothing here reaches a launch"""
    from torecsys_amd import _abi
    jobs, rows = DEEP, 128 * S16
    assert _splits(jobs, rows) == S16 and _splits(jobs, rows - 128) == 0 and _splits(jobs, rows + 64) == 0
    assert _splits(jobs[:2], rows) == 0
    xbuf = torch.zeros(rows * 2496 + 64, dtype=BF16, device=dev)
    gbuf = torch.zeros(rows * 512 + 64, dtype=BF16, device=dev)
    xs, gs = [xbuf] * 3, [gbuf] * 3
    parts = [torch.full((S16, j[0], j[2]), -12345.0, dtype=torch.float32, device=dev) for j in jobs]

    def rc(jobs_=jobs, xs_=xs, gs_=gs, rows_=rows, S_=S16, parts_=parts):
        return _product(jobs_, xs_, gs_, rows_, S_, parts_, rc_only=True)

    for S_bad in (S16 - 1, S16 + 1, 0, 21):
        assert rc(S_=S_bad) == ESHAPE, S_bad
    assert rc(rows_=rows + 64) == ESHAPE and rc(rows_=rows - 128) == ESHAPE
    assert rc(jobs_=[jobs[0], (416, 512, 400, 392), jobs[2]]) == ESHAPE
    assert rc(jobs_=jobs[:2], xs_=xs[:2], gs_=gs[:2], parts_=parts[:2]) == ESHAPE
    assert rc(xs_=[xbuf[4:], xbuf, xbuf]) == ESHAPE and "aligned" in _abi.last_error()      # 8 bytes off
    assert rc(gs_=[gbuf, gbuf[4:], gbuf]) == ESHAPE and "aligned" in _abi.last_error()
    assert rc(xs_=[xbuf, 0, xbuf]) == EINVAL and rc(parts_=[parts[0], parts[1], 0]) == EINVAL
    with pytest.raises(RuntimeError, match="code"):
        _product(jobs, xs, gs, rows, S16 + 1, parts)
    torch.cuda.synchronize()
    assert all(bool((p == -12345.0).all()) for p in parts), "a refused call wrote partials"


def _stack(dev, rows):
    from torecsys_amd.layers import MultilayerPerceptionLayer
    torch.manual_seed(31)
    mlp = MultilayerPerceptionLayer(2496, 1, [400, 400, 400]).to(dev).bfloat16()
    x = (torch.randn(rows, 2496, device=dev) * 0.5).bfloat16().requires_grad_()
    gout = torch.randn(rows, 1, device=dev).bfloat16()
    return mlp, x, gout


def _grads(mlp, x, gout):
    for p in mlp.model.parameters():
        p.grad = None
    x.grad = None
    mlp(x).rename(None).backward(gout)
    torch.cuda.synchronize()
    return {n: p.grad.clone() for n, p in mlp.model.named_parameters()}, x.grad.clone()


# a finish entry as (name, batched): a batched finish carries two or more jobs, the finish of one product one
ENTRIES = ["trs_wgrad_wide_many", ("trs_wgrad_finish_t", True), "trs_wgrad_wide", ("trs_wgrad_finish_t", False),
           "trs_wgrad_rows_many", ("trs_wgrad_finish", True)]


def _counted(fn):
    """fn() and how often it called each of ENTRIES"""
    from torecsys_amd import functional as F_
    seen, call = [], F_.call

    def record(name, *a):
        seen.append((name, a[0] >= 2) if name in ("trs_wgrad_finish", "trs_wgrad_finish_t") else name)
        return call(name, *a)

    F_.call = record
    try:
        out = fn()
        return out, [seen.count(e) for e in ENTRIES]
    finally:
        F_.call = call


def _check_layer_grads(got, want, products):
    for n in want:
        if n in products:
            d = float((got[n].float() - want[n].float()).abs().max()) / float(want[n].float().abs().max())
            print(f"{n}: max difference {d:.3e} of the maximum")
            assert d <= TOL, (n, d)
        else:
            assert torch.equal(got[n], want[n]), n


@pytest.mark.parametrize("rows", [8192, None], ids=["8192", "threshold"])
def test_hybrid_stack_routed_both_ways(dev, monkeypatch, rows):
    """2496-400-400-400-1, forward + backward through _HybridMLP: the merged launch pair against today's two pairs.  At
    8192 rows the routing constant is lowered to take the merged path; at functional.DEEP_WGRAD_MIN_ROWS the stack takes
    it by itself and keeps today's launches 128 rows below.  The three weight gradients that change their grouping agree
    within 2**-7 of their maximum; the input gradient, every bias gradient and the output layer are bit-equal."""
    from torecsys_amd import functional as F_
    at_threshold = rows is None
    rows = rows or F_.DEEP_WGRAD_MIN_ROWS
    mlp, x, gout = _stack(dev, rows)
    if not at_threshold:
        monkeypatch.setattr(F_, "DEEP_WGRAD_MIN_ROWS", rows)
    (new, gx_new), counts = _counted(lambda: _grads(mlp, x, gout))
    assert counts == [1, 1, 0, 0, 0, 0], counts
    monkeypatch.setattr(F_, "DEEP_WGRAD_MIN_ROWS", 1 << 30)
    (old, gx_old), counts = _counted(lambda: _grads(mlp, x, gout))
    assert counts == [0, 0, 1, 1, 1, 1], counts
    products = [n for n, p in mlp.model.named_parameters() if p.dim() == 2 and p.shape[0] == 400]
    assert len(products) == 3
    assert torch.equal(gx_new, gx_old)
    _check_layer_grads(new, old, products)
    if at_threshold:
        monkeypatch.undo()
        mlp2, x2, gout2 = _stack(dev, rows - 128)
        _, counts = _counted(lambda: _grads(mlp2, x2, gout2))
        assert counts == [0, 0, 1, 1, 1, 1], counts


def test_hybrid_stack_merged_replays_from_a_graph(dev, monkeypatch):
    """the stack at 8192 rows on the merged path, captured with graph.GraphedStep: three replays give the eager
    gradients bit for bit (nothing is uploaded or allocated behind the capture's back)"""
    from torecsys_amd import functional as F_
    from torecsys_amd.graph import GraphedStep
    monkeypatch.setattr(F_, "DEEP_WGRAD_MIN_ROWS", 8192)
    mlp, x, gout = _stack(dev, 8192)
    x = x.detach()
    (eager, _), counts = _counted(lambda: _grads(mlp, x.clone().requires_grad_(), gout))
    assert counts[:2] == [1, 1], counts
    params = list(mlp.model.parameters())

    def fn(xi, go):
        y = mlp(xi).rename(None)
        loss = (y.float() * go.float()).sum()
        loss.backward()
        return loss.detach()

    step = GraphedStep(fn, [x, gout], params=params)
    for _ in range(3):
        for p in params:
            if p.grad is not None:
                p.grad.fill_(float("nan"))
        step.replay(0)
        torch.cuda.synchronize()
        for n, p in mlp.model.named_parameters():
            assert torch.equal(p.grad, eager[n]), n

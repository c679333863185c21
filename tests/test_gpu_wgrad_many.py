"""trs_wgrad_rows_many + one trs_wgrad_finish: the weight gradients of several dense layers over the same rows in one
launch of the eight-wave LDS-DMA kernel of csrc/wgrad_rows.hip and one finish (the 400 x 400 tail layers of the deep
branch: gz[0] (rows, 416) against h1 (rows, 512), gz[1] (rows, 416) against hidden[0] (rows, 416)).

Exact sums: operands in {-1, 0, 1} and fewer than 2**14 + 2**10 rows, so every fp32 partial and every sum of partials is an
integer below 2**24 in any grouping, and the finish must return the float64 product rounded once (exact_ref.expect).

Against the per-layer entries (Gaussian operands) the batched launch sums the same fp32 products in another grouping
and rounds once to bf16: each job within 2**-7 of its maximum, the bound the wide first layer was held to
(profiles/wgrad_wide.md); the bias gradients are casts of the same fp32 values and must be bit-equal."""
import ctypes

import pytest
import torch

import exact_ref as X

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
# (M, N, ldg, ldx): the two pairings of the deep branch, and one job whose 416 columns are all live
JOBS = [(400, 400, 416, 512), (400, 400, 416, 416), (416, 416, 416, 416)]
CASES = {"1": JOBS[:1], "2": JOBS[:2], "3": JOBS[:3], "1x416": JOBS[2:]}
MAX_ROWS = 16384 + 5 * 128
TOL = 2.0 ** -7
ESHAPE, EINVAL = -3, -1


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
    return int(_abi.load().trs_wgrad_rows_many_splits(len(jobs), _ia([j[0] for j in jobs]), _ia([j[1] for j in jobs]),
                                                       _ia([j[2] for j in jobs]), _ia([j[3] for j in jobs]), rows))


def _smallest_rows(jobs):
    """the fewest rows the query admits for these jobs (asked, not assumed)"""
    for rows in range(128, MAX_ROWS + 1, 128):
        if _splits(jobs, rows) > 0:
            return rows
    raise AssertionError(f"trs_wgrad_rows_many_splits takes no row count up to {MAX_ROWS} for {jobs}")


def _run(dev, jobs, gs, xs, rows, S, dtype, gbf=None, rc_only=False, parts=None):
    """the batched product + finish on device operands; returns (gw list, gb list, partials)"""
    from torecsys_amd import _abi
    J = len(jobs)
    Ms, Ns = _ia([j[0] for j in jobs]), _ia([j[1] for j in jobs])
    parts = parts or [torch.full((S, j[0], j[1]), -12345.0, dtype=torch.float32, device=dev) for j in jobs]
    args = (J, _pa(gs), _ia([j[2] for j in jobs]), _pa(xs), _ia([j[3] for j in jobs]), rows, Ms, Ns, S, _pa(parts),
            _abi.stream_ptr())
    if rc_only:
        return int(_abi.load().trs_wgrad_rows_many(*args))
    _abi.call("trs_wgrad_rows_many", *args)
    gw = [torch.empty(j[0], j[1], dtype=dtype, device=dev) for j in jobs]
    gb = [torch.empty(j[0], dtype=dtype, device=dev) if gbf is not None else None for j in jobs]
    _abi.call("trs_wgrad_finish", J, _pa(parts), S, Ms, Ns, Ms, Ns, _abi.value_dtype_code(gw[0]), _pa(gw),
              _pa(gbf if gbf is not None else [None] * J), _pa(gb), None, None, _abi.stream_ptr())
    torch.cuda.synchronize()
    return gw, gb, parts


@pytest.fixture(scope="module")
def operands():
    """per job shape: integer operands of MAX_ROWS rows (every row count is a prefix) with values that must not reach
    the result behind the live columns, and a memo of float64 products"""
    out = []
    for k, (M, N, ldg, ldx) in enumerate(JOBS):
        g_ = X.gen(k, M, N, ldg, ldx)
        g, x = X.ints((MAX_ROWS, ldg), g_), X.ints((MAX_ROWS, ldx), g_)
        g[:, M:] = 1.0
        x[:, N:] = 1.0
        out.append((g, x, {}))
    return out


def _reference(operands, k, rows):
    g, x, memo = operands[k]
    if rows not in memo:
        M, N = JOBS[k][:2]
        memo[rows] = g[:rows, :M].t() @ x[:rows, :N]
        X.assert_exact_domain({"g": g[:rows], "x": x[:rows]}, {"dW": memo[rows]})
    return memo[rows]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["smallest", "plus128", "ragged"])
@pytest.mark.parametrize("case", list(CASES))
def test_wgrad_many_exact_sums(dev, operands, case, which):
    """1, 2 and 3 jobs at the smallest row count the query admits, 128 rows more, and a count whose 128-row quads the
    row ranges do not divide evenly; offset operand views; bf16 result = the float64 product rounded once, and the fp32
    result the product itself"""
    jobs = CASES[case]
    ks = [JOBS.index(j) for j in jobs]
    r0 = _smallest_rows(jobs)
    if case == "2":
        assert r0 == 8192
    S = _splits(jobs, r0)
    rows = r0 + (0, 128, 5 * 128)[which]
    assert _splits(jobs, rows) == S and _splits(jobs, r0 - 128) == 0
    if which == 2:
        assert (rows // 128) % S != 0
    gs, xs, keep = [], [], []
    for n, k in enumerate(ks):
        M, N, ldg, ldx = JOBS[k]
        off = 8 * (3 + n)
        gbuf = torch.full((off + rows * ldg + 64,), 2.0, dtype=BF16, device=dev)
        xbuf = torch.full((off + rows * ldx + 64,), 2.0, dtype=BF16, device=dev)
        g, x = gbuf[off:off + rows * ldg].view(rows, ldg), xbuf[off:off + rows * ldx].view(rows, ldx)
        g.copy_(operands[k][0][:rows].to(BF16))
        x.copy_(operands[k][1][:rows].to(BF16))
        assert g.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0 and g.data_ptr() != gbuf.data_ptr()
        gs.append(g), xs.append(x), keep.append((gbuf, xbuf))
    for dtype in (BF16, torch.float32):
        gw, _, parts = _run(dev, jobs, gs, xs, rows, S, dtype)
        for n, k in enumerate(ks):
            m = X.mismatch(f"wgrad_many {case} job {n} rows={rows} S={S} {dtype}", gw[n], X.expect(_reference(operands, k, rows), dtype))
            assert m is None, m
            assert not bool((parts[n] == -12345.0).any()), "a partial was not written"


def test_wgrad_many_jobs_do_not_read_each_others_operands(dev, operands):
    """job 0 on non-zero operands beside job 1 on zeros, then the other way round: the zero job's partials and result
    are exactly zero, the other job's result is its own product"""
    jobs = JOBS[:2]
    rows = _smallest_rows(jobs)
    S = _splits(jobs, rows)
    live = [(operands[k][0][:rows].to(BF16).to(dev), operands[k][1][:rows].to(BF16).to(dev)) for k in range(2)]
    for zero in (1, 0):
        gs = [torch.zeros_like(live[k][0]) if k == zero else live[k][0] for k in range(2)]
        xs = [torch.zeros_like(live[k][1]) if k == zero else live[k][1] for k in range(2)]
        gw, _, parts = _run(dev, jobs, gs, xs, rows, S, torch.float32)
        assert not bool(parts[zero].any()) and not bool(gw[zero].any()), f"job {zero} on zeros returned non-zero sums"
        m = X.mismatch(f"job {1 - zero} beside a zero job", gw[1 - zero], X.expect(_reference(operands, 1 - zero, rows), torch.float32))
        assert m is None, m


@pytest.mark.parametrize("case,rows", [("2", None), ("3", None), ("2", 32768)], ids=["2-smallest+128", "3-smallest+128", "2-32768"])
def test_wgrad_many_against_the_per_layer_entries(dev, case, rows):
    """Gaussian operands: every job within 2**-7 of its maximum of trs_wgrad_rows + trs_wgrad_finish, bias gradients
    bit-equal.  Near the smallest row count both paths cut the same row ranges; at 32 768 rows the per-layer entry cuts 64
    and the batched one 32, so the fp32 sums are grouped differently (measured there: 2.6e-3 and 1.1e-3 of the maximum;
    0 where the ranges coincide)."""
    from torecsys_amd import _abi
    jobs = CASES[case]
    rows = rows or _smallest_rows(jobs) + 128
    S = _splits(jobs, rows)
    if rows == 32768:
        assert S == 32 and int(_abi.load().trs_wgrad_rows_splits(400, 400, rows)) == 64
    torch.manual_seed(5)
    gs = [torch.randn(rows, j[2], device=dev).to(BF16) for j in jobs]
    xs = [(torch.randn(rows, j[3], device=dev) * 0.5).to(BF16) for j in jobs]
    gbf = [torch.randn(j[2], device=dev) for j in jobs]
    gw, gb, _ = _run(dev, jobs, gs, xs, rows, S, BF16, gbf)
    for n, (M, N, ldg, ldx) in enumerate(jobs):
        S1 = int(_abi.load().trs_wgrad_rows_splits(M, N, rows))
        assert S1 > 0
        part = torch.empty(S1, M, N, dtype=torch.float32, device=dev)
        _abi.call("trs_wgrad_rows", _abi.ptr(gs[n]), ldg, _abi.ptr(xs[n]), ldx, rows, M, N, _abi.TRS_BF16, S1, _abi.ptr(part),
                  _abi.stream_ptr())
        gw1 = torch.empty(M, N, dtype=BF16, device=dev)
        gb1 = torch.empty(M, dtype=BF16, device=dev)
        _abi.call("trs_wgrad_finish", 1, _pa([part]), S1, _ia([M]), _ia([N]), _ia([M]), _ia([N]), _abi.TRS_BF16, _pa([gw1]),
                  _pa([gbf[n]]), _pa([gb1]), None, None, _abi.stream_ptr())
        torch.cuda.synchronize()
        diff = float((gw[n].float() - gw1.float()).abs().max()) / float(gw1.float().abs().max())
        print(f"job {n} ({M}x{N}, S {S} against {S1}): max difference {diff:.3e} of the maximum")
        assert diff <= TOL, (n, diff)
        assert torch.equal(gb[n], gb1), n


def test_wgrad_many_refusals(dev):
    """what the query answers 0 to and what the entry returns an error code for; nothing here reaches a launch"""
    from torecsys_amd import _abi
    jobs = JOBS[:2]
    rows = _smallest_rows(jobs)
    S = _splits(jobs, rows)
    assert S == 32
    assert _splits(jobs, rows + 37) == 0 and _splits(jobs, rows + 64) == 0      # rows % 128 != 0
    assert _splits(jobs, rows - 128) == 0                                        # too few rows for the ranges
    # a row stride under 208 columns behind the second block (its image would reach past the row)
    assert _splits([(400, 400, 392, 512), JOBS[1]], rows) == 0
    assert _splits([JOBS[0], (400, 400, 416, 392)], rows) == 0
    assert _splits([(400, 400, 420, 512), JOBS[1]], rows) == 0                   # stride not a multiple of 8
    assert _splits([JOBS[0], (8, 400, 8, 416)], rows) == 0                       # a job that is not the DMA kernel's
    assert _splits([JOBS[0]] * 9, 1 << 16) == 0                                  # more jobs than the table holds
    assert _splits([JOBS[2]] * 8, 1 << 16) > 0
    gbuf = torch.zeros(rows * 416 + 64, dtype=BF16, device=dev)
    xbuf = torch.zeros(rows * 512 + 64, dtype=BF16, device=dev)
    gs, xs = [gbuf[:rows * 416], gbuf[:rows * 416]], [xbuf[:rows * 512], xbuf[:rows * 416]]
    parts = [torch.full((S, 400, 400), -12345.0, dtype=torch.float32, device=dev) for _ in range(2)]

    def rc(jobs_=jobs, gs_=gs, xs_=xs, rows_=rows, S_=S, parts_=parts):
        return _run(dev, jobs_, gs_, xs_, rows_, S_, BF16, rc_only=True, parts=parts_)

    for S_bad in (S - 1, S + 1, 0, 8):
        assert rc(S_=S_bad) == ESHAPE, S_bad
    assert rc(rows_=rows + 64) == ESHAPE and rc(rows_=rows - 128) == ESHAPE
    assert rc(jobs_=[(400, 400, 392, 512), JOBS[1]]) == ESHAPE
    assert rc(gs_=[gbuf[4:4 + rows * 416], gs[1]]) == ESHAPE and "aligned" in _abi.last_error()      # 8 bytes off
    assert rc(xs_=[xs[0], xbuf[4:4 + rows * 416]]) == ESHAPE and "aligned" in _abi.last_error()
    assert rc(gs_=[gs[0], 0]) == EINVAL
    nine = [JOBS[1]] * 9
    assert _run(dev, nine, [gs[0]] * 9, [xs[1]] * 9, 1 << 16, 8, BF16, rc_only=True, parts=[parts[0]] * 9) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((p == -12345.0).all()) for p in parts), "a refused call wrote partials"


def _stack(dev, rows):
    from torecsys_amd.layers import MultilayerPerceptionLayer
    torch.manual_seed(29)
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


def _check_layer_grads(got, want, names_batched):
    for n in want:
        if n in names_batched:
            d = float((got[n].float() - want[n].float()).abs().max()) / float(want[n].float().abs().max())
            print(f"{n}: max difference {d:.3e} of the maximum")
            assert d <= TOL, (n, d)
        else:
            assert torch.equal(got[n], want[n]), n


def test_hybrid_stack_routes_its_tail_through_the_batched_launch(dev, monkeypatch):
    """2496-400-400-400-1 at 8192 rows, forward + backward: the routing forced to the per-layer calls against the
    batched path.  The two 400 x 400 weight gradients agree within 2**-7 of their maximum; every other gradient (input,
    biases, first and output layer) is bit-equal."""
    from torecsys_amd import _abi
    from torecsys_amd import functional as F_
    mlp, x, gout = _stack(dev, 8192)
    n_jobs, call = [], F_.call      # the job count of every trs_wgrad_finish: a batched finish carries two or more
    monkeypatch.setattr(F_, "call", lambda name, *a: (n_jobs.append(a[0]) if name == "trs_wgrad_finish" else None,
                                                      call(name, *a))[1])
    _abi.time_kernel("trs_wgrad_rows_many", True)
    _abi.time_kernel("trs_wgrad_finish", True)
    try:
        new, gx_new = _grads(mlp, x, gout)
        assert len(_abi.kernel_times_ms("trs_wgrad_rows_many")) == 1 and len(_abi.kernel_times_ms("trs_wgrad_finish")) == 1
        assert len(n_jobs) == 1 and n_jobs[0] >= 2
        monkeypatch.setattr(F_, "_wgrad_many_splits", lambda jobs: 0)
        old, gx_old = _grads(mlp, x, gout)
        assert len(_abi.kernel_times_ms("trs_wgrad_rows_many")) == 0
    finally:
        _abi.time_kernel("trs_wgrad_rows_many", False)
        _abi.time_kernel("trs_wgrad_finish", False)
    batched = [n for n, p in mlp.model.named_parameters() if tuple(p.shape) == (400, 400)]
    assert len(batched) == 2
    assert torch.equal(gx_new, gx_old)
    _check_layer_grads(new, old, batched)


def test_hybrid_stack_batched_tail_replays_from_a_graph(dev):
    """the same stack captured with graph.GraphedStep: three replays give the eager gradients (nothing is uploaded or
    allocated behind the capture's back)"""
    from torecsys_amd.graph import GraphedStep
    mlp, x, gout = _stack(dev, 8192)
    x = x.detach()
    eager, _ = _grads(mlp, x.clone().requires_grad_(), gout)
    params = list(mlp.model.parameters())

    def fn(xi, go):
        y = mlp(xi).rename(None)
        loss = (y.float() * go.float()).sum()
        loss.backward()
        return loss.detach()

    step = GraphedStep(fn, [x, gout], params=params)
    batched = [n for n, p in mlp.model.named_parameters() if tuple(p.shape) == (400, 400)]
    for _ in range(3):
        for p in params:
            if p.grad is not None:
                p.grad.fill_(float("nan"))
        step.replay(0)
        torch.cuda.synchronize()
        _check_layer_grads({n: p.grad for n, p in mlp.model.named_parameters()}, eager, batched)

"""trs_wgrad_finish / trs_wgrad_finish_t on every route, bit for bit (csrc/mlp_epilogue.hip): the plain kernel, the
few-rows kernel, the transposed tiles, the bias cast on a vector and on partial rows, batches, jobs without a product.

Exact sums: partial products and fp32 bias sources are integers in [-4, 4], at most 256 of them meet in one value, so every
sum is an integer below 2**24 in any order and fp32 holds it exactly.  The reference is computed on the CPU in float64,
cut to the un-padded corner and cast once; the comparison is torch.equal.  Every partial is larger than the corner it
gives (R > out_rows, Cc > out_cols) with non-zero values in the padding, every partial-row source has a stride larger
than its column count, and every output lies inside a larger buffer of -0.5 -- no integer sum equals it, so an element
that was not written shows as well as one written next to the output."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = -0.5
DTYPES = [torch.bfloat16, torch.float32]
EINVAL, ESHAPE = "code -1", "code -3"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ints(g, shape):
    return torch.randint(-4, 5, shape, generator=g).float()


def _source(g, kind, n):
    """an fp32 source of n values: None, "vec" (a vector with three more entries behind it) or (nparts, extra) -- a buffer
    of nparts partial rows n + extra floats apart"""
    if kind is None:
        return None
    return _ints(g, (n + 3,)) if kind == "vec" else _ints(g, (kind[0], n + kind[1]))


def _product(g, S, out_rows, out_cols, transposed, bias="vec", pad=(1, 2)):
    R, Cc = out_rows + pad[0], out_cols + pad[1]
    return dict(part=_ints(g, (S, Cc, R) if transposed else (S, R, Cc)), R=R, Cc=Cc, out_rows=out_rows, out_cols=out_cols,
                src=_source(g, bias, out_rows))


def _cast(g, out_cols, kind="vec"):
    return dict(part=None, R=0, Cc=0, out_rows=0, out_cols=out_cols, src=_source(g, kind, out_cols))


def _guarded(dev, n, dtype):
    return torch.full((GUARD + n + GUARD,), FILL, dtype=dtype, device=dev)


def _launch(dev, jobs, S, dtype, transposed):
    """the device buffers of every job and the call; returns [(gw buffer or None, gb buffer or None)]"""
    from torecsys_amd import _abi, functional as F_
    bufs, tuples = [], []
    for j in jobs:
        n_b = j["out_rows"] if j["part"] is not None else j["out_cols"]
        gw = _guarded(dev, j["out_rows"] * j["out_cols"], dtype) if j["part"] is not None else None
        gb = _guarded(dev, n_b, dtype) if j["src"] is not None else None
        src = j["src"].to(dev) if j["src"] is not None else None
        if src is not None and src.dim() == 2:
            src = src[:, :n_b]      # partial rows: the row stride stays the buffer's
            assert src.stride(0) > n_b
        tuples.append((j["part"].to(dev) if j["part"] is not None else None, gw[GUARD:] if gw is not None else None, src,
                       gb[GUARD:] if gb is not None else None, j["R"], j["Cc"], j["out_rows"], j["out_cols"]))
        bufs.append((gw, gb))
    F_.wgrad_finish(tuples, S, _abi.value_dtype_code(torch.empty(0, dtype=dtype)), transposed=transposed)
    torch.cuda.synchronize()
    return bufs


def _expect(buf, want, what):
    got = buf.cpu()
    n = want.numel()
    assert bool((got[:GUARD] == FILL).all()) and bool((got[GUARD + n:] == FILL).all()), f"{what}: written outside the output"
    assert torch.equal(got[GUARD:GUARD + n], want.reshape(-1)), f"{what}: not the exact sum"


def _check(dev, jobs, S, dtype, transposed, what):
    bufs = _launch(dev, jobs, S, dtype, transposed)
    for k, (j, (gw, gb)) in enumerate(zip(jobs, bufs)):
        tag = f"{what}, job {k} of {len(jobs)}, {dtype}"
        n_b = j["out_rows"] if j["part"] is not None else j["out_cols"]
        if j["part"] is not None:
            full = j["part"].double().sum(0)
            full = full.t() if transposed else full
            _expect(gw, full[:j["out_rows"], :j["out_cols"]].to(dtype), tag + " (gw)")
        if j["src"] is not None:
            src = j["src"].double()
            _expect(gb, (src.sum(0) if src.dim() == 2 else src)[:n_b].to(dtype), tag + " (gb)")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_plain_route_one_job(dev, dtype):
    """one thread per column, 256 columns per workgroup, the slices four at a time and their tail; with a vector as the
    bias source the job runs on the kernel with loose arguments, with partial rows on the table kernel"""
    for out_cols in (1, 255, 256, 257):
        for out_rows in (1, 2):
            for S in (1, 3, 4, 5, 9):
                for bias in ("vec", (17, 5)):
                    g = _gen(1, out_cols, out_rows, S)
                    _check(dev, [_product(g, S, out_rows, out_cols, False, bias=bias)], S, dtype, False,
                           f"{out_rows}x{out_cols} S={S}, {bias}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_few_rows_route_one_job(dev, dtype):
    """S >= 64 and ceil(out_cols / 256) * out_rows < 64: sixteen threads per column, sixteen columns per workgroup; S = 63
    and 64 rows of one workgroup stay on the plain kernel"""
    for S in (63, 64, 65, 127, 128, 129):
        for out_cols in (1, 15, 16, 17):
            for out_rows in (1, 3):
                g = _gen(2, out_cols, out_rows, S)
                _check(dev, [_product(g, S, out_rows, out_cols, False)], S, dtype, False, f"{out_rows}x{out_cols} S={S}")
    for out_rows in (63, 64):
        _check(dev, [_product(_gen(2, out_rows), 64, out_rows, 5, False)], 64, dtype, False, f"{out_rows}x5 S=64")
    # without a bias, and a bias on partial rows (that job is the plain kernel's)
    _check(dev, [_product(_gen(2, 0), 64, 3, 17, False, bias=None)], 64, dtype, False, "3x17 S=64, no bias")
    _check(dev, [_product(_gen(2, 1), 64, 3, 17, False, bias=(17, 5))], 64, dtype, False, "3x17 S=64, partial rows")


@pytest.mark.parametrize("dtype", DTYPES)
def test_transposed_one_job(dev, dtype):
    """32 x 32 tiles through LDS, the slices two at a time and their tail; bias sources as in the plain route"""
    for out_rows in (1, 31, 32, 33):
        for out_cols in (1, 31, 32, 33):
            for S in (1, 2, 3):
                for bias in ("vec", (17, 5)):
                    g = _gen(3, out_cols, out_rows, S)
                    _check(dev, [_product(g, S, out_rows, out_cols, True, bias=bias)], S, dtype, True,
                           f"{out_rows}x{out_cols} S={S}, {bias}")


@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_ride(dev, dtype, transposed):
    """the bias cast of a product job from a vector and from partial rows (sixteen running sums, then sixteen onto one)"""
    for kind in ["vec"] + [(nparts, 5) for nparts in (1, 15, 16, 17, 33, 256)]:
        _check(dev, [_product(_gen(4, str(kind)), 2, 33, 40, transposed, bias=kind)], 2, dtype, transposed, f"33x40, {kind}")
    # more rows than one 256-wide (32-wide) workgroup of the bias row holds
    for kind in ("vec", (17, 7)):
        _check(dev, [_product(_gen(4, str(kind), 1), 1, 300, 257, transposed, bias=kind)], 1, dtype, transposed,
               f"300x257, {kind}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_row_limit(dev, dtype):
    """trs_wgrad_finish: out_rows = 256 * ceil(out_cols / 256) is the last count whose bias cast rides; one more is
    TRS_ESHAPE and nothing is written.  trs_wgrad_finish_t has no such limit."""
    for out_cols in (1, 257):
        limit = (out_cols + 255) // 256 * 256
        _check(dev, [_product(_gen(5, out_cols), 2, limit, out_cols, False)], 2, dtype, False, f"{limit}x{out_cols}")
        job = _product(_gen(5, out_cols, 1), 2, limit + 1, out_cols, False)
        with pytest.raises(RuntimeError, match=ESHAPE):
            _launch_untouched(dev, job, 2, dtype)
    _check(dev, [_product(_gen(5, 2), 2, 257, 1, True)], 2, dtype, True, "257x1 transposed")


def _launch_untouched(dev, job, S, dtype):
    """a call that must be refused: raises what the call raises after checking that no output was written"""
    from torecsys_amd import _abi, functional as F_
    gw = _guarded(dev, job["out_rows"] * job["out_cols"], dtype)
    gb = _guarded(dev, job["out_rows"], dtype)
    try:
        F_.wgrad_finish([(job["part"].to(dev), gw[GUARD:], job["src"].to(dev), gb[GUARD:], job["R"], job["Cc"],
                          job["out_rows"], job["out_cols"])], S, _abi.value_dtype_code(gw))
    finally:
        torch.cuda.synchronize()
        assert bool((gw == FILL).all()) and bool((gb == FILL).all()), "a refused call wrote an output"


# (out_rows, out_cols) of a batch's jobs: unequal, the largest neither first nor last
SIZES = [(3, 5), (40, 300), (1, 1), (17, 33), (2, 257), (33, 31), (5, 16), (64, 2)]
BIAS = ["vec", (17, 5), None, (33, 9), "vec", (1, 1), None, (256, 3)]


@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_batches_of_unequal_jobs(dev, dtype, n, transposed):
    """the grid is sized by the largest job: the surplus workgroups of the smaller ones write nothing"""
    g = _gen(6, n, transposed)
    jobs = [_product(g, 3, r, c, transposed, bias=b, pad=(1 + k, 2 + k)) for k, ((r, c), b) in enumerate(zip(SIZES[:n], BIAS))]
    _check(dev, jobs, 3, dtype, transposed, f"batch of {n}")


@pytest.mark.parametrize("transposed", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_jobs_without_a_product(dev, dtype, transposed):
    """a cast alone and beside a product job, from a vector and from partial rows; 1000 columns on partial rows need 63
    workgroups of sixteen columns, more than the plane of an 8 x 8 product has: the entry grows it"""
    casts = [(c, "vec") for c in (1, 256, 257)] + [(c, (17, 5)) for c in (1, 16, 17)]
    for cols, kind in casts:
        g = _gen(7, cols, str(kind))
        _check(dev, [_cast(g, cols, kind)], 1, dtype, transposed, f"cast of {cols} alone, {kind}")
        _check(dev, [_cast(g, cols, kind), _product(g, 2, 8, 8, transposed)], 2, dtype, transposed, f"cast of {cols} first, {kind}")
    g = _gen(7, 1000)
    _check(dev, [_product(g, 2, 8, 8, transposed), _cast(g, 1000, (33, 24))], 2, dtype, transposed, "cast of 1000 behind 8x8")
    _check(dev, [_product(g, 2, 8, 8, transposed)] + [_cast(g, c, k) for c, k in casts], 2, dtype, transposed, "six casts")


def test_argument_checks(dev):
    """refused before anything is launched: 0 and 9 jobs, gb_nparts without gb_stride (and the reverse)"""
    from torecsys_amd import _abi, functional as F_
    job = _product(_gen(8), 2, 8, 8, False)
    with pytest.raises(RuntimeError, match=EINVAL):
        F_.wgrad_finish([], 2, _abi.TRS_F32)
    for transposed in (False, True):
        part, src = job["part"].to(dev), job["src"].to(dev)
        gw, gb = _guarded(dev, 64, torch.float32), _guarded(dev, 8, torch.float32)
        one = (part, gw[GUARD:], src, gb[GUARD:], job["R"], job["Cc"], 8, 8)
        with pytest.raises(RuntimeError, match=EINVAL):
            F_.wgrad_finish([], 2, _abi.TRS_F32, transposed=transposed)
        with pytest.raises(RuntimeError, match=EINVAL):
            F_.wgrad_finish([one] * 9, 2, _abi.TRS_F32, transposed=transposed)
        entry = getattr(_abi.load(), "trs_wgrad_finish_t" if transposed else "trs_wgrad_finish")
        pa, ia = F_._ptr_array, F_._i32_array
        args = (1, pa([part]), 2, ia([9]), ia([10]), ia([8]), ia([8]), _abi.TRS_F32, pa([gw[GUARD:]]), pa([src]), pa([gb[GUARD:]]))
        assert int(entry(*args, ia([0]), None, _abi.stream_ptr())) == -1
        assert int(entry(*args, None, ia([0]), _abi.stream_ptr())) == -1
        torch.cuda.synchronize()
        assert bool((gw == FILL).all()) and bool((gb == FILL).all()), "a refused call wrote an output"
        assert int(entry(*args, None, None, _abi.stream_ptr())) == 0      # the same arguments without either array
        torch.cuda.synchronize()
        assert not bool((gw[GUARD:GUARD + 64] == FILL).any())

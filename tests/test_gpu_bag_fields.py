"""GPU tests of functional.bag_pool_fields and RaggedMultiListIndicesEmbedding (csrc/bag_fields.hip:
trs_bag_pool_fields_fwd, trs_bag_owner_fields; the gradients are trs_scatter_rows_ragged / trs_bag_weight_grad_ragged of
csrc/bag.hip on the map the owner kernel writes).  Reference: tests/bag_fields_ref.py, the fp64 restatement that
tests/test_bag_fields_host.py pins to F.embedding_bag per field.

Every case: F = 3 fields of sizes (7, 1, 50) -- a one-row field in the middle -- and B = 13, so f = j / B is no shift.  Each
field holds the 13 fixed lengths of bag_ragged_ref.boundary_lengths(g, T), T = bag_ragged_long_len() read from the library,
rotated by field: [0, 1, 3, 4, 5, 7, 8, 9, T-1, T, T+1, 2T+3, 0] -- an empty bag, both sides of the walks' 4 and 8 rows in
flight, both sides of T; a few ids sit behind the last offset.

Exact tests.  fp32 ("wide"): integer table entries in [-4, 4], weights in {0.5, 1, 2}, output-gradient entries in [-2, 2],
n < 2^12: every sum is a multiple of 2^-11 below 2^13 (the argument of tests/test_gpu_bag_ragged.py), 24 bits, so fp32 holds
the fp64 result itself.  bf16 ("narrow") holds 8 bits, so the lengths are cut to powers of two for every mode (2T+3 -> 2T is
still a bag of the second tier), a bag of more than 8 ids holds one id and one weight throughout, table entries lie in
[-2, 2] and gradient entries in [-1, 1], and for the (weighted) sum the gradient of such a bag is divided by its length: a
pooled row is then (a power of two) x (a small integer) or a sum of at most 8 small terms, a table-gradient row a sum of
small integers or halves below 128, the mean's terms eighths below 32.  Each case asserts on the CPU that its expected
output and gradients pass through the dtype unchanged, then compares with torch.equal."""
import functools

import pytest
import torch

from bag_fields_ref import (cut_pow2, field_major_lengths, field_starts, fields_bag, one_id_long_bags, values_for)
from bag_ragged_ref import boundary_lengths
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL32 = 1e-5      # tests/test_gpu_bag_ragged.py
TOLBF = 1e-2
SIZES = (7, 1, 50)
NF, B, TRAIL = 3, 13, 5
V = sum(SIZES)
MODES = (("sum", False), ("mean", False), ("max", False), ("sum", True))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _T():
    from torecsys_amd import functional as F_
    return F_.bag_ragged_long_len()


def _bags(g):
    """offsets (F*B + 1,) and values with TRAIL ids behind the last offset: every field holds the 13 boundary lengths"""
    T = _T()
    per_field = []
    for f in range(NF):
        ls = boundary_lengths(g, T, B=B)
        assert len(ls) == B and 0 in ls and 2 * T + 3 in ls and T in ls and T + 1 in ls
        per_field.append(ls[4 * f:] + ls[:4 * f])
    offsets = field_major_lengths(per_field)
    return values_for(g, offsets, SIZES, TRAIL), offsets


def _run(dev, dtype, vt, ot, w, values, offsets, mode, psw, gout, table_grad=True):
    """one forward + backward on the device; returns (out (B,F,E), table grad, dw), all on the CPU"""
    from torecsys_amd import functional as F_
    wd = w.to(dtype).to(dev).requires_grad_(table_grad)
    pd = psw.to(dtype).to(dev).requires_grad_() if psw is not None else None
    y = F_.bag_pool_fields(wd, values.to(dev).to(vt), offsets.to(dev).to(ot), field_starts(SIZES).to(dev), mode,
                           per_sample_weights=pd)
    nb = (offsets.numel() - 1) // NF
    assert tuple(y.shape) == (nb, NF, w.shape[1]) and y.dtype == dtype and y.is_contiguous()
    if table_grad or pd is not None:
        y.backward(gout.to(dtype).to(dev))
    return (y.detach().cpu(), wd.grad.cpu() if wd.grad is not None else None,
            pd.grad.cpu() if pd is not None and pd.grad is not None else None)


# ------------------------------------------------------------------------------------------------ 1. exact, every path
@functools.lru_cache(maxsize=None)
def _exact_case(E, narrow):
    """[(mode, weighted, values, offsets, psw, gout, (out, grad, dw))] in fp64, built once per (E, operand kind)"""
    T = _T()
    g = torch.Generator().manual_seed(2000 + E + (11 if narrow else 0))
    values, offsets = _bags(g)
    cut_v, cut_o = cut_pow2(values, offsets)
    if narrow:
        values, offsets = one_id_long_bags(g, cut_v, cut_o, SIZES), cut_o
        cut_v = values
    n = values.numel()
    assert n < 2 ** 12 and n == int(offsets[-1]) + TRAIL
    lo, glim = (2, 1) if narrow else (4, 2)
    w = torch.randint(-lo, lo + 1, (V, E), generator=g).double()
    psw = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=g)]
    gout = torch.randint(-glim, glim + 1, (B, NF, E), generator=g).double()
    g_sum = gout.clone()
    if narrow:
        for j in range(NF * B):
            beg, end = int(offsets[j]), int(offsets[j + 1])
            if end - beg > 8:
                psw[beg:end] = psw[beg]
                g_sum[j % B, j // B] /= end - beg                              # a power of two
    cases = []
    for mode, weighted in MODES:
        v, o = (cut_v, cut_o) if mode == "mean" else (values, offsets)
        lens = (o[1:] - o[:-1]).reshape(NF, B)
        assert bool((lens == 0).any(dim=1).all()) and bool((lens > T).any(dim=1).all())
        p = psw[:v.numel()] if weighted else None
        go = g_sum if mode == "sum" else gout
        cases.append((mode, weighted, v, o, p, go, fields_bag(w, v, o, SIZES, mode, p, go)))
    return w, cases


@pytest.mark.parametrize("vt,ot", [(torch.int64, torch.int32), (torch.int32, torch.int64)])
@pytest.mark.parametrize("dtype,E", [(torch.bfloat16, 8), (torch.float32, 32), (torch.bfloat16, 512), (torch.float32, 5)])
def test_exact_integer_operands(dev, dtype, E, vt, ot):
    """One lane per bag (bf16 E = 8), 8 lanes (fp32 E = 32), 64 lanes (bf16 E = 512) and the any-E path (fp32 E = 5), pairs
    of WIDTHS in tests/test_gpu_bag_ragged.py: sum / mean / max / weighted sum; values and offsets of different index
    types.  Out, the dense table gradient and dw equal the fp64 result, which the dtype holds exactly."""
    w, cases = _exact_case(E, dtype == torch.bfloat16)
    for mode, weighted, values, offsets, psw, gout, (want_y, want_g, want_dw) in cases:
        tag = (mode, weighted)
        for t in (w, gout, psw, want_y, want_g, want_dw):                      # no rounding anywhere: nothing passes by luck
            assert t is None or torch.equal(t.to(dtype).double(), t), tag
        y, grad, dw = _run(dev, dtype, vt, ot, w, values, offsets, mode, psw, gout)
        assert torch.equal(y.double(), want_y), tag
        assert torch.equal(grad.double(), want_g), tag
        empty = ((offsets[1:] - offsets[:-1]) == 0).reshape(NF, B).t()
        assert float(y[empty].abs().max()) == 0.0, tag                        # empty bags: exactly zero rows
        if weighted:
            assert torch.equal(dw.double(), want_dw), tag
            assert float(dw[int(offsets[-1]):].abs().max()) == 0.0, tag       # ids that no bag holds


# ------------------------------------------------------------------------------------------------ 2. real values
@functools.lru_cache(maxsize=None)
def _real_batch(E):
    g = torch.Generator().manual_seed(700 + E)
    values, offsets = _bags(g)
    w = torch.randn(V, E, generator=g)
    psw = torch.rand(values.numel(), generator=g) * 2
    gout = torch.randn(B, NF, E, generator=g)
    return values, offsets, w, psw, gout


def _fields_fwd_raw(dev, wd, values, offsets, mode):
    """the C entry itself: (out (B*F, E), argmax (B*F, E))"""
    from torecsys_amd._abi import call, index_dtype_code, ptr, size_query, stream_ptr, value_dtype_code
    E = wd.shape[1]
    fb = offsets.numel() - 1
    out = torch.empty(fb, E, dtype=wd.dtype, device=dev)
    amax = torch.empty(fb, E, dtype=torch.int32, device=dev)
    inv = torch.empty(fb, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = size_query("trs_bag_fields_workspace_bytes", fb)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    fo = field_starts(SIZES).to(dev)
    call("trs_bag_pool_fields_fwd", ptr(wd), V, E, value_dtype_code(wd), ptr(values), index_dtype_code(values),
         values.numel(), ptr(offsets), index_dtype_code(offsets), offsets.numel(), fb // NF, NF, ptr(fo), mode, None,
         ptr(out), ptr(amax), ptr(inv), ptr(ws), nbytes, ptr(flag), stream_ptr())
    torch.cuda.synchronize()
    return out, amax


def _ragged_fwd_raw(dev, wd, ids, offsets, mode):
    from torecsys_amd._abi import call, index_dtype_code, ptr, size_query, stream_ptr, value_dtype_code
    rows, E = wd.shape
    nb = offsets.numel() - 1
    out = torch.empty(nb, E, dtype=wd.dtype, device=dev)
    amax = torch.empty(nb, E, dtype=torch.int32, device=dev)
    inv = torch.empty(nb, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = size_query("trs_bag_ragged_workspace_bytes", nb)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("trs_bag_pool_ragged_fwd", ptr(wd), rows, E, value_dtype_code(wd), ptr(ids), index_dtype_code(ids), ids.numel(),
         ptr(offsets), index_dtype_code(offsets), offsets.numel(), nb, mode, -1, None, ptr(out), ptr(amax), ptr(inv),
         ptr(ws), nbytes, ptr(flag), stream_ptr())
    torch.cuda.synchronize()
    return out, amax


@pytest.mark.parametrize("E", [64, 12])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_forward_bit_equal_to_single_field_calls(dev, dtype, E):
    """Real values: the forward is F calls of bag_pool_ragged on the field's table slice, id slice and rebased offsets, bit
    for bit (the same walk, the same order), the max positions included once rebased; the gradients against fp64 within
    the bounds of tests/test_gpu_bag_ragged.py."""
    from torecsys_amd import functional as F_
    values, offsets, w, psw, gout = _real_batch(E)
    w, psw, gout = (t.to(dtype) for t in (w, psw, gout))
    fo = field_starts(SIZES)
    wd, vd, od = w.to(dev), values.to(dev), offsets.to(dev)
    tol = TOL32 if dtype == torch.float32 else TOLBF
    for mode, weighted in MODES:
        tag = (mode, weighted)
        p = psw if weighted else None
        y, grad, dw = _run(dev, dtype, torch.int64, torch.int64, w, values, offsets, mode, p, gout)
        with torch.no_grad():
            for f in range(NF):
                off = od[f * B:(f + 1) * B + 1]
                beg, end = int(offsets[f * B]), int(offsets[(f + 1) * B])
                z = F_.bag_pool_ragged(wd[int(fo[f]):int(fo[f + 1])], vd[beg:end], off - beg, mode,
                                       per_sample_weights=None if p is None else p.to(dev)[beg:end],
                                       include_last_offset=True)
                assert torch.equal(y[:, f], z.squeeze(1).cpu()), (tag, f)
        want_y, want_g, want_dw = fields_bag(w.double(), values, offsets, SIZES, mode,
                                             None if p is None else p.double(), gout.double())
        assert rel_err(grad, want_g) <= tol, tag
        if weighted:
            assert rel_err(dw, want_dw) <= tol, tag
    # the max positions: flat positions of the whole values vector = the field's own positions + the field's first one
    _, amax = _fields_fwd_raw(dev, wd, vd, od, 2)
    amax = amax.view(B, NF, E)
    for f in range(NF):
        beg, end = int(offsets[f * B]), int(offsets[(f + 1) * B])
        _, am_f = _ragged_fwd_raw(dev, wd[int(fo[f]):int(fo[f + 1])].contiguous(), vd[beg:end].contiguous(),
                                  (od[f * B:(f + 1) * B + 1] - beg).contiguous(), 2)
        assert torch.equal(amax[:, f], torch.where(am_f >= 0, am_f + beg, am_f)), f
        assert int((am_f < 0).sum()) > 0                                      # the empty bags: -1 on both sides


@pytest.mark.parametrize("E", [64, 12])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_same_call_twice_is_bit_identical(dev, dtype, E):
    """forward and backward, real values, bags on both sides of T: the same tensors twice give the same bits"""
    from torecsys_amd import functional as F_
    values, offsets, w, psw, gout = _real_batch(E)
    vd, od, gd, fo = values.to(dev), offsets.to(dev), gout.to(dtype).to(dev), field_starts(SIZES).to(dev)

    def run(mode, p):
        wd = w.to(dtype).to(dev).requires_grad_()
        pd = p.to(dtype).to(dev).requires_grad_() if p is not None else None
        y = F_.bag_pool_fields(wd, vd, od, fo, mode, per_sample_weights=pd)
        y.backward(gd)
        return {"out": y.detach(), "grad": wd.grad, "dw": None if pd is None else pd.grad}

    for mode, weighted in MODES:
        a, b = run(mode, psw if weighted else None), run(mode, psw if weighted else None)
        for k in a:
            assert a[k] is None or torch.equal(a[k], b[k]), (mode, weighted, k)


# ------------------------------------------------------------------------------------------------ 3. range checks
@pytest.mark.parametrize("E", [16, 5])
def test_an_id_is_checked_against_its_own_field(dev, E):
    """an id equal to field_sizes[0] in a bag of field 0 would be row 0 of field 1, which holds a sentinel: the bag pools a
    zero row in its place (the mean still counts it), the index flag is raised, and the sentinel row's gradient is that of
    its own lookups alone"""
    from torecsys_amd import functional as F_
    g = torch.Generator().manual_seed(31)
    values, offsets = _bags(g)
    j = 3                                                                     # field 0, a bag of 4 ids
    beg, end = int(offsets[j]), int(offsets[j + 1])
    assert j < B and end - beg == 4
    values = values.clone()
    values[beg + 1] = SIZES[0]
    w = torch.randint(-4, 5, (V, E), generator=g).double()
    w[SIZES[0]] = 1000.0                                                      # the neighbour's row 0
    gout = torch.randint(1, 3, (B, NF, E), generator=g).double()
    clean = values.clone()
    clean[beg + 1] = 0
    F_.index_errors_seen()
    for mode in ("sum", "mean", "max"):
        want_y, want_g, _ = fields_bag(w, values, offsets, SIZES, mode, None, gout)
        assert float(want_y[j, 0].abs().max()) < 100                          # the reference did not read the sentinel
        y, grad, _ = _run(dev, torch.float32, torch.int64, torch.int64, w, clean, offsets, mode, None, gout)
        assert not F_.index_errors_seen(), mode                               # ids inside their fields, ids behind the bags
        y, grad, _ = _run(dev, torch.float32, torch.int64, torch.int64, w, values, offsets, mode, None, gout)
        assert F_.index_errors_seen(), mode
        assert rel_err(y, want_y) <= TOL32 and float(y[j, 0].abs().max()) < 100, mode
        assert rel_err(grad, want_g) <= TOL32, mode
        own = fields_bag(w, clean, offsets, SIZES, mode, None, gout)[1][SIZES[0]]
        assert torch.allclose(grad[SIZES[0]].double(), own, rtol=TOL32, atol=0), mode      # nothing from the planted id
    # a negative id, and the one-row field's only valid id is 0
    values[beg + 2] = -1
    values[int(offsets[B + 10])] = 1                                          # field 1, bag 10 (one id)
    assert int(offsets[B + 11] - offsets[B + 10]) == 1
    want_y, want_g, _ = fields_bag(w, values, offsets, SIZES, "sum", None, gout)
    y, grad, _ = _run(dev, torch.float32, torch.int32, torch.int32, w, values, offsets, "sum", None, gout)
    assert F_.index_errors_seen()
    assert rel_err(y, want_y) <= TOL32 and rel_err(grad, want_g) <= TOL32
    assert float(y[10, 1].abs().max()) == 0.0


@pytest.mark.parametrize("ot", [torch.int64, torch.int32])
@pytest.mark.parametrize("E", [16, 5])
def test_bad_offsets_are_clamped_and_flagged(dev, E, ot):
    """A decreasing pair, an offset above n and a negative one: clamped to [0, n] and flagged; a bag whose end lies before
    its begin and a bag that begins behind n are empty, every bag whose own pair is untouched is bit-equal to the clean
    run.  The backward: the map gives every position one owner (the forward's clamped ranges may overlap after a decreasing
    pair), so with mode sum and a gradient of ones -- where a table-gradient entry is a COUNT of lookups -- every entry
    lies in [0, reference], the reference counting every lookup of every clamped bag: nothing lands outside it."""
    from torecsys_amd import functional as F_
    g = torch.Generator().manual_seed(17)
    nb = 4
    lens = [[3, 0, 4, 2], [1, 1, 0, 2], [5, 2, 3, 1]]
    good = field_major_lengths(lens)
    values = values_for(g, good, SIZES, 3)
    n = values.numel()
    assert n == int(good[-1]) + 3 == 27
    bad = good.clone()
    bad[2] = 1                      # bags 1 and 2 of field 0: (3, 1) is empty, (1, 7) overlaps bag 0
    bad[6] = -3                     # bag 1 of field 1 ends, bag 2 begins, below 0: (10, 0) empty, (0, 11) overlaps
    bad[-1] = n + 9                 # the last bag's end lies above n: clamped to n, it takes in the trailing ids
    touched = {1, 2, 5, 6, 11}
    w = torch.randint(-4, 5, (V, E), generator=g).double()
    ones = torch.ones(nb, NF, E, dtype=torch.float64)
    fo = field_starts(SIZES).to(dev)
    F_.index_errors_seen()
    for mode in ("sum", "mean", "max"):
        y0, _, _ = _run(dev, torch.float32, torch.int64, ot, w, values, good, mode, None, ones)
        assert not F_.index_errors_seen(), mode
        y1, grad, _ = _run(dev, torch.float32, torch.int64, ot, w, values, bad, mode, None, ones)
        assert F_.index_errors_seen(), mode
        want_y, want_g, _ = fields_bag(w, values, bad, SIZES, mode, None, ones)
        assert rel_err(y1, want_y) <= TOL32, mode
        assert float(y1[1, 0].abs().max()) == 0.0 and float(y1[1, 1].abs().max()) == 0.0, mode      # bags 1 and 5: empty
        for j in range(NF * nb):
            if j not in touched:
                assert torch.equal(y1[j % nb, j // nb], y0[j % nb, j // nb]), (mode, j)
        assert bool(torch.isfinite(grad).all()), mode
        if mode == "sum":
            assert bool((grad >= 0).all()) and bool((grad.double() <= want_g).all())
            assert float(grad[want_g == 0].abs().max()) == 0.0
    # a weighted sum through the bad offsets: dw stays inside the reference's support too
    wd = w.float().to(dev).requires_grad_()
    pd = torch.ones(n, device=dev, requires_grad=True)
    F_.bag_pool_fields(wd, values.to(dev), bad.to(dev).to(ot), fo, "sum", per_sample_weights=pd).sum().backward()
    assert F_.index_errors_seen()
    assert bool(torch.isfinite(pd.grad).all()) and bool(torch.isfinite(wd.grad).all())


# ------------------------------------------------------------------------------------------------ 4. edge sizes
def test_no_values_and_no_bags(dev):
    from torecsys_amd import functional as F_
    fo = field_starts(SIZES).to(dev)
    wd = torch.randn(V, 16, device=dev, requires_grad=True)
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    for mode in ("sum", "mean", "max"):
        wd.grad = None
        y = F_.bag_pool_fields(wd, none, torch.zeros(NF * 2 + 1, dtype=torch.int64, device=dev), fo, mode)
        assert tuple(y.shape) == (2, NF, 16) and float(y.detach().abs().max()) == 0.0
        y.sum().backward()
        assert tuple(wd.grad.shape) == (V, 16) and float(wd.grad.abs().max()) == 0.0
    y = F_.bag_pool_fields(wd, torch.ones(4, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                           fo, "sum")
    assert tuple(y.shape) == (0, NF, 16)
    y.sum().backward()
    assert float(wd.grad.abs().max()) == 0.0


@pytest.mark.parametrize("method", ["avg_pooling", "max_pooling", "sum"])
def test_one_field_is_the_single_field_module(dev, method):
    """F = 1: the forward of RaggedListIndicesEmbedding(include_last_offset=True), bit for bit"""
    from torecsys_amd.inputs import RaggedListIndicesEmbedding, RaggedMultiListIndicesEmbedding
    E = 16
    g = torch.Generator().manual_seed(41)
    lens = boundary_lengths(g, _T(), B=B)
    offsets = field_major_lengths([lens])
    values = values_for(g, offsets, (50,), TRAIL)
    one = RaggedListIndicesEmbedding(embed_size=E, field_size=50, padding_idx=None, output_method=method,
                                     include_last_offset=True).to(dev)
    m = RaggedMultiListIndicesEmbedding(E, [50], output_method=method).to(dev)
    m.load_state_dict(one.state_dict())
    p = torch.rand(values.numel(), generator=g).to(dev) if method == "sum" else None
    gout = torch.randn(B, 1, E, generator=g).to(dev)
    a = m(values.to(dev), offsets.to(dev), p)
    b = one(values.to(dev), offsets.to(dev), p)
    assert a.names == b.names == ("B", "N", "E") and torch.equal(a.rename(None), b.rename(None))
    a.rename(None).backward(gout)
    b.rename(None).backward(gout)
    # the two modules bucket their lookups in builds of their own, and the order inside a bucket is the build's: the
    # gradients agree within rounding, not bit for bit
    assert rel_err(m.embedding.weight.grad, one.embedding.weight.grad) <= TOL32


def test_frozen_table(dev):
    """a frozen table with weights that need a gradient gives dw alone; a frozen table without weights no gradient work"""
    from torecsys_amd import functional as F_
    w, cases = _exact_case(32, False)
    mode, weighted, values, offsets, psw, gout, (want_y, _, want_dw) = cases[3]
    assert mode == "sum" and weighted
    y, grad, dw = _run(dev, torch.float32, torch.int64, torch.int64, w, values, offsets, "sum", psw, gout, table_grad=False)
    assert grad is None and torch.equal(y.double(), want_y) and torch.equal(dw.double(), want_dw)
    wd = w.float().to(dev)
    x = torch.ones(1, device=dev, requires_grad=True)      # something upstream that needs a gradient, the table does not
    y = F_.bag_pool_fields(wd, values.to(dev), offsets.to(dev), field_starts(SIZES).to(dev), "sum") * x
    y.sum().backward()
    assert wd.grad is None and x.grad is not None


# ------------------------------------------------------------------------------------------------ 5. module and router
@pytest.mark.parametrize("method", ["avg_pooling", "max_pooling", "sum"])
def test_module_inputs_route_and_fm_layer(dev, method):
    from torecsys_amd import functional as F_
    from torecsys_amd.inputs import Inputs, ListIndicesEmbedding, RaggedMultiListIndicesEmbedding
    from torecsys_amd.layers import FactorizationMachineLayer
    from torecsys_amd.optim import FusedSparseSGD
    E = 16
    values, offsets, _, psw, _ = _real_batch(E)
    m = RaggedMultiListIndicesEmbedding(E, list(SIZES), output_method=method).to(dev)
    assert list(m.state_dict().keys()) == ["embedding.weight"] and len(m) == NF and m.offsets.device.type == "cuda"
    p = psw.to(dev) if method == "sum" else None
    out = m(values.to(dev), offsets.to(dev), p)
    assert out.names == ("B", "N", "E") and tuple(out.shape) == (B, NF, E)
    mode = ListIndicesEmbedding._POOL[method]
    direct = F_.bag_pool_fields(m.embedding.weight, values.to(dev), offsets.to(dev), m.offsets, mode, per_sample_weights=p)
    assert torch.equal(out.rename(None), direct)
    # the Inputs route hands the offsets column, and the weights column if one is named, to the module
    m.set_schema("tags", offsets="tag_offsets", weights="tag_weights" if p is not None else None)
    batch = {"tags": values.to(dev), "tag_offsets": offsets.to(dev)}
    if p is not None:
        batch["tag_weights"] = p
    routed = Inputs(schema={"tags": m})(batch)["tags"]
    assert routed.names == ("B", "N", "E") and torch.equal(routed.rename(None), out.rename(None))
    # unchanged into an interaction layer and back: the table gradient against fp64
    fm = FactorizationMachineLayer().to(dev)
    fm(routed).rename(None).sum().backward()
    w64 = m.embedding.weight.detach().cpu().double()
    p64 = None if p is None else psw.double()
    x = fields_bag(w64, values, offsets, SIZES, mode, p64)[0].requires_grad_()
    (0.5 * (x.sum(1) ** 2 - (x ** 2).sum(1))).sum().backward()
    want_g = fields_bag(w64, values, offsets, SIZES, mode, p64, x.grad)[1]
    assert rel_err(out.rename(None).cpu(), x.detach()) <= TOL32
    assert rel_err(m.embedding.weight.grad.cpu(), want_g) <= TOL32
    with pytest.raises(NotImplementedError):
        m.set_fused_optimizer(FusedSparseSGD(0.1))

"""GPU tests of functional.bag_pool_ragged and RaggedListIndicesEmbedding (csrc/bag_ragged.hip: trs_bag_pool_ragged_fwd,
trs_bag_owner; csrc/bag.hip: trs_scatter_rows_ragged, trs_bag_weight_grad_ragged).  Reference: tests/bag_ragged_ref.py, the
fp64 restatement that tests/test_bag_ragged_host.py pins to torch.nn.functional.embedding_bag(ids, w, offsets, ...), and
F.embedding_bag itself on the CPU for the real-valued test.

Exact tests use the operands of tests/test_gpu_bag_masked.py: integer table entries in [-4, 4], weights in {0.5, 1, 2},
output-gradient entries in [-2, 2].  Every sum is then exact in fp32: the finest terms are the mean's gradient, multiples
of 1 / cnt >= 2^-11 (cnt a power of two <= 2048) below 2 in size, so a table row's sum over all n < 2^12 lookups is a
multiple of 2^-11 below 2^13 -- 24 bits; the weighted terms (multiples of 1/2 below 4) and the forward sums need fewer.  So
the kernel's result is the fp64 result rounded once to the dtype, whatever order the terms are added in: torch.equal.  For
the mean the live counts are powers of two.  One batch carries every boundary of the forward
(bag_ragged_ref.boundary_lengths): T = trs_bag_ragged_long_len() is read from the library, not written here."""
import functools

import pytest
import torch

from bag_ragged_ref import (bag_bounds, bags_from_lengths, boundary_lengths, embedding_bag_ref, pad_bags, pow2_lengths,
                            pow2_live, ragged_bag)
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
TOLBF = 1e-2
V, PAD = 53, 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _T():
    from torecsys_amd import functional as F_
    return F_.bag_ragged_long_len()


def _run(dev, dtype, idt, w, ids, offsets, mode, pad, exclude, psw, gout, last):
    """one forward + backward on the device; returns (out (B,E), table grad, dw), all on the CPU"""
    from torecsys_amd import functional as F_
    wd = w.to(dtype).to(dev).requires_grad_()
    pd = psw.to(dtype).to(dev).requires_grad_() if psw is not None else None
    y = F_.bag_pool_ragged(wd, ids.to(dev).to(idt), offsets.to(dev).to(idt), mode, pad, exclude_padding=exclude,
                           per_sample_weights=pd, include_last_offset=last)
    B = offsets.numel() - (1 if last else 0)
    assert tuple(y.shape) == (B, 1, w.shape[1]) and y.dtype == dtype
    y.backward(gout.to(dtype).to(dev).unsqueeze(1))
    return y.detach().squeeze(1).cpu(), wd.grad.cpu(), (pd.grad.cpu() if pd is not None else None)


# table rows with exactly this many lookups inside the bags: both sides of the walk's thresholds -- 32 / 33 (any-E path: one
# thread / queued), 64 / 65 (a lane group by itself / queued, one wave), 257 (two chunks of 256), 600 (three chunks)
HOT_ROWS = ((9, 32), (10, 33), (5, 64), (6, 65), (7, 257), (8, 600))


def _plant_hot_rows(g, ids, offsets):
    """the same bags with the live positions inside them re-drawn: HOT_ROWS planted, the rest spread over rows 11 .. V - 1"""
    ids = ids.clone()
    inside = torch.arange(ids.numel()) < int(offsets[-1])
    pos = ((ids != PAD) & inside).nonzero().flatten()
    pos = pos[torch.randperm(pos.numel(), generator=g)]
    k = 0
    for r, cnt in HOT_ROWS:
        ids[pos[k:k + cnt]] = r
        k += cnt
    assert k < pos.numel()
    ids[pos[k:]] = torch.randint(11, V, (pos.numel() - k,), generator=g)
    ids[~inside] = torch.randint(11, V, (int((~inside).sum()),), generator=g)
    for r, cnt in HOT_ROWS:
        assert int((ids == r).sum()) == cnt
    return ids


@functools.lru_cache(maxsize=None)
def _exact_case(kind, E, last):
    """(ids, offsets, w, psw, gout) and the expected (out, grad, dw) of every (mode, exclude, weighted) on one batch; built
    and evaluated in fp64 once per (batch kind, E, calling form), shared by the dtypes and index types"""
    T = _T()
    g = torch.Generator().manual_seed(1000 + E + (7 if kind == "long" else 0))
    if kind in ("boundary", "hot"):
        lengths, all_pad = boundary_lengths(g, T), (5,)
    else:                                         # every bag longer than T: the queue holds all B of them
        lengths, all_pad = [T + 1, 2 * T, T + 70, 2 * T + 5, T + 2], ()
    ids, offsets = bags_from_lengths(g, lengths, V, PAD, trailing=5, sprinkle=0.15, all_pad=all_pad)
    if kind == "hot":
        ids = _plant_hot_rows(g, ids, offsets)
    n = ids.numel()
    assert n < 2 ** 12
    w = torch.randint(-4, 5, (V, E), generator=g).double()
    psw = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (n,), generator=g)]
    gout = torch.randint(-2, 3, (len(lengths), E), generator=g).double()
    batches = {"plain": (ids, offsets), "pow2_live": (pow2_live(ids, offsets, PAD), offsets),
               "pow2_len": pow2_lengths(ids, offsets)}
    if not last:      # the last bag runs to the end of ids: no ids behind it
        batches = {k: (i[:int(o[-1])], o[:-1]) for k, (i, o) in batches.items()}
    cases = []
    for mode, exclude, weighted in (("sum", True, False), ("sum", False, False), ("max", True, False),
                                    ("max", False, False), ("sum", True, True), ("sum", False, True),
                                    ("mean", True, False), ("mean", False, False)):
        i, o = batches["plain" if mode != "mean" else ("pow2_live" if exclude else "pow2_len")]
        p = psw[:i.numel()] if weighted else None
        want = ragged_bag(w, i, o, mode, PAD, exclude, p, gout, last)
        cases.append((mode, exclude, i, o, p, want))
    return w, gout, cases


def _check_exact(dev, dtype, idt, kind, E, last):
    w, gout, cases = _exact_case(kind, E, last)
    for mode, exclude, ids, offsets, psw, (want_y, want_g, want_dw) in cases:
        tag = (mode, exclude, psw is not None)
        y, grad, dw = _run(dev, dtype, idt, w, ids, offsets, mode, PAD, exclude, psw, gout, last)
        assert torch.equal(y, want_y.to(dtype)), tag
        assert torch.equal(grad, want_g.to(dtype)), tag
        assert float(grad[PAD].abs().max()) == 0.0, tag                       # the padding row: exactly zero
        empty = torch.tensor([all(exclude and int(ids[p]) == PAD for p in range(b, e))      # no position, or no live one
                              for b, e in bag_bounds(offsets, ids.numel(), last)])
        assert kind == "long" or int(empty.sum()) >= (3 if exclude else 2), tag
        if bool(empty.any()):
            assert float(y[empty].abs().max()) == 0.0, tag                    # empty bags: exactly zero rows
        if psw is not None:
            assert torch.equal(dw, want_dw.to(dtype)), tag
            if exclude:
                assert float(dw[ids == PAD].abs().max()) == 0.0, tag
            if last:
                assert float(dw[int(offsets[-1]):].abs().max()) == 0.0, tag   # ids that no bag holds


# ------------------------------------------------------------------------------------------------ 1. exact, every path
WIDTHS = ([(torch.bfloat16, E) for E in (8, 16, 32, 64, 128, 256, 512)]
          + [(torch.float32, E) for E in (4, 8, 16, 32, 64, 128, 256)]
          + [(torch.float32, 5), (torch.float32, 12), (torch.bfloat16, 5), (torch.bfloat16, 12)])


@pytest.mark.parametrize("idt,last", [(torch.int64, True), (torch.int32, False)])
@pytest.mark.parametrize("dtype,E", WIDTHS)
def test_exact_integer_operands(dev, dtype, E, idt, last):
    """Every lane-group width (1 .. 64 lanes per row) and the any-E path (E = 5, 12): sum / mean / max / weighted sum, each
    with and without exclusion, on the batch of bag lengths [0, 1, 3, 4, 5, 7, 8, 9, T-1, T, T+1, 2T+3, 0, random <= 12];
    padding sprinkled in, one bag of nothing but padding, ids behind the last bag in the include_last_offset form.  Out, the
    dense table gradient and dw equal the fp64 result rounded once."""
    _check_exact(dev, dtype, idt, "boundary", E, last)


@pytest.mark.parametrize("dtype,E", [(torch.bfloat16, 64), (torch.bfloat16, 512), (torch.float32, 4), (torch.float32, 16),
                                     (torch.float32, 5)])
def test_exact_every_bag_long(dev, dtype, E):
    """B = 5 bags, all longer than T: every bag goes through the queue (none on the any-E path, which has no second tier)"""
    _check_exact(dev, dtype, torch.int64, "long", E, True)


@pytest.mark.parametrize("dtype,E,last", [(torch.bfloat16, 64, True), (torch.bfloat16, 8, False), (torch.bfloat16, 512, True),
                                          (torch.float32, 16, False), (torch.float32, 256, True), (torch.float32, 5, True),
                                          (torch.bfloat16, 12, False)])
def test_exact_hot_table_rows(dev, dtype, E, last):
    """The boundary batch with a few ids repeated: table rows of exactly 32, 33, 64, 65, 257 and 600 lookups, so the table
    gradient of the lane-group path goes through the hot-row queue -- one wave per (row, chunk), its lane groups striding
    the bucket, the fold across them, the single-chunk store and the chunk partials added by the finish kernel -- and that
    of the any-E path through its queue.  Sum, weighted sum and max (and the mean, whose power-of-two cut leaves the
    largest rows above both thresholds): out, table gradient and dw equal the fp64 result rounded once."""
    _, _, cases = _exact_case("hot", E, last)
    for mode, exclude, ids, _, _, _ in cases:
        counts = torch.bincount(ids[ids != PAD], minlength=V)
        assert int(counts.max()) > 256 and int(((counts > 64) & (counts <= 256)).sum()) >= 1, (mode, exclude)
    _check_exact(dev, dtype, torch.int64 if last else torch.int32, "hot", E, last)


@pytest.mark.parametrize("idt,last", [(torch.int64, False), (torch.int32, True)])
@pytest.mark.parametrize("dtype,E", [(torch.bfloat16, 64), (torch.float32, 5)])
def test_exact_other_index_type_and_form_pairs(dev, dtype, E, idt, last):
    """test_exact_integer_operands pairs int64 with a closing offset and int32 without: the other two pairings"""
    _check_exact(dev, dtype, idt, "boundary", E, last)


def test_mixed_index_types_and_frozen_table(dev):
    """int64 ids with int32 offsets and the other way round give the result of one type throughout; a frozen table with
    weights that need a gradient gives dw alone, a frozen table without weights no gradient work at all"""
    from torecsys_amd import functional as F_
    w, gout, cases = _exact_case("boundary", 16, True)
    mode, exclude, ids, offsets, psw, (want_y, _, want_dw) = cases[4]
    assert mode == "sum" and exclude and psw is not None
    wd = w.float().to(dev)
    for it, ot in ((torch.int64, torch.int32), (torch.int32, torch.int64)):
        pd = psw.float().to(dev).requires_grad_()
        y = F_.bag_pool_ragged(wd, ids.to(dev).to(it), offsets.to(dev).to(ot), "sum", PAD, exclude_padding=True,
                               per_sample_weights=pd, include_last_offset=True)
        y.backward(gout.float().to(dev).unsqueeze(1))
        assert torch.equal(y.detach().squeeze(1).cpu(), want_y.float()) and torch.equal(pd.grad.cpu(), want_dw.float())
    x = torch.ones(1, device=dev, requires_grad=True)      # something upstream that needs a gradient, the table does not
    y = F_.bag_pool_ragged(wd, ids.to(dev), offsets.to(dev), "sum", PAD, include_last_offset=True) * x
    y.sum().backward()
    assert wd.grad is None and x.grad is not None


# ------------------------------------------------------------------------------------------------ 2. real values
@functools.lru_cache(maxsize=None)
def _real_batch(E, short):
    """Gaussian table, ids with repeats, 20 % padding; bags on both sides of T (``short``: none above T)"""
    T = _T()
    g = torch.Generator().manual_seed(500 + E)
    lengths = boundary_lengths(g, T, B=48)
    if short:
        lengths = [min(x, T) for x in lengths]
    ids, offsets = bags_from_lengths(g, lengths, 200, PAD, sprinkle=0.2, all_pad=(5,))
    w = torch.randn(200, E, generator=g)
    psw = torch.rand(ids.numel(), generator=g) * 2
    gout = torch.randn(len(lengths), E, generator=g)
    return ids, offsets, w, psw, gout


@pytest.mark.parametrize("E", [64, 12])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_real_values_against_embedding_bag(dev, dtype, E):
    """F.embedding_bag(ids, w, offsets) on the CPU, in fp64 on the dtype-rounded inputs, is the reference; bounds of
    tests/test_gpu_bag.py: 1e-5 fp32, 1e-2 bf16, the max bit-exact"""
    ids, offsets, w, psw, gout = _real_batch(E, False)
    w, psw, gout = (t.to(dtype).double() for t in (w, psw, gout))
    tol = TOL32 if dtype == torch.float32 else TOLBF
    for mode, p in (("sum", None), ("mean", None), ("max", None), ("sum", psw)):
        want_y, want_g, want_dw = embedding_bag_ref(w, ids, offsets, mode, PAD, p, gout, True)
        y, grad, dw = _run(dev, dtype, torch.int64, w, ids, offsets, mode, PAD, True, p, gout, True)
        tag = (mode, p is not None)
        if mode == "max":
            assert torch.equal(y.double(), want_y), tag
        else:
            assert rel_err(y, want_y) <= tol, tag
        assert rel_err(grad, want_g) <= tol, tag
        assert float(grad[PAD].abs().max()) == 0.0 and float(y[5].abs().max()) == 0.0, tag
        if p is not None:
            assert rel_err(dw, want_dw) <= tol, tag


@pytest.mark.parametrize("E", [64, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_same_call_twice_is_bit_identical(dev, dtype, E):
    """The order in which the long bags enter the queue is free, the result is not: out, the table gradient and dw of two
    runs of the same call are equal bit for bit (real values, bags on both sides of T).  The same call: the same tensors --
    the table gradient is summed in the order of the row buckets of ``ids``, which the bucket build fixes once per ids
    tensor (its order inside a bucket is not specified, and is not this kernel's)."""
    from torecsys_amd import functional as F_
    ids, offsets, w, psw, gout = _real_batch(E, False)
    ids_d, off_d, g_d = ids.to(dev), offsets.to(dev), gout.to(dtype).to(dev).unsqueeze(1)
    assert max(e - b for b, e in bag_bounds(offsets, ids.numel(), True)) > _T()

    def run(mode, p):
        wd = w.to(dtype).to(dev).requires_grad_()
        pd = p.to(dtype).to(dev).requires_grad_() if p is not None else None
        y = F_.bag_pool_ragged(wd, ids_d, off_d, mode, PAD, exclude_padding=True, per_sample_weights=pd,
                               include_last_offset=True)
        y.backward(g_d)
        return {"out": y.detach(), "grad": wd.grad, "dw": None if pd is None else pd.grad}

    for mode, p in (("sum", None), ("mean", None), ("max", None), ("sum", psw)):
        a, b = run(mode, p), run(mode, p)
        for k in a:
            assert a[k] is None or torch.equal(a[k], b[k]), (mode, p is not None, k)


@pytest.mark.parametrize("E", [64, 16, 12])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_forward_bit_equal_to_padded_op(dev, dtype, E):
    """bags of at most T ids: the same list-order fp32 sum as bag_pool(exclude_padding=True) on the bags padded to the
    longest -- sum, mean, max and the weighted sum, real values"""
    from torecsys_amd import functional as F_
    ids, offsets, w, psw, _ = _real_batch(E, True)
    idx, wts = pad_bags(ids, offsets, PAD, True, psw)
    assert idx.shape[1] == _T()
    wd = w.to(dtype).to(dev)
    with torch.no_grad():
        for mode, p, pw in (("sum", None, None), ("mean", None, None), ("max", None, None), ("sum", psw, wts)):
            y = F_.bag_pool_ragged(wd, ids.to(dev), offsets.to(dev), mode, PAD, exclude_padding=True,
                                   per_sample_weights=None if p is None else p.to(dtype).to(dev),
                                   include_last_offset=True)
            z = F_.bag_pool(wd, idx.to(dev), mode, PAD, exclude_padding=True,
                            per_sample_weights=None if pw is None else pw.to(dtype).to(dev))
            assert torch.equal(y, z), mode


# ------------------------------------------------------------------------------------------------ 3. offsets out of range
@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
@pytest.mark.parametrize("E", [16, 5])
def test_bad_offsets_are_clamped_and_flagged(dev, E, idt):
    """a decreasing pair (that bag is empty) and an offset past n (clamped: the bag that begins there is empty): zero rows
    for those, the other bags right, the index flag raised -- and nothing read outside ids[0, n)"""
    from torecsys_amd import functional as F_
    g = torch.Generator().manual_seed(9)
    n = 20
    ids = torch.randint(1, V, (n,), generator=g)
    w = torch.randint(-4, 5, (V, E), generator=g).double()
    wd = w.float().to(dev)
    good = torch.tensor([0, 3, 3, 6, 10, 20])
    bad = torch.tensor([0, 3, 2, 6, 10, 25])
    assert bag_bounds(bad, n) == [(0, 3), (3, 3), (2, 6), (6, 10), (10, 20), (20, 20)]
    F_.index_errors_seen()
    with torch.no_grad():
        for mode in ("sum", "mean", "max"):
            y = F_.bag_pool_ragged(wd, ids.to(dev).to(idt), good.to(dev).to(idt), mode).squeeze(1).cpu()
            assert rel_err(y, ragged_bag(w, ids, good, mode)[0]) <= TOL32, mode
            assert not F_.index_errors_seen(), mode
            y = F_.bag_pool_ragged(wd, ids.to(dev).to(idt), bad.to(dev).to(idt), mode).squeeze(1).cpu()
            assert F_.index_errors_seen(), mode
            assert rel_err(y, ragged_bag(w, ids, bad, mode)[0]) <= TOL32, mode
            assert float(y[1].abs().max()) == 0.0 and float(y[5].abs().max()) == 0.0, mode
            # a negative offset and, with include_last_offset, a last offset past n
            neg = torch.tensor([-4, 3, 30])
            y = F_.bag_pool_ragged(wd, ids.to(dev).to(idt), neg.to(dev).to(idt), mode, include_last_offset=True)
            assert F_.index_errors_seen(), mode
            assert rel_err(y.squeeze(1).cpu(), ragged_bag(w, ids, neg, mode, include_last_offset=True)[0]) <= TOL32, mode


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bad_offsets_on_a_bag_of_the_second_tier(dev, dtype):
    """an offset past n closes a bag of more than T ids: the wave that takes it from the queue clamps it as the lane group
    did (its own bounds call carries no flag); a decreasing pair and the empty bag behind n beside it"""
    from torecsys_amd import functional as F_
    T, E = _T(), 16
    g = torch.Generator().manual_seed(13)
    n = 2 * T + 40
    ids = torch.randint(1, V, (n,), generator=g)
    w = torch.randint(-4, 5, (V, E), generator=g).double()
    bad = torch.tensor([0, 10, 5, 20, 3 * T])
    bounds = bag_bounds(bad, n)
    assert bounds == [(0, 10), (10, 10), (5, 20), (20, n), (n, n)] and n - 20 > T
    wd = w.to(dtype).to(dev)
    F_.index_errors_seen()
    with torch.no_grad():
        for mode in ("sum", "max", "mean"):
            y = F_.bag_pool_ragged(wd, ids.to(dev), bad.to(dev), mode).squeeze(1).cpu()
            assert F_.index_errors_seen(), mode
            want = ragged_bag(w, ids, bad, mode)[0]
            if mode == "mean":
                assert rel_err(y, want) <= (TOL32 if dtype == torch.float32 else TOLBF)
            else:
                assert torch.equal(y, want.to(dtype)), mode      # integer sums below 2^12: exact, rounded once
            assert float(y[1].abs().max()) == 0.0 and float(y[4].abs().max()) == 0.0, mode


def test_no_ids_and_no_bags(dev):
    from torecsys_amd import functional as F_
    wd = torch.randn(V, 16, device=dev, requires_grad=True)
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    y = F_.bag_pool_ragged(wd, none, torch.zeros(3, dtype=torch.int64, device=dev), "max")
    assert tuple(y.shape) == (3, 1, 16) and float(y.detach().abs().max()) == 0.0
    y.sum().backward()
    assert float(wd.grad.abs().max()) == 0.0
    y = F_.bag_pool_ragged(wd, torch.ones(4, dtype=torch.int64, device=dev), none, "sum")
    assert tuple(y.shape) == (0, 1, 16)


# ------------------------------------------------------------------------------------------------ 4. module and router
@pytest.mark.parametrize("method", ["avg_pooling", "max_pooling", "sum"])
def test_module_and_inputs_route(dev, method):
    from torecsys_amd import functional as F_
    from torecsys_amd.inputs import Inputs, ListIndicesEmbedding, RaggedListIndicesEmbedding
    from torecsys_amd.optim import FusedSparseSGD
    E = 16
    ids, offsets, _, psw, _ = _real_batch(E, False)
    B = offsets.numel() - 1
    old = ListIndicesEmbedding(embed_size=E, field_size=200, output_method=method).to(dev)
    m = RaggedListIndicesEmbedding(embed_size=E, field_size=200, output_method=method, exclude_padding=True,
                                   include_last_offset=True).to(dev)
    assert list(m.state_dict().keys()) == list(old.state_dict().keys()) == ["embedding.weight"]
    m.load_state_dict(old.state_dict())                      # a ListIndicesEmbedding checkpoint loads
    assert torch.equal(m.embedding.weight, old.embedding.weight)
    p = psw.to(dev) if method == "sum" else None
    out = m(ids.to(dev), offsets.to(dev), p)
    assert out.names == ("B", "N", "E") and tuple(out.shape) == (B, 1, E)
    mode = ListIndicesEmbedding._POOL[method]
    w = m.embedding.weight.detach().cpu().double()
    want = ragged_bag(w, ids, offsets, mode, PAD, True, None if p is None else psw.double(), None, True)[0]
    got = out.rename(None).squeeze(1).cpu()
    assert torch.equal(got.double(), want) if mode == "max" else rel_err(got, want) <= TOL32
    direct = F_.bag_pool_ragged(m.embedding.weight, ids.to(dev), offsets.to(dev), mode, PAD, exclude_padding=True,
                                per_sample_weights=p, include_last_offset=True)
    assert torch.equal(out.rename(None), direct)
    # the Inputs route hands the offsets column, and the weights column if one is named, to the module
    m.set_schema("tags", offsets="tag_offsets", weights="tag_weights" if p is not None else None)
    batch = {"tags": ids.to(dev), "tag_offsets": offsets.to(dev)}
    if p is not None:
        batch["tag_weights"] = p
    routed = Inputs(schema={"tags": m})(batch)["tags"]
    assert routed.names == ("B", "N", "E") and torch.equal(routed.rename(None), out.rename(None))
    with pytest.raises(NotImplementedError):
        m.set_fused_optimizer(FusedSparseSGD(0.1))
    with pytest.raises(NotImplementedError):
        F_.bag_pool_ragged(m.embedding.weight, ids.to(dev), offsets.to(dev), "sum", opt=FusedSparseSGD(0.1))

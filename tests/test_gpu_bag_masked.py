"""GPU tests of bag_pool(exclude_padding=, per_sample_weights=) and ListIndicesEmbedding(exclude_padding=True)
(csrc/bag.hip: trs_bag_pool_masked_fwd, trs_scatter_rows_weighted, trs_bag_weight_grad).  Reference: what
torch.nn.functional.embedding_bag(idx, w, mode, padding_idx=pad, per_sample_weights=) computes on the CPU for 2-D ids --
directly where it serves the case, through its restatement tests/bag_masked_ref.py (pinned to it in fp64 by
tests/test_bag_masked_host.py) where it does not: the weighted sum without exclusion, an out-of-range id, fp64 operands
for the exact tests.

Exact tests: integer table entries in [-4, 4], weights in {0.5, 1, 2}, output-gradient entries in [-2, 2]; every sum is
then exact in fp32 (the largest, a table row's gradient over all B * L lookups, stays below 2^14), so the kernel's result
is the fp64 result rounded once to the dtype, whatever order the terms are added in: torch.equal.  Real-valued tests use the
bounds of tests/test_gpu_bag.py: 1e-5 relative for fp32, 1e-2 for bf16, the max bit-exact."""
import pytest
import torch

from bag_masked_ref import embedding_bag_ref, masked_bag
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
TOLBF = 1e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _other_ids(g, shape, V, pad):
    """ids in [0, V) that are not ``pad``"""
    ids = torch.randint(0, V - 1, shape, generator=g)
    return ids + (ids >= pad).long()


def _exact_bags(g, B, L, V, pad):
    """bag 0: nothing but padding; bag 1: no padding; bag 2: padding at every even position; the rest: trailing padding of
    random length (0 .. L)"""
    idx = _other_ids(g, (B, L), V, pad)
    keep = torch.randint(0, L + 1, (B,), generator=g)
    keep[1] = L
    keep[2] = L
    idx = torch.where(torch.arange(L).view(1, L) < keep.view(B, 1), idx, torch.full_like(idx, pad))
    idx[0] = pad
    idx[2, 0::2] = pad
    return idx


def _pow2_counts(idx, pad):
    """the same bags with every live count cut down to a power of two (0, 1, 2, 4, ...): live positions past it are padded"""
    live = idx != pad
    cnt = live.sum(1)
    target = torch.where(cnt > 0, 2 ** torch.log2(cnt.clamp_min(1).double()).floor().long(), torch.zeros_like(cnt))
    drop = live & (live.cumsum(1) > target.view(-1, 1))
    out = torch.where(drop, torch.full_like(idx, pad), idx)
    c = (out != pad).sum(1)
    assert bool(((c & (c - 1)) == 0).all())
    return out


def _exact_operands(g, B, L, V, E):
    w = torch.randint(-4, 5, (V, E), generator=g).double()
    psw = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (B, L), generator=g)]
    gout = torch.randint(-2, 3, (B, E), generator=g).double()
    return w, psw, gout


def _run(dev, dtype, idt, w, idx, mode, pad, exclude, psw, gout, opt=None):
    """one forward + backward on the device; returns (out (B,E), table grad, dw), all on the CPU"""
    from torecsys_amd import functional as F_
    wd = w.to(dtype).to(dev).requires_grad_()
    pd = psw.to(dtype).to(dev).requires_grad_() if psw is not None else None
    y = F_.bag_pool(wd, idx.to(dev).to(idt), mode, padding_idx=pad, exclude_padding=exclude, per_sample_weights=pd)
    assert tuple(y.shape) == (idx.shape[0], 1, w.shape[1]) and y.dtype == dtype
    y.backward(gout.to(dtype).to(dev).unsqueeze(1))
    return y.detach().squeeze(1).cpu(), wd.grad.cpu(), (pd.grad.cpu() if pd is not None else None)


def _check_exact(dev, dtype, idt, w, idx, mode, pad, exclude, psw, gout):
    V = w.shape[0]
    row = pad + V if pad < 0 else pad
    want_y, want_g, want_dw = masked_bag(w, idx, mode, pad=row, exclude=exclude, psw=psw, gout=gout)
    y, grad, dw = _run(dev, dtype, idt, w, idx, mode, pad, exclude, psw, gout)
    tag = (mode, exclude, psw is not None)
    assert torch.equal(y, want_y.to(dtype)), tag
    assert torch.equal(grad, want_g.to(dtype)), tag
    assert float(grad[row].abs().max()) == 0.0, tag                       # the padding row: exactly zero
    empty = (idx != row).sum(1) == 0
    if exclude and bool(empty.any()):
        assert float(y[empty].abs().max()) == 0.0, tag                    # an empty bag: exactly a zero row
    if psw is not None:
        assert torch.equal(dw, want_dw.to(dtype)), tag
        if exclude:
            assert float(dw[idx == row].abs().max()) == 0.0, tag          # excluded positions: exactly zero
    # (no gradient from the empty bag: its gout rows are non-zero and the table gradient above is exact)


def _all_exact_cases(dev, dtype, idt, g, B, L, V, E, pad):
    row = pad + V if pad < 0 else pad
    idx = _exact_bags(g, B, L, V, row)
    w, psw, gout = _exact_operands(g, B, L, V, E)
    assert bool((idx[0] == row).all()) and float(gout[0].abs().max()) > 0.0      # the empty bag, with a gradient coming in
    _check_exact(dev, dtype, idt, w, idx, "sum", pad, True, None, gout)
    _check_exact(dev, dtype, idt, w, idx, "max", pad, True, None, gout)
    _check_exact(dev, dtype, idt, w, idx, "sum", pad, True, psw, gout)
    _check_exact(dev, dtype, idt, w, idx, "sum", pad, False, psw, gout)
    _check_exact(dev, dtype, idt, w, _pow2_counts(idx, row), "mean", pad, True, None, gout)


# ------------------------------------------------------------------------------------------------ 1. exact, every path
@pytest.mark.parametrize("L", [1, 7, 9, 50])
@pytest.mark.parametrize("E", [64, 128, 16, 8, 10, 4])
@pytest.mark.parametrize("dtype,idt", [(torch.float32, torch.int64), (torch.float32, torch.int32),
                                       (torch.bfloat16, torch.int64), (torch.bfloat16, torch.int32)])
def test_exact_integer_operands(dev, dtype, idt, E, L):
    """sum / max / weighted sum with and without exclusion / mean over power-of-two counts: outputs, the dense table
    gradient and dw equal the fp64 result rounded once.  E = 10 (and 4 in bf16) take the one-thread-per-element path; L
    sits on either side of the walks' 4 and 8 rows in flight."""
    g = torch.Generator().manual_seed(100 + 7 * L + E)
    _all_exact_cases(dev, dtype, idt, g, 67, L, 53, E, 0)


@pytest.mark.parametrize("pad", [52, -1])
@pytest.mark.parametrize("E", [64, 10])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_exact_integer_operands_last_row_as_padding(dev, dtype, E, pad):
    """the padding row is V - 1, given as such and as -1"""
    g = torch.Generator().manual_seed(17 + E)
    _all_exact_cases(dev, dtype, torch.int64, g, 67, 9, 53, E, pad)


# ------------------------------------------------------------------------------------------------ 2. walk thresholds
def _planted(g, B, L, V, pad, planted, live_per_bag=None):
    """(B, L) ids in which table row r holds exactly n lookups for every (r, n) of ``planted``; the remaining positions are
    spread over the other rows or padded.  ``live_per_bag``: every bag has exactly that many live positions."""
    n_pos = B * L
    n_live = n_pos if live_per_bag is None else B * live_per_bag
    rows = [r for r in range(V) if r != pad and r not in dict(planted)]
    flat = torch.cat([torch.full((n,), r, dtype=torch.long) for r, n in planted])
    spare = n_live - flat.numel()
    assert spare >= 0
    if live_per_bag is None:
        spare //= 2                                                   # the other half of what is left: padding
    spread = torch.tensor(rows)[torch.randint(0, len(rows), (spare,), generator=g)]
    flat = torch.cat([flat, spread])
    flat = flat[torch.randperm(flat.numel(), generator=g)]
    if live_per_bag is None:
        full = torch.full((n_pos,), pad, dtype=torch.long)
        full[torch.randperm(n_pos, generator=g)[:flat.numel()]] = flat
        idx = full.reshape(B, L)
    else:
        idx = torch.full((B, L), pad, dtype=torch.long)
        where = torch.rand(B, L, generator=g).argsort(1)[:, :live_per_bag]
        idx.scatter_(1, where, flat.reshape(B, live_per_bag))
    for r, n in planted:
        assert int((idx == r).sum()) == n
    return idx


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("E,planted", [(16, ((5, 64), (6, 65), (7, 257), (8, 600))), (10, ((5, 32), (6, 33), (7, 257)))])
def test_exact_walk_thresholds(dev, dtype, E, planted):
    """Table rows with exactly 64, 65 (one lane group / queued), 257 (two chunks of 256) and 600 lookups (three chunks);
    on the element path (E = 10) 32, 33 and 257.  The weighted walk uses the thresholds of the argmax walk, so these are
    its thresholds too.  B * L = 1152 positions; weighted and max gradients on one batch that holds all planted rows.  The
    mean needs a power-of-two live count per bag for an exact scale -- 8 of L = 12, 768 live positions, fewer than the four
    planted rows need together -- so it runs on two batches of 8 live ids per bag: the rows of up to 257 lookups in one,
    the row of 600 in the other."""
    B, L, V, pad = 96, 12, 40, 0
    g = torch.Generator().manual_seed(29 + E)
    w, psw, gout = _exact_operands(g, B, L, V, E)
    idx = _planted(g, B, L, V, pad, planted)
    _check_exact(dev, dtype, torch.int64, w, idx, "sum", pad, True, psw, gout)
    _check_exact(dev, dtype, torch.int64, w, idx, "sum", pad, False, psw, gout)
    _check_exact(dev, dtype, torch.int64, w, idx, "max", pad, True, None, gout)
    small = tuple(p for p in planted if p[1] <= 257)
    for part in (small, tuple(p for p in planted if p[1] > 257)):
        if part:
            idx8 = _planted(g, B, L, V, pad, part, live_per_bag=8)
            want_y, want_g, _ = masked_bag(w, idx8, "mean", pad=pad, exclude=True, gout=gout)
            y, grad, _ = _run(dev, dtype, torch.int64, w, idx8, "mean", pad, True, None, gout)
            assert torch.equal(y, want_y.to(dtype)) and torch.equal(grad, want_g.to(dtype)), part


# ------------------------------------------------------------------------------------------------ 3. real values
def _zipf_bags(g, B, L, V, pad_frac):
    """as tests/test_gpu_bag.py: Zipf(1.05) ids in [1, V), trailing padding (id 0) of random length, one empty bag"""
    ranks = torch.arange(1, V, dtype=torch.float64)
    p = ranks.pow(-1.05)
    idx = 1 + torch.multinomial(p / p.sum(), B * L, replacement=True, generator=g).reshape(B, L)
    keep = torch.rand(B, generator=g) * 2 * (1 - pad_frac) * L
    idx = torch.where(torch.arange(L).view(1, L) < keep.view(B, 1), idx, torch.zeros_like(idx))
    idx[0] = 0
    return idx


@pytest.mark.parametrize("L", [3, 50, 300])
@pytest.mark.parametrize("E", [64, 10])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_real_values_against_embedding_bag(dev, dtype, E, L):
    """Gaussian table, Zipf ids, 60 % padding: F.embedding_bag on the CPU, on the dtype-rounded inputs, is the reference;
    the mean's counts are whatever the padding leaves (not powers of two).  It is evaluated in fp64: in fp32 its own
    backward (a serial index_add, 7076 lookups on the head row at L = 300) is 1.07e-5 away from its fp64 self on the sum's
    gradient, more than the 1e-5 asked of the kernel."""
    B, V, pad = 384, 1000, 0
    g = torch.Generator().manual_seed(77 + L + E)
    idx = _zipf_bags(g, B, L, V, 0.6)
    cnt = (idx != pad).sum(1)
    assert L < 50 or bool(((cnt & (cnt - 1)) != 0).any())
    w = torch.randn(V, E, generator=g).to(dtype).double()
    psw = (torch.rand(B, L, generator=g) * 2).to(dtype).double()
    gout = torch.randn(B, E, generator=g).to(dtype).double()
    tol = TOL32 if dtype == torch.float32 else TOLBF
    for mode, exclude, p in (("sum", True, None), ("mean", True, None), ("max", True, None), ("sum", True, psw),
                             ("sum", False, psw)):
        want_y, want_g, want_dw = embedding_bag_ref(w, idx, mode, pad if exclude else None, p, gout)
        if not exclude:
            want_g[pad] = 0                       # read like any row, but it receives no gradient
        y, grad, dw = _run(dev, dtype, torch.int64, w, idx, mode, pad, exclude, p, gout)
        tag = (mode, exclude, p is not None)
        if mode == "max":
            assert torch.equal(y.double(), want_y), tag
        else:
            assert rel_err(y, want_y) <= tol, tag
        assert rel_err(grad, want_g) <= tol, tag
        assert float(grad[pad].abs().max()) == 0.0, tag
        if exclude:
            assert float(y[0].abs().max()) == 0.0, tag
        if p is not None:
            assert rel_err(dw, want_dw) <= tol, tag
            if exclude:
                assert float(dw[idx == pad].abs().max()) == 0.0, tag


# ------------------------------------------------------------------------------------------------ 4. module and flags
@pytest.mark.parametrize("method", ["avg_pooling", "max_pooling", "sum"])
def test_module_exclude_padding(dev, method):
    from torecsys_amd import functional as F_
    from torecsys_amd.inputs import ListIndicesEmbedding
    B, L, E, V = 67, 9, 16, 53
    g = torch.Generator().manual_seed(5)
    idx = _exact_bags(g, B, L, V, 0)
    m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method, exclude_padding=True).to(dev)
    off = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method).to(dev)
    assert list(m.state_dict().keys()) == list(off.state_dict().keys())
    off.load_state_dict(m.state_dict())
    out = m(idx.to(dev))
    assert out.names == ("B", "N", "E") and tuple(out.shape) == (B, 1, E)
    mode = ListIndicesEmbedding._POOL[method]
    w = m.embedding.weight.detach().cpu()
    want, _, _ = embedding_bag_ref(w, idx, mode, 0)
    if mode == "max":
        assert torch.equal(out.rename(None).squeeze(1).cpu(), want)
    else:
        assert rel_err(out.rename(None).squeeze(1).cpu(), want) <= TOL32
    # the option off: exactly the existing call
    plain = F_.bag_pool(off.embedding.weight, idx.to(dev), mode, 0)
    assert torch.equal(off(idx.to(dev)).rename(None), plain)
    if mode == "mean":                            # (the module's padding row is zeros: only the divisor tells them apart)
        assert not torch.equal(plain, out.rename(None))
    if method == "sum":
        psw = torch.rand(B, L, generator=g)
        yw = m(idx.to(dev), psw.to(dev))
        assert yw.names == ("B", "N", "E") and tuple(yw.shape) == (B, 1, E)
        want_w, _, _ = embedding_bag_ref(w, idx, "sum", 0, psw)
        assert rel_err(yw.rename(None).squeeze(1).cpu(), want_w) <= TOL32


@pytest.mark.parametrize("E", [16, 10])
def test_live_out_of_range_id(dev, E):
    """a live id outside [0, V) reads as a zero row, still counts in the mean's divisor, and raises the lazy flag"""
    from torecsys_amd import functional as F_
    V, pad = 20, 0
    g = torch.Generator().manual_seed(3)
    w = torch.randn(V, E, generator=g)
    idx = torch.tensor([[1, V + 5, 3, 0, 0], [4, 4, 2, 0, 7], [0, 0, 0, 0, 0]])
    gout = torch.randn(3, E, generator=g)
    F_.index_errors_seen()
    for mode in ("mean", "sum", "max"):
        want_y, want_g, _ = masked_bag(w.double(), idx, mode, pad=pad, exclude=True, gout=gout.double())
        y, grad, _ = _run(dev, torch.float32, torch.int64, w, idx, mode, pad, True, None, gout)
        assert rel_err(y, want_y) <= TOL32 and rel_err(grad, want_g) <= TOL32, mode
        assert F_.index_errors_seen(), mode
        assert not F_.index_errors_seen()
    want_mean = (w[1] + w[3]) / 3                                     # three live positions, one of them a zero row
    y, _, _ = _run(dev, torch.float32, torch.int64, w, idx, "mean", pad, True, None, gout)
    assert rel_err(y[0], want_mean) <= TOL32
    assert F_.index_errors_seen()


@pytest.mark.parametrize("E", [16, 10])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_no_padding_present_equals_plain_bag_pool(dev, dtype, E):
    """One autograd node serves both forward entries (trs_bag_pool_fwd, trs_bag_pool_masked_fwd) and both backward routes.
    Where no position holds the padding id they coincide: the same terms, so sum and max agree bit for bit, outputs and
    table gradients.  Integer operands as in the exact tests above: each call builds its own row buckets, and the order of
    the lookups inside a bucket (positions handed out by atomics) is not the same from build to build, so only sums that
    are exact in fp32 can be compared with torch.equal.  (Not the mean: 1 / L in the table's dtype against 1 / cnt in
    fp32, by design.)"""
    B, L, V, pad = 67, 9, 53, 0
    g = torch.Generator().manual_seed(23)
    idx = torch.randint(1, V, (B, L), generator=g)
    w, _, gout = _exact_operands(g, B, L, V, E)
    assert int(idx.min()) >= 1
    for mode in ("sum", "max"):
        y_m, grad_m, _ = _run(dev, dtype, torch.int64, w, idx, mode, pad, True, None, gout)
        y_p, grad_p, _ = _run(dev, dtype, torch.int64, w, idx, mode, pad, False, None, gout)
        assert torch.equal(y_m, y_p), mode
        assert torch.equal(grad_m, grad_p), mode
        assert float(grad_p.abs().max()) > 0.0 and float(grad_p[pad].abs().max()) == 0.0, mode


# ------------------------------------------------------------------------------------------------ 5. fused optimizer
@pytest.mark.parametrize("kind", ["sgd", "adagrad"])
def test_fused_optimizer_masked_mean_equals_dense_step(dev, kind):
    from torecsys_amd import functional as F_
    from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseSGD
    B, L, E, V, pad, lr = 384, 12, 16, 300, 0, 0.05
    g = torch.Generator().manual_seed(11)
    idx = _zipf_bags(g, B, L, V, 0.4)
    idx = torch.where(idx >= 200, torch.zeros_like(idx), idx)          # rows 200.. are never looked up
    w0 = torch.randn(V, E, generator=g)
    gout = torch.randn(B, 1, E, generator=g).to(dev)
    # the dense gradient of the same call, and the dense step from it
    wd = w0.to(dev).requires_grad_()
    F_.bag_pool(wd, idx.to(dev), "mean", pad, exclude_padding=True).backward(gout)
    dense = torch.optim.SGD([wd], lr=lr) if kind == "sgd" else torch.optim.Adagrad([wd], lr=lr, eps=1e-10)
    dense.step()
    wf = w0.to(dev).requires_grad_()
    opt = FusedSparseSGD(lr) if kind == "sgd" else FusedSparseAdagrad(lr, eps=1e-10)
    F_.bag_pool(wf, idx.to(dev), "mean", pad, opt, exclude_padding=True).backward(gout)
    assert wf.grad is None
    got, want = wf.detach().cpu(), wd.detach().cpu()
    assert rel_err(got, want) <= TOL32
    touched = torch.zeros(V, dtype=torch.bool)
    touched[idx.reshape(-1)] = True
    touched[pad] = False
    assert bool(touched.any()) and not bool(touched[200:].any())
    assert torch.equal(got[~touched], w0[~touched])                   # the padding row and rows without lookups: bit-unchanged
    assert not torch.equal(got[touched], w0[touched])
    with pytest.raises(NotImplementedError):
        F_.bag_pool(wf, idx.to(dev), "sum", pad, opt, exclude_padding=True,
                    per_sample_weights=torch.ones(B, L, device=dev))

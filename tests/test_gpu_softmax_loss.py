"""functional.softmax_scores_loss / EmbeddingPairScorer.softmax_loss / losses.FullSoftmaxLoss (csrc/softmax_loss.hip) against
the fp64 reference of tests/softmax_loss_ref.py over the operands after rounding to the table dtype.  B = 70 leaves a ragged
anchor tile; Vt = 127 / 129 / 1 000 / 5 003 are below one 128-row tile, one past it, and several tiles over 1, 3 and 19
target ranges whose last tile is partial.

Bounds, per element, first order; u = 2^-24, gamma as tests/topk_ref.py, c = 2 fp32 ulps (relative 2 c u) for the device's expf and logf: HIP's published table of
single-precision functions gives 1 ulp for both; that document is not part of this tree, so twice its figure is taken.
  score   bz[b, j] = gamma(E) scale sum_e |a_be t_je|: E - 1 additions and the multiplication by scale.
  lse     max_j bz (logsumexp moves by at most the largest score error) + gamma(n_sum) + u (2 c log Vt + |lse|).  n_sum
          counts what one term exp(z - m) of the sum can pass: its subtraction and expf (2 c + 1), at most Vt additions,
          and one rescaling s * expf(m - m') (2 c + 2 roundings) per tile of at least 32 rows and per fold (the four lanes of
          an anchor, the ranges; 4 spare).  The rounded subtraction z - m perturbs a term by u |z - m| relative, over the sum
          at most u times the p-weighted mean of m - z <= u log Vt, inside the log Vt term.
  loss    = (m - z_y) + log s, so the lse bound without u |lse|, plus bz[b, y_b] and u (log Vt + 2 |loss|) for the two
          roundings (|m - z_y| <= log Vt + |loss|).
  w       = g (p - onehot), p = exp(z - lse): dp = p (bz + b_lse + u |z - lse| + 2 c u), dw = |g| dp + 2 u |w|.
  dA, dT  scale sum (dw + (ub + gamma(n + 2)) |w|) |t_je| resp. |a_be| + (uo + u) |result|: the operand w rounded once to
          the table dtype (ub = 2^-9 for bf16, 0 for fp32: the figure the kernel was specified with.  It is half of bf16's
          unit roundoff, so the kernel feeds w to the matrix cores as a bf16 pair hi + lo, 2^-16 relative), n = Vt resp. B fp32 accumulations (any
          order), the scaling, and one output rounding by the format's unit roundoff, uo = 2^-8 for bf16's 8 significant
          bits and 0 for fp32.
The largest error / bound ratios each test prints are recorded in profiles/softmax_loss_kernels.md."""
import math
from functools import lru_cache

import pytest
import torch

from softmax_loss_ref import softmax_loss_ref, splits
from topk_ref import gamma

gpu = pytest.mark.gpu
B = 70
DTYPES = [torch.bfloat16, torch.float32]
U, C_ULP = 2.0 ** -24, 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _F():
    from torecsys_amd import functional as F_
    return F_


def bounds(a, t, scale, g, ref, dtype):
    (nb, E), Vt = a.shape, t.shape[0]
    ub, uo = (2.0 ** -9, 2.0 ** -8) if dtype == torch.bfloat16 else (0.0, 0.0)
    A, T = a.double().abs(), t.double().abs()
    bz = gamma(E) * scale * (A @ T.T)
    n_sum = Vt + (2 * C_ULP + 2) * (Vt // 32 + 4) + 2 * C_ULP + 1
    b_sum = bz.amax(dim=1) + gamma(n_sum) + U * 2 * C_ULP * math.log(Vt)
    y = ref["keep"].nonzero().reshape(-1)
    b_loss = torch.zeros(nb, dtype=torch.float64)
    b_loss[y] = (b_sum + U * (math.log(Vt) + 2 * ref["loss"]))[y] + bz[y, ref["labels"][y]]
    b_lse = b_sum + U * ref["lse"].abs()
    p = torch.exp(ref["z"] - ref["lse"][:, None])
    dp = p * (bz + b_lse[:, None] + U * (ref["z"] - ref["lse"][:, None]).abs() + 2 * C_ULP * U)
    w = ref["w"].abs()
    dw = (g.double().abs() * ref["keep"])[:, None] * dp + 2 * U * w
    b_da = scale * ((dw + (ub + gamma(Vt + 2)) * w) @ T) + (uo + U) * ref["dA"].abs()
    b_dt = scale * ((dw + (ub + gamma(nb + 2)) * w).T @ A) + (uo + U) * ref["dT"].abs()
    return b_loss, b_da, b_dt


def run(dev, a, t, y, scale, g, dtype, need=(True, True), **kw):
    ad = a.to(dev, dtype).requires_grad_(need[0])
    td = t.to(dev, dtype).requires_grad_(need[1])
    loss = _F().softmax_scores_loss(ad, td, y.to(dev), scale, **kw)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (a.shape[0],)
    loss.backward(g.to(dev))
    return loss.detach().cpu(), None if ad.grad is None else ad.grad.cpu(), None if td.grad is None else td.grad.cpu()


def check(got, ref, bnd, what):
    """every element within its bound; prints the largest error / bound ratio of loss, dA, dT"""
    ratios = []
    for x, r, b in zip(got, (ref["loss"], ref["dA"], ref["dT"]), bnd):
        err = (x.double() - r).abs()
        assert bool(torch.isfinite(x).all())
        ratios.append(float((err / b.clamp_min(1e-300)).max()))
        assert bool((err <= b).all()), (what, ratios)
    print(f"{what}: max err / bound  loss {ratios[0]:.3f}  dA {ratios[1]:.3f}  dT {ratios[2]:.3f}")


@lru_cache(maxsize=None)
def case(Vt, E, dtype, scale, nb=B, integer=False):
    """inputs (already holding the dtype's values), labels over the whole range, g random per sample, and the reference"""
    gen = torch.Generator().manual_seed(Vt * 31 + E + nb)
    if integer:
        a, t = (torch.randint(-2, 3, (n, E), generator=gen).float() for n in (nb, Vt))
    else:
        a, t = ((0.5 * torch.randn(n, E, generator=gen)).to(dtype).float() for n in (nb, Vt))
    y = torch.randint(0, Vt, (nb,), generator=gen)
    g = torch.randn(nb, generator=gen)
    ref = softmax_loss_ref(a, t, y, scale, g)
    ref["labels"] = y
    return a, t, y, g, ref


def width(E, dtype):
    return (8 if dtype == torch.bfloat16 else 4) if E == "vec" else E


@gpu
@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("Vt", [127, 129, 1000, 5003])
@pytest.mark.parametrize("E", [32, 64, "vec"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_forward_and_gradients(dev, dtype, E, Vt, scale):
    a, t, y, g, ref = case(Vt, width(E, dtype), dtype, scale)
    check(run(dev, a, t, y, scale, g, dtype), ref, bounds(a, t, scale, g, ref, dtype), f"{dtype} E={E} Vt={Vt} scale={scale}")


@gpu
@pytest.mark.parametrize("E", [80, 256])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_wide_rows(dev, dtype, E):
    """more than four 16-column blocks of gradient per lane; 80: bf16 rows padded in LDS; 256: the smaller arrangements"""
    a, t, y, g, ref = case(1000, E, dtype, 0.25)
    check(run(dev, a, t, y, 0.25, g, dtype), ref, bounds(a, t, 0.25, g, ref, dtype), f"{dtype} E={E}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_stability(dev, dtype):
    """integer operands: scores reach +-256 and exp of them overflows without the running max"""
    Vt, E = 1000, 64
    a, t, y, g, ref = case(Vt, E, dtype, 1.0, integer=True)
    check(run(dev, a, t, y, 1.0, g, dtype), ref, bounds(a, t, 1.0, g, ref, dtype), f"{dtype} integer")
    # identical rows: every score is the same exact integer, the loss is log Vt
    loss, da, dt = run(dev, a, t[:1].expand(Vt, E).contiguous(), y, 1.0, g, dtype)
    ulp = 2.0 ** (math.floor(math.log2(math.log(Vt))) - 23)
    print(f"identical rows: loss - log Vt = {float((loss.double() - math.log(Vt)).abs().max()) / ulp:.2f} ulp")
    assert float((loss.double() - math.log(Vt)).abs().max()) <= 4 * ulp
    # a positive more than 200 ahead of every other row: a = 2 everywhere, row y_b of 2s, the others of at most 0
    ones = torch.full((B, E), 2.0)
    far = -torch.randint(0, 3, (Vt, E), generator=torch.Generator().manual_seed(1)).float()
    y1 = torch.full((B,), 17)
    far[17] = 2.0
    loss, da, dt = run(dev, ones, far, y1, 1.0, g, dtype)
    assert bool((loss >= 0).all()) and bool((loss <= 1e-30).all())
    assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(dt).all())


@gpu
@pytest.mark.parametrize("Vt", [1000, 5003])
@pytest.mark.parametrize("ldt", [torch.int32, torch.int64])
def test_labels(dev, Vt, ldt):
    """labels on every boundary: rows 0, 127, 128, Vt - 1 and the first and last row of every target range; every third
    sample ignored; then one label out of range"""
    F_ = _F()
    dtype, E = torch.bfloat16, 32
    a, t, _, g, _ = case(Vt, E, dtype, 1.0)
    S = splits(B, Vt)
    per = (Vt + S - 1) // S
    spots = [0, 127, 128, Vt - 1] + [r for s in range(S) for r in (s * per, min((s + 1) * per, Vt) - 1)]
    y = torch.full((B,), -1)
    live = [b for b in range(B) if b % 3 != 0]
    assert len(spots) <= len(live)
    for i, b in enumerate(live):
        y[b] = spots[i % len(spots)]
    ref = softmax_loss_ref(a, t, y, 1.0, g)
    ref["labels"] = y
    F_.index_errors_seen()
    loss, da, dt = run(dev, a, t, y.to(ldt), 1.0, g, dtype)
    assert not F_.index_errors_seen()
    check((loss, da, dt), ref, bounds(a, t, 1.0, g, ref, dtype), f"labels Vt={Vt}")
    assert bool((loss[0::3] == 0).all()) and bool((da[0::3] == 0).all())
    y2 = y.clone()
    y2[1] = Vt      # one past the table: flagged, and treated as ignored
    loss2, da2, dt2 = run(dev, a, t, y2.to(ldt), 1.0, g, dtype)
    assert F_.index_errors_seen()
    y[1] = -1
    loss3, da3, dt3 = run(dev, a, t, y.to(ldt), 1.0, g, dtype)
    assert float(loss2[1]) == 0 and torch.equal(loss2, loss3) and torch.equal(da2, da3) and torch.equal(dt2, dt3)


@gpu
@pytest.mark.parametrize("Vt", [129, 5003])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_needs_grad_and_reproducible(dev, dtype, Vt):
    a, t, y, g, _ = case(Vt, 64, dtype, 0.25)
    both = run(dev, a, t, y, 0.25, g, dtype)
    again = run(dev, a, t, y, 0.25, g, dtype)
    assert all(torch.equal(x, z) for x, z in zip(both, again))
    only_a = run(dev, a, t, y, 0.25, g, dtype, need=(True, False))
    only_t = run(dev, a, t, y, 0.25, g, dtype, need=(False, True))
    assert only_a[2] is None and only_t[1] is None
    assert torch.equal(only_a[0], both[0]) and torch.equal(only_a[1], both[1]) and torch.equal(only_t[2], both[2])


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_in_batch(dev, dtype):
    """targets = the batch's positives, labels = arange; 600 samples cut the anchors of the target gradient into 2 ranges"""
    nb, E = 600, 32
    a, t, _, g, _ = case(nb, E, dtype, 1.0, nb=nb)
    y = torch.arange(nb)
    y[5] = -1
    assert splits(nb, nb) == 2
    ref = softmax_loss_ref(a, t, y, 1.0, g)
    ref["labels"] = y
    check(run(dev, a, t, y, 1.0, g, dtype), ref, bounds(a, t, 1.0, g, ref, dtype), f"in-batch {dtype}")


@gpu
@pytest.mark.parametrize("in_batch", [False, True])
def test_module_shared_table(dev, in_batch):
    """EmbeddingPairScorer.softmax_loss on one shared fp32 table, targets behind target_offset = 100: the mean over the
    non-ignored samples and the gradient of both regions of the table; FullSoftmaxLoss on the same rows"""
    from torecsys_amd.fused import EmbeddingPairScorer
    from torecsys_amd.losses import FullSoftmaxLoss
    torch.manual_seed(4)
    E, off, scale = 32, 100, 0.25
    m = EmbeddingPairScorer(E, 400, None, target_offset=off).to(dev)
    with torch.no_grad():
        m.anchor.weight.mul_(20.0)
    a_idx = torch.randint(0, 100, (B,), device=dev)
    pos = torch.randperm(300, device=dev)[:B]
    if not in_batch:
        pos[::7] = -1
    loss = m.softmax_loss(a_idx, pos, scale=scale, in_batch=in_batch)
    loss.backward()
    w = m.anchor.weight.detach().cpu()
    a = w[a_idx.cpu()]
    t = w[off + pos.cpu()] if in_batch else w[off:]
    y = torch.arange(B) if in_batch else pos.cpu()
    kept = int((y >= 0).sum())
    ref = softmax_loss_ref(a, t, y, scale, torch.full((B,), 1.0 / kept))
    ref["labels"] = y
    b_loss, b_da, b_dt = bounds(a, t, scale, torch.full((B,), 1.0 / kept), ref, torch.float32)
    assert abs(float(loss) - float(ref["loss"].sum()) / kept) <= float(b_loss.sum()) / kept + 2 * B * U * abs(float(loss))
    grad = torch.zeros(400, E, dtype=torch.float64)      # both regions: scatter the reference's rows, with their bounds
    gb = torch.full((400, E), 64 * U, dtype=torch.float64)
    gb = gb * m.anchor.weight.grad.abs().max().item()      # the dense additions of autograd's scatter and slice
    grad.index_add_(0, a_idx.cpu(), ref["dA"])
    gb.index_add_(0, a_idx.cpu(), b_da)
    rows = off + pos.cpu() if in_batch else torch.arange(off, 400)
    grad.index_add_(0, rows, ref["dT"])
    gb.index_add_(0, rows, b_dt)
    assert bool(((m.anchor.weight.grad.cpu().double() - grad).abs() <= gb).all())
    crit = FullSoftmaxLoss(scale=scale, reduction='sum')
    assert torch.equal(crit(a.to(dev), t.to(dev), y.to(dev)), _F().softmax_scores_loss(a.to(dev), t.to(dev), y.to(dev), scale).sum())


@pytest.mark.parametrize("case_,exc", [("mixed", TypeError), ("width", NotImplementedError), ("strided", ValueError),
                                       ("empty", ValueError), ("labels", TypeError), ("ignore", ValueError)])
def test_argument_errors_before_any_launch(case_, exc):
    """CPU tensors: every check comes before the device is looked at"""
    a, t, y = torch.zeros(4, 32), torch.zeros(200, 32), torch.zeros(4, dtype=torch.int64)
    if case_ == "mixed":
        t = t.bfloat16()
    if case_ == "width":
        a, t = torch.zeros(4, 6), torch.zeros(200, 6)
    if case_ == "strided":
        t = torch.zeros(200, 64)[:, ::2]
    if case_ == "empty":
        t = t[:0]
    if case_ == "labels":
        y = y.float()
    with pytest.raises(exc, match="softmax_scores_loss"):
        _F().softmax_scores_loss(a, t, y, ignore_index=3 if case_ == "ignore" else -1)

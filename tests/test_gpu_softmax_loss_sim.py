"""functional.softmax_scores_loss with sim='cosine' and / or a per-target bias, EmbeddingPairScorer.softmax_loss(target_bias=)
and losses.FullSoftmaxLoss(similarity=) against the fp64 autograd reference of tests/softmax_loss_sim_ref.py.

Bounds, per element, first order, on top of tests/test_gpu_softmax_loss.py's (u = 2^-24, gamma of tests/topk_ref.py, c = 2
ulps = 2 c u relative for a device function; ra, rt the inverse norms, 1 for 'dot'; S the number of streamed ranges):
  r       er = gamma(E) / 2 + 4 c u relative: the fp32 sum of E squares (gamma(E), halved by the root), sqrtf and the
          reciprocal taken as device functions (2 c u each).  A clamped norm gives 1 / eps with the same allowance.
  s       bs = gamma(E) ra rt sum_e |a_be t_je| + (2 er + 2 u) |s|: the dot product, the two inverse norms, the two extra
          multiplications.  'dot': the first term alone.
  z       bz = scale bs + u |z|: the multiplication by scale is inside gamma(E) as there, u |z| is the fp32 bias addition.
  lse, loss, w   as there with this bz (log sum exp(z - m) <= log Vt whatever the bias): b_sum, b_loss, dp, dw.
  d_bias  sum_b (dw + gamma(B + 2) |w|): B fp32 additions in any order, the fold of the four lanes and of the ranges.
  c       bc[b] = sum_j (dw |s| + |w| bs + (u + gamma(Vt + 2)) |w s|): the factors' errors, the product, the sum.
  dA      = scale ra (G - P), G = sum_j (w rt) T[j], P = ra c A[b] (absent where |A[b]| <= eps, and for 'dot').
          bG = sum_j (dw + |w| (er + u + ub + gamma(Vt + 2))) rt |t_je|: the factor rt and its product, the operand rounded
          to the table dtype (ub = 2^-9 for bf16 as there, 0 for fp32), Vt accumulations.  bP = ra |a_be| (bc + |c| (er +
          2 u)).  The two sides cancel, so what follows them is bounded in |G|_1 = sum_j |w| rt |t_je| and |P|_1 = ra |a_be|
          sum_j |w s|, not in |G - P|: per range the subtraction and the multiplication by scale ra (its er apart), then
          S - 1 additions of the ranges' partials: (gamma(S + 3) + er) (|G|_1 + |P|_1).  In all
          b_dA = scale ra (bG + bP + (gamma(S + 3) + er) (|G|_1 + |P|_1)) + uo |dA|, uo = 2^-8 for bf16, 0 for fp32.
  dT      the same with the roles exchanged (sums over b, B for Vt, c'[j]).
The largest error / bound ratios each test prints are recorded in profiles/softmax_loss_kernels.md."""
import math
from functools import lru_cache

import pytest
import torch

from softmax_loss_ref import splits
from softmax_loss_sim_ref import softmax_loss_sim_ref
from topk_ref import gamma

gpu = pytest.mark.gpu
both_dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
B, U, C_ULP = 70, 2.0 ** -24, 2
SCALE = {"cosine": 16.0, "dot": 0.25}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def loss_fn(*args, **kw):
    from torecsys_amd import functional as F_
    return F_.softmax_scores_loss(*args, **kw)


def bounds(a, t, scale, g, ref, dtype, sim, bias):
    """b_loss (B), b_dA (B, E), b_dT (Vt, E), b_dB (Vt) of the docstring"""
    (nb, E), Vt = a.shape, t.shape[0]
    ub, uo = (2.0 ** -9, 2.0 ** -8) if dtype == torch.bfloat16 else (0.0, 0.0)
    er = gamma(E) / 2 + 4 * C_ULP * U if sim == "cosine" else 0.0
    A, T, ra, rt = a.double().abs(), t.double().abs(), ref["ra"], ref["rt"]
    s, z, w = ref["s"].abs(), ref["z"], ref["w"].abs()
    bs = gamma(E) * (A @ T.T) * ra[:, None] * rt[None, :] + ((2 * er + 2 * U) * s if sim == "cosine" else 0.0)
    bz = scale * bs + (U * z.abs() if bias is not None else 0.0)
    n_sum = Vt + (2 * C_ULP + 2) * (Vt // 32 + 4) + 2 * C_ULP + 1
    b_sum = bz.amax(dim=1) + gamma(n_sum) + U * 2 * C_ULP * math.log(Vt)
    y = ref["keep"].nonzero().reshape(-1)
    b_loss = torch.zeros(nb, dtype=torch.float64)
    b_loss[y] = (b_sum + U * (math.log(Vt) + 2 * ref["loss"]))[y] + bz[y, ref["labels"][y]]
    b_lse = b_sum + U * ref["lse"].abs()
    p = torch.exp(z - ref["lse"][:, None])
    dp = p * (bz + b_lse[:, None] + U * (z - ref["lse"][:, None]).abs() + 2 * C_ULP * U)
    dw = (g.double().abs() * ref["keep"])[:, None] * dp + 2 * U * w

    def grad(dw, w, s, bs, rs, rr, Xs, Xr, ps, n, S, d):      # stationary rows s (rs, Xs, ps), streamed rows r, n of them
        bc = (dw * s + w * bs + (U + gamma(n + 2)) * w * s).sum(dim=1)
        c = (w * s).sum(dim=1)      # >= |c|
        bG = ((dw + w * (er + U + ub + gamma(n + 2))) * rr[None, :]) @ Xr
        bP = (ps * rs * (bc + c * (er + 2 * U)))[:, None] * Xs
        mag = (w * rr[None, :]) @ Xr + (ps * rs * c)[:, None] * Xs
        return scale * rs[:, None] * (bG + bP + (gamma(S + 3) + er) * mag) + uo * d.abs()

    b_da = grad(dw, w, s, bs, ra, rt, A, T, ref["pa"], Vt, splits(nb, Vt), ref["dA"])
    b_dt = grad(dw.T, w.T, s.T, bs.T, rt, ra, T, A, ref["pt"], nb, splits(Vt, nb), ref["dT"])
    return b_loss, b_da, b_dt, (dw + gamma(nb + 2) * w).sum(dim=0)


def run(dev, a, t, y, scale, g, dtype, sim, bias, need=(True, True, True)):
    ad = a.to(dev, dtype).requires_grad_(need[0])
    td = t.to(dev, dtype).requires_grad_(need[1])
    bd = None if bias is None else bias.to(dev).requires_grad_(need[2])
    loss = loss_fn(ad, td, y.to(dev), scale, sim=sim, bias=bd)
    loss.backward(g.to(dev))
    return [loss.detach().cpu()] + [None if x is None or x.grad is None else x.grad.cpu() for x in (ad, td, bd)]


def check(got, ref, bnd, what):
    """every element within its bound; prints the largest error / bound ratio of loss, dA, dT, d_bias"""
    ratios = []
    for x, r, b in zip(got, (ref["loss"], ref["dA"], ref["dT"], ref["dB"]), bnd):
        if x is not None:
            err = (x.double() - r).abs()
            ratios.append(float((err / b.clamp_min(1e-300)).max()))
            assert bool(torch.isfinite(x).all()) and bool((err <= b).all()), (what, ratios)
    print(f"{what}: max err / bound (loss, dA, dT, d_bias) " + " ".join(f"{r:.3f}" for r in ratios))


@lru_cache(maxsize=None)
def case(Vt, E, dtype, sim, with_bias, nb=B, degenerate=False):
    """inputs (already holding the dtype's values), labels over the whole range, g random per sample, and the reference"""
    gen = torch.Generator().manual_seed(Vt * 31 + E + nb)
    a, t = ((0.5 * torch.randn(n, E, generator=gen)).to(dtype).float() for n in (nb, Vt))
    y = torch.randint(0, Vt, (nb,), generator=gen)
    if degenerate:      # a zero row and a row of norm 1e-9 < eps on either side; sample 5 is labelled with the zero target
        a[3], t[7], a[11], t[130] = 0.0, 0.0, 0.0, 0.0
        a[11, 1] = t[130, 2] = float(torch.tensor(1e-9).to(dtype))
        y[5] = 7
    g = torch.randn(nb, generator=gen)
    bias = torch.randn(Vt, generator=gen) if with_bias else None
    ref = softmax_loss_sim_ref(a, t, y, SCALE[sim], g, sim, bias)
    ref["labels"] = y
    return a, t, y, g, bias, ref


def whole(dev, dtype, sim, with_bias, what, y=None, **kw):
    a, t, y0, g, bias, ref = case(dtype=dtype, sim=sim, with_bias=with_bias, **kw)
    if y is not None:      # other labels: a reference of its own
        ref = softmax_loss_sim_ref(a, t, y, SCALE[sim], g, sim, bias)
        ref["labels"] = y
    got = run(dev, a, t, y0 if y is None else y, SCALE[sim], g, dtype, sim, bias)
    check(got, ref, bounds(a, t, SCALE[sim], g, ref, dtype, sim, bias), f"{what} {dtype} {sim} bias={with_bias}")
    return ref


@gpu
@pytest.mark.parametrize("Vt", [129, 5003])
@pytest.mark.parametrize("E", [32, "vec"])
@pytest.mark.parametrize("sim,with_bias", [("cosine", False), ("cosine", True), ("dot", True)])
@both_dtypes
def test_forward_and_gradients(dev, dtype, sim, with_bias, E, Vt):
    E = (8 if dtype == torch.bfloat16 else 4) if E == "vec" else E
    whole(dev, dtype, sim, with_bias, f"E={E} Vt={Vt}", Vt=Vt, E=E)


@gpu
@pytest.mark.parametrize("E", [80, 256])
@both_dtypes
def test_wide_rows(dev, dtype, E):
    """16 column blocks of gradient per lane (bf16: one group of 16 stationary rows per wave); 80: bf16 rows padded in LDS"""
    whole(dev, dtype, "cosine", True, f"wide E={E}", Vt=1000, E=E)


@gpu
@both_dtypes
def test_in_batch(dev, dtype):
    """targets = the batch's positives, labels = arange, one ignored: the target gradient and d_bias cross 2 anchor ranges"""
    y = torch.arange(600)
    y[5] = -1
    assert splits(600, 600) == 2
    whole(dev, dtype, "cosine", True, "in-batch", y=y, Vt=600, E=32, nb=600)


@gpu
@both_dtypes
def test_degenerate_norms(dev, dtype):
    """zero rows and rows below eps on both sides: finite, within the bounds of the clamped reference, and no projection
    term: the zero rows' gradients are scale r sum (w r) x alone, which the reference's (pa = pt = 0) bounds already say"""
    ref = whole(dev, dtype, "cosine", True, "degenerate", Vt=1000, E=32, degenerate=True)
    assert float(ref["pa"][3]) == float(ref["pa"][11]) == float(ref["pt"][7]) == float(ref["pt"][130]) == 0.0
    assert float(ref["pa"].sum()) == B - 2 and float(ref["pt"].sum()) == 1000 - 2


@gpu
@pytest.mark.parametrize("Vt", [129, 5003])
@both_dtypes
def test_gradient_requests_and_reproducible(dev, dtype, Vt):
    a, t, y, g, bias, _ = case(Vt, 32, dtype, "cosine", True)
    all3 = run(dev, a, t, y, 16.0, g, dtype, "cosine", bias)
    assert all(torch.equal(x, z) for x, z in zip(all3, run(dev, a, t, y, 16.0, g, dtype, "cosine", bias)))
    for i in range(3):
        one = run(dev, a, t, y, 16.0, g, dtype, "cosine", bias, need=tuple(j == i for j in range(3)))
        assert [x is None for x in one[1:]] == [j != i for j in range(3)]
        assert torch.equal(one[0], all3[0]) and torch.equal(one[1 + i], all3[1 + i])


@gpu
@pytest.mark.parametrize("in_batch", [False, True])
def test_modules(dev, in_batch):
    """EmbeddingPairScorer(similarity='cosine').softmax_loss(target_bias=) on one shared fp32 table, targets behind
    target_offset = 100: loss, the gradient of both regions of the table and of the bias; FullSoftmaxLoss on the same rows"""
    from torecsys_amd.fused import EmbeddingPairScorer
    from torecsys_amd.losses import FullSoftmaxLoss
    torch.manual_seed(4)
    E, off, scale = 32, 100, 16.0
    m = EmbeddingPairScorer(E, 400, None, similarity='cosine', target_offset=off).to(dev)
    tb = torch.randn(300, device=dev).requires_grad_()
    a_idx = torch.randint(0, 100, (B,), device=dev)
    pos = torch.randperm(300, device=dev)[:B]
    if not in_batch:
        pos[::7] = -1
    loss = m.softmax_loss(a_idx, pos, scale=scale, in_batch=in_batch, target_bias=tb)
    loss.backward()
    w = m.anchor.weight.detach().cpu()
    a = w[a_idx.cpu()]
    t = w[off + pos.cpu()] if in_batch else w[off:]
    bias = tb.detach().cpu()[pos.cpu()] if in_batch else tb.detach().cpu()
    y = torch.arange(B) if in_batch else pos.cpu()
    g = torch.full((B,), 1.0 / int((y >= 0).sum()))
    ref = softmax_loss_sim_ref(a, t, y, scale, g, "cosine", bias)
    ref["labels"] = y
    b_loss, b_da, b_dt, b_db = bounds(a, t, scale, g, ref, torch.float32, "cosine", bias)
    loss = float(loss.detach())
    assert abs(loss - float((ref["loss"] * g).sum())) <= float((b_loss * g).sum()) + 2 * B * U * abs(loss)
    # both regions of the table, then the bias: the reference's rows scattered, with their bounds
    grad, db = torch.zeros(400, E, dtype=torch.float64), torch.zeros(300, dtype=torch.float64)
    gb = torch.full((400, E), 64 * U, dtype=torch.float64) * m.anchor.weight.grad.abs().max().item()      # autograd's adds
    bb = torch.zeros(300, dtype=torch.float64)
    rows = off + pos.cpu() if in_batch else torch.arange(off, 400)
    for dst, bnd, idx, d, b in ((grad, gb, a_idx.cpu(), ref["dA"], b_da), (grad, gb, rows, ref["dT"], b_dt),
                                (db, bb, rows - off, ref["dB"], b_db)):
        dst.index_add_(0, idx, d)
        bnd.index_add_(0, idx, b)
    assert bool(((m.anchor.weight.grad.cpu().double() - grad).abs() <= gb).all())
    assert bool(((tb.grad.cpu().double() - db).abs() <= bb).all())
    crit = FullSoftmaxLoss(scale=scale, reduction='sum', similarity='cosine')
    args = a.to(dev), t.to(dev), y.to(dev)
    assert torch.equal(crit(*args, bias.to(dev)), loss_fn(*args, scale, sim='cosine', bias=bias.to(dev)).sum())


@pytest.mark.parametrize("case_,exc", [("sim", ValueError), ("dtype", TypeError), ("length", ValueError), ("strided", ValueError)])
def test_argument_errors_before_any_launch(case_, exc):
    """CPU tensors: every check comes before the device is looked at"""
    a, t, y = torch.zeros(4, 32), torch.zeros(200, 32), torch.zeros(4, dtype=torch.int64)
    bias = {"sim": None, "dtype": torch.zeros(200).double(), "length": torch.zeros(199), "strided": torch.zeros(400)[::2]}[case_]
    with pytest.raises(exc, match="softmax_scores_loss"):
        loss_fn(a, t, y, sim="euclid" if case_ == "sim" else "cosine", bias=bias)

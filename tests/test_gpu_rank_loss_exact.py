"""The three ranking-loss kernels of csrc/rank.hip (rank_loss_partial_kernel, rank_loss_finish_kernel, rank_loss_bwd_kernel)
against tests/rank_ref.py in float64, the hinge kinds BIT FOR BIT: scores that are multiples of 1 / 4 in [-4, 4], so every
hinge term is a multiple of 1 / 8 and every fp32 sum of them exact (tests/gate_exact_ref.py; the guard and the trip
counts are checked on the CPU by tests/test_gate_exact_host.py).

Sizes: one workgroup and either side of two; 16 385 samples are 65 partials, the finish kernel's second trip; 65 537 the
partial kernel's.  Margin 0.625 leaves no hinge argument at 0, margin 1.0 many: there the gradient passes, as through
ATen's clamp(min=0) and margin_ranking_loss (derivative 1 at exactly 0), and sample 0 of every case (p = 1, n = 0) sits on
the kink with all its negatives tied for the adaptive hinge's maximum -- the first takes the gradient.

The smooth kinds (pointwise, bpr) run at the same sizes under the bounds of tests/test_gpu_rank.py: their terms are not
negative, so one dropped workgroup partial (256 samples of 16 385 or 65 537) moves the sum by 4e-3 to 1.6e-2 of itself."""
import pytest
import torch

import gate_exact_ref as R
from conftest import rel_err, sum_err

pytestmark = pytest.mark.gpu

F32, BF16, F64 = R.F32, R.BF16, R.F64
TOL = {F32: 1e-5, BF16: 1e-2}                   # tests/test_gpu_rank.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _forms(s, dtype, dev):
    """the scores as one (B, 1 + K) matrix (read in place, column 0 the positive) and as separate operands"""
    sd = s.to(dtype).to(dev)
    return (("matrix", sd, None), ("separate", sd[:, 0].contiguous(), sd[:, 1:].contiguous()))


def _grad_of(form, gp, gn):
    return gp if form == "matrix" else torch.cat([gp.reshape(-1, 1), gn], dim=1)


def _dev_mask(mask, dev):
    return None if mask is None else mask.to(dev)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dt_tag)
@pytest.mark.parametrize("case", R.RANK_SIZES, ids=R.rank_id)
def test_hinge_sum_and_gradient_exact(dev, case, dtype):
    """'sum': the loss has the float64 sum's bits and the gradient is exact, under both margins, every mask pattern and
    both operand forms; 'sample' and 'mean': denom is the count, the loss the float64 quotient rounded once"""
    from torecsys_amd import functional as F_
    B, K = case
    s = R.rank_scores(B, K)
    forms = _forms(s, dtype, dev)
    d = R.Diffs()
    for kind in R.RANK_EXACT_KINDS:
        for margin in R.RANK_MARGINS:
            zeros = int((R.rank_hinge_args(s, kind, margin) == 0).sum())
            assert (zeros > 0) == (margin == 1.0), (kind, margin, zeros)
            if kind == "adaptive_hinge" and K > 1:
                assert bool(R.rank_tied_first(s)[0])
            for pattern in R.RANK_MASKS:
                mask = R.rank_mask(B, pattern)
                r = R.rank_ref(s, kind, margin, mask, "sum")
                for form, pd, nd in forms:
                    where = f"rank {kind} m={margin} {R.dt_tag(dtype)} B{B} K{K} mask={pattern} {form}:"
                    md = _dev_mask(mask, dev)
                    loss, denom = F_.rank_loss_forward_raw(pd, nd, kind, margin, md, "sum")
                    d.check(where, "sum loss", loss, r.loss)
                    d.check(where, "sum denom", denom, torch.tensor(1.0, dtype=F64))
                    gp, gn = F_.rank_loss_backward_raw(pd, nd, kind, margin, md, "sum", None, denom)
                    grad = _grad_of(form, gp, gn)
                    d.check(where, "sum gradient", grad, r.grad)
                    if mask is not None and not bool(mask.all()):
                        dropped = grad[~md]
                        d.check(where, "gradient rows of the dropped samples", dropped, torch.zeros(dropped.shape, dtype=F64))
                    for red in ("sample", "mean"):
                        div = R.rank_divisor(kind, K, r.kept, red)
                        loss, denom = F_.rank_loss_forward_raw(pd, nd, kind, margin, md, red)
                        d.check(where, f"{red} denom", denom, torch.tensor(float(div), dtype=F64))
                        d.check(where, f"{red} loss (float64 quotient rounded once)", loss, r.loss / div)
    torch.cuda.synchronize()
    d.done()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dt_tag)
@pytest.mark.parametrize("case", R.RANK_POW2_SIZES, ids=R.rank_id)
def test_hinge_power_of_two_means_exact(dev, case, dtype):
    """masks that keep 2**j samples with K in {1, 2, 4}: every divisor is a power of two, so loss and gradients of the
    two mean reductions are exact through F_.rank_loss and autograd, for output gradients 1, 0.5 and 2"""
    from torecsys_amd import functional as F_
    B, K = case
    s = R.rank_scores(B, K)
    forms = _forms(s, dtype, dev)
    d = R.Diffs()
    for kind in R.RANK_EXACT_KINDS:
        for margin in R.RANK_MARGINS:
            for j, gout in zip((1, 5, 8), R.RANK_GOUTS):
                mask = R.rank_pow2_mask(B, j)
                for red in ("mean", "sample"):
                    r = R.rank_ref(s, kind, margin, mask, red, gout)
                    div = R.rank_divisor(kind, K, r.kept, red)
                    assert div & (div - 1) == 0 and r.kept == 1 << j
                    for form, pd, nd in forms:
                        where = f"rank {kind} m={margin} {R.dt_tag(dtype)} B{B} K{K} keep 2**{j} {red} gout {gout} {form}:"
                        pd = pd.clone().requires_grad_()
                        nd = None if nd is None else nd.clone().requires_grad_()
                        loss = F_.rank_loss(pd, nd, kind, margin, mask.to(dev), red)
                        (loss * gout).backward()
                        d.check(where, "loss", loss.detach(), r.loss)
                        grad = _grad_of(form, pd.grad, None if nd is None else nd.grad)
                        d.check(where, "gradient", grad, r.grad)
                        dropped = grad[~mask.to(dev)]
                        d.check(where, "gradient rows of the dropped samples", dropped, torch.zeros(dropped.shape, dtype=F64))
    torch.cuda.synchronize()
    d.done()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dt_tag)
@pytest.mark.parametrize("case", R.RANK_SIZES, ids=R.rank_id)
def test_smooth_kinds_at_the_same_sizes(dev, case, dtype):
    """pointwise and bpr: sum_err of the loss against float64 <= 1e-5 (all terms >= 0: the sum of magnitudes IS the sum),
    rel_err of the gradients <= 1e-5 (fp32) / 1e-2 (bf16)"""
    from torecsys_amd import functional as F_
    B, K = case
    s = R.rank_scores(B, K)
    forms = _forms(s, dtype, dev)
    worst = [0.0, 0.0]
    for kind in R.RANK_SMOOTH_KINDS:
        for pattern in ("none", "drop_block"):
            mask = R.rank_mask(B, pattern)
            for red in ("sum", "mean"):
                r = R.rank_ref(s, kind, 1.0, mask, red)
                for form, pd, nd in forms:
                    md = _dev_mask(mask, dev)
                    loss, denom = F_.rank_loss_forward_raw(pd, nd, kind, 1.0, md, red)
                    gp, gn = F_.rank_loss_backward_raw(pd, nd, kind, 1.0, md, red, None, denom)
                    e_loss = sum_err(loss.cpu(), r.loss, r.loss)
                    e_grad = rel_err(_grad_of(form, gp, gn).float().cpu(), r.grad)
                    worst = [max(worst[0], e_loss), max(worst[1], e_grad)]
                    assert e_loss <= 1e-5 and e_grad <= TOL[dtype], (kind, pattern, red, form, e_loss, e_grad)
    print(f"rank smooth {R.dt_tag(dtype)} B{B} K{K}: worst sum_err {worst[0]:.2e}, worst gradient rel_err {worst[1]:.2e}")

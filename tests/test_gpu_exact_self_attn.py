"""The MFMA path of csrc/self_attn.hip on operands for which bf16 rounding and fp32 summation are exact
(tests/exact_attn_ref.py, premise asserted by tests/test_exact_attn_host.py): Y, dX, dWin, dWout and both bias gradients
must equal the float64 result bit for bit after the one rounding to bf16.  A missing, doubled or misplaced term -- a tile
edge, a k-step, a head offset, a slab left out of the reduction -- changes them."""
import pytest
import torch

from exact_attn_ref import EXACT_ATTN_CASES, attn_tag, make_case, reference
from exact_ref import expect, mismatch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", EXACT_ATTN_CASES, ids=attn_tag)
def test_self_attn_mfma_is_exact(case):
    from torecsys_amd import functional as F_
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    c = make_case(*case)
    want, _ = reference(c)
    assert F_.self_attn_path(c.L, c.E, c.H, torch.bfloat16) == 2
    x, w_in, b_in, w_out, b_out = (t.to(torch.bfloat16).to(dev).requires_grad_()
                                   for t in (c.x, c.w_in, c.b_in, c.w_out, c.b_out))
    y = F_.self_attn_residual(x, w_in, b_in, w_out, b_out, c.H)
    y.backward(c.gout.to(torch.bfloat16).to(dev))
    got = dict(y=y.detach(), dx=x.grad, dw_in=w_in.grad, db_in=b_in.grad, dw_out=w_out.grad, db_out=b_out.grad)
    bad = [m for m in (mismatch(k, got[k], expect(want[k], torch.bfloat16)) for k in want) if m]
    assert not bad, "\n".join(bad)

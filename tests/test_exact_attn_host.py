"""The premise of tests/test_gpu_exact_self_attn.py, asserted in float64 on the host: in every case of
exact_attn_ref.EXACT_ATTN_CASES each tensor the MFMA path of csrc/self_attn.hip rounds to bf16 survives the rounding, and
each fp32 accumulation is exact whatever its order."""
import pytest
import torch

from exact_attn_ref import EXACT_ATTN_CASES, attn_tag, make_case, reference
from exact_ref import F64

QUANTUM = 2.0 ** -14          # 1 / (4 L**2) at L = 64: every value of every case is a multiple of it


def _bf16_exact(name, t):
    back = t.to(torch.bfloat16).to(F64)
    assert torch.equal(back, t), f"{name}: {int((back != t).sum())} values change in a bf16 round trip"


def _sum_exact(name, terms_abs_sum, quantum=QUANTUM):
    """a sum of multiples of ``quantum`` whose magnitudes add up to less than 2**24 quanta is exact in fp32 in any order"""
    assert float(terms_abs_sum.max()) / quantum < 2 ** 24, name


@pytest.mark.parametrize("case", EXACT_ATTN_CASES, ids=attn_tag)
def test_exact_domain(case):
    c = make_case(*case)
    out, mid = reference(c)
    B, L, E, H = c.B, c.L, c.E, c.H
    d = E // H
    assert d == 16
    assert float(mid["qkv"][..., :E].abs().max()) == 0.0                    # Q = 0: every score is 0
    assert torch.equal(mid["P"], torch.full_like(mid["P"], 1.0 / L))
    assert float(mid["dK"].abs().max()) == 0.0
    for name, t in mid.items():
        assert torch.equal((t / QUANTUM).round() * QUANTUM, t), f"{name}: not a multiple of 2**-14"
        _bf16_exact(name, t)
    for name, t in out.items():
        assert torch.equal(t.float().double(), t), f"{name}: not an fp32 value"
    # the products, by the sums of the magnitudes of their terms
    X, G, O, dO = c.x.abs(), c.gout.abs(), mid["O"].abs(), mid["dO"].abs()
    qkv = mid["qkv"].abs()
    K, V = (qkv[..., i * E:(i + 1) * E].reshape(B, L, H, d).transpose(1, 2) for i in (1, 2))
    P, dS, dQ, dV = mid["P"].abs(), mid["dS"].abs(), mid["dQ"].abs(), mid["dV"].abs()
    dqkv = torch.cat([t.transpose(1, 2).reshape(B, L, E) for t in (dQ, mid["dK"].abs(), dV)], dim=-1)
    _sum_exact("qkv", X @ c.w_in.abs().t() + c.b_in.abs(), 1.0)
    _sum_exact("O", P @ V, 1.0 / L)
    _sum_exact("y", X + O @ c.w_out.abs().t() + c.b_out.abs(), 1.0 / L)
    _sum_exact("dO", G @ c.w_out.abs(), 1.0)
    _sum_exact("dP", dO.reshape(B, L, H, d).transpose(1, 2) @ V.transpose(-1, -2), 1.0)
    _sum_exact("dV", P.transpose(-1, -2) @ dO.reshape(B, L, H, d).transpose(1, 2), 1.0 / L)
    _sum_exact("dQ", dS @ K)
    _sum_exact("dx", G + dqkv @ c.w_in.abs())
    _sum_exact("dw_in", torch.einsum("bli,blj->ij", dqkv, X))            # over the list AND the batch (the slabs)
    _sum_exact("dw_out", torch.einsum("bli,blj->ij", G, O), 1.0 / L)
    _sum_exact("db_in", dqkv.sum((0, 1)))
    _sum_exact("db_out", G.sum((0, 1)), 1.0)
    # what the case is there to show
    assert float(out["dw_in"][:E].abs().max()) > 0, "the query rows of dWin must not be zero"
    assert float(out["dw_in"][E:2 * E].abs().max()) == 0.0 and float(out["db_in"][E:2 * E].abs().max()) == 0.0
    for k in ("y", "dx", "dw_out", "db_out"):
        assert float(out[k].abs().max()) > 0, k
    assert float(out["db_in"][:E].abs().max()) > 0 and float(out["db_in"][2 * E:].abs().max()) > 0

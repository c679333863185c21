"""Float64 restatement of the row-wise Adagrad sink of csrc/scatter.hip (sink_vec, RW) -- a test helper, not product code.

    s[r]   += mean_e(G[r,e]^2)
    w[r,e] -= lr * G[r,e] / (sqrt(s[r]) + eps)          for the looked-up rows; other rows and their s untouched
"""
import math

import torch

import scatter_ref as R

U32 = R.U32


def gamma(n):
    """n roundings of relative size u compounded: (1 + u)^n - 1 <= n*u / (1 - n*u)"""
    return n * U32 / (1.0 - n * U32)


def sum_depth(E, ve):
    """adds a square passes through on its way into the row's sum: the lane's left-to-right chain over its ``ve`` values
    (at most ve - 1) and one per butterfly step over the L = E / ve lanes of the row (log2 L).  E = 1 (the element walk,
    where the rule is element-wise Adagrad): the single square is the sum"""
    if E == 1:
        return 0
    L = E // ve
    assert L * ve == E and L & (L - 1) == 0 and 1 <= L <= 64, (E, ve)
    return (ve - 1) + int(math.log2(L))


def rowwise_adagrad_step(w, s, G, touched, lr, eps, ve=None):
    """One step from (w, s) with the exact row gradients G (V,E) float64; ``touched`` (V,) bool; ``s`` (V,).
    Returns (w', s', tol_w, tol_s), float64, w' / tol_w (V,E) and s' / tol_s (V,).  ``ve``: values per 16-byte vector of
    the table (4 fp32, 8 bf16); taken from ``w.dtype`` when not given.

    The bounds count the fp32 roundings of the kernel as written, u = 2**-24 each (``gamma(n)`` compounds n of them):

      state   E squares, one rounding each; every square then passes through at most D = (ve - 1) + log2(L) adds (the
              lane's chain, then the butterfly of the L = E / ve lanes); one scale by 1/E (a power of two: exact, counted
              all the same); all terms are non-negative, so the relative errors do not amplify:
                  m_hat = m (1 + d1),  |d1| <= gamma(D + 2),    m = mean_e(G^2)
              and one add,  s_hat = (s + m_hat)(1 + d2), |d2| <= u:
                  |s_hat - s'| <= gamma(D + 2) * m + u * (s + m (1 + gamma(D + 2)))          = tol_s
      weight  den = sqrt(s_hat) + eps: root and sum, one rounding each, on non-negative terms; the root halves the
              relative error s_hat inherits, at most gamma(D + 3) / 2.  d = lr * G / den: product and quotient.
              w' = w - d: the difference, relative to the result.  With X = max(|w|, |d|, |w'|) the largest operand:
                  |w_hat - w'| <= (gamma(4) + gamma(D + 3) / 2) (1 + gamma(4)) * |d|  +  u * (|w'| + that)
                               <= (gamma(5) + gamma(D + 3) / 2) (1 + gamma(5)) * X                = tol_w
      bf16    the caller adds scatter_ref.bf16_half_ulp(w') for the final store.
    lr and eps are taken as the fp32 values the kernel receives (scatter_ref.as_f32)."""
    if ve is None:
        ve = 8 if w.dtype == torch.bfloat16 else 4
    E = G.shape[1]
    D = sum_depth(E, ve)
    w, s, G = w.double(), s.double().reshape(-1), G.double()
    t = touched.reshape(-1)
    m = (G * G).mean(1)
    s2 = s + m
    den = (s2.sqrt() + eps).view(-1, 1)
    d = lr * G / den
    w2 = w - d
    g2 = gamma(D + 2)
    tol_s = g2 * m + U32 * (s + m * (1.0 + g2))
    X = torch.maximum(torch.maximum(w.abs(), d.abs()), w2.abs())
    tol_w = (gamma(5) + gamma(D + 3) / 2.0) * (1.0 + gamma(5)) * X
    zs, zw = torch.zeros_like(s), torch.zeros_like(w)
    tw = t.view(-1, 1)
    return torch.where(tw, w2, w), torch.where(t, s2, s), torch.where(tw, tol_w, zw), torch.where(t, tol_s, zs)

"""Plain torch restatements (CPU) of ListIndicesEmbedding(use_attn=True) followed by a sum / mean over the list, which the
attention-pooling tests compare against:

``mha_compose``  -- the composition itself: ``F.embedding -> nn.MultiheadAttention -> pool`` through ``list_ref.compose``;
``collapsed``    -- the algebra csrc/attn_pool.hip relies on.  Per sample and head (d = E / H, X the (L, E) rows):
    Q = X Wq^T + bq,  K = X Wk^T + bk,  P = softmax_rows(Q_h K_h^T / sqrt(d))
    pbar_h[m] = c sum_l P[l, m]              c  = 1 / L (mean) or 1 (sum)
    xt_h      = sum_m pbar_h[m] X[m, :]      (what the kernel emits, (B, H, E))
    o_h       = xt_h Wv_h^T + c' bv_h        c' = sum_m pbar_h[m] = 1 (mean) or L (sum)
    y         = concat_h(o_h) Wout^T + c' bout
  because sum_l (P V)[l] = (sum_l P[l, :]) V and V = X Wv^T + bv is linear in X.
tests/test_list_attn_host.py pins both to the reference's own outputs and gradients (tests/golden/list_attn.npz)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from list_ref import compose

ATTN_KEYS = ["attention.in_proj_weight", "attention.in_proj_bias", "attention.out_proj.weight", "attention.out_proj.bias"]
# (B, L, E, V, H, bias) of list_attn.npz
ATTN_SHAPES = [(6, 5, 16, 12, 2, True), (5, 7, 64, 20, 4, True), (4, 1, 8, 9, 1, True), (7, 33, 32, 40, 1, False),
               (6, 4, 10, 7, 5, True)]
POOL = {"avg_pooling": "mean", "mean": "mean", "sum": "sum"}


def attn_tag(s):
    return "%d_%d_%d_%d_h%d_b%d" % (s[0], s[1], s[2], s[3], s[4], int(s[5]))


def make_attention(E, H, bias=True, params=None, generator=None):
    """nn.MultiheadAttention(E, H) on the CPU; ``params``: {in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias}
    to load, else (with ``generator``) weights ~ N(0, 1 / E) and biases ~ N(0, 0.1): no term of a gradient is zero by
    initialisation, and the scores stay of order one at every E"""
    a = nn.MultiheadAttention(embed_dim=E, num_heads=H, bias=bias)
    if params is not None:
        a.load_state_dict({k: v.detach().float() for k, v in params.items()})
    elif generator is not None:
        with torch.no_grad():
            for k, p in a.named_parameters():
                p.copy_(torch.randn(p.shape, generator=generator) * (0.1 if k.endswith("bias") else E ** -0.5))
    return a


def attention_params(a):
    return {k: p for k, p in a.named_parameters()}


def mha_compose(weight, idx, attention, mode, padding_idx=None):
    """(B, 1, E): embedding -> attention(seq, seq, seq) on (L, B, E) -> sum / mean over L"""
    return compose(weight, idx, mode, padding_idx=padding_idx, attention=attention)


def collapsed(weight, idx, in_w, in_b, out_w, out_b, H, mode, padding_idx=None):
    """(B, 1, E) by the collapsed formula; every argument may require grad"""
    X = F.embedding(idx.long(), weight, padding_idx=padding_idx)                      # (B, L, E)
    B, L, E = X.shape
    d = E // H
    qk = X @ in_w[:2 * E].t()
    if in_b is not None:
        qk = qk + in_b[:2 * E]
    q = qk[..., :E].reshape(B, L, H, d).transpose(1, 2)                               # (B, H, L, d)
    k = qk[..., E:].reshape(B, L, H, d).transpose(1, 2)
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), dim=-1)                 # (B, H, L, L)
    c, cb = (1.0 / L, 1.0) if mode == "mean" else (1.0, float(L))
    pbar = c * P.sum(dim=2)                                                           # (B, H, L): summed over the rows l
    xt = torch.einsum("bhm,bme->bhe", pbar, X)
    o = torch.einsum("bhe,hde->bhd", xt, in_w[2 * E:].reshape(H, d, E)).reshape(B, E)
    if in_b is not None:
        o = o + cb * in_b[2 * E:]
    y = o @ out_w.t()
    if out_b is not None:
        y = y + cb * out_b
    return y.unsqueeze(1)


def collapsed_with(weight, idx, attention, mode, padding_idx=None):
    a = attention
    return collapsed(weight, idx, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, a.num_heads, mode,
                     padding_idx)


def reference_grads(fn, w, attention, gout):
    """outputs and the gradients of the table and of the attention parameters of ``fn(w, attention)`` for ``gout``"""
    w = w.detach().clone().requires_grad_()
    for p in attention.parameters():
        p.grad = None
    y = fn(w, attention)
    (y * gout).sum().backward()
    grads = {"embedding.weight": w.grad}
    grads.update({"attention." + k: p.grad for k, p in attention.named_parameters()})
    return y.detach(), grads

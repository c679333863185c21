"""CPU restatement of functional.bag_pool(exclude_padding=, per_sample_weights=) with hand-written gradients, in whatever
dtype the table has (the tests use fp64): what nn.EmbeddingBag computes for 2-D ids with ``padding_idx`` and
``per_sample_weights``, plus the one case it does not have -- the weighted sum WITHOUT exclusion, which is
``(F.embedding(idx, w) * psw[..., None]).sum(1)``.  tests/test_bag_masked_host.py pins it to
torch.nn.functional.embedding_bag + autograd; the GPU tests use it because it also takes an out-of-range id (a zero row
that still counts as live) and returns the dense table gradient with the padding row zeroed."""
import torch
import torch.nn.functional as F


def masked_bag(w, idx, mode, pad=None, exclude=False, psw=None, gout=None):
    """w (V, E), idx (B, L) int, pad: resolved padding row or None, psw (B, L) or None, gout (B, E) or None.
    Returns (out (B, E), grad_w (V, E) or None, dw (B, L) or None)."""
    V, E = w.shape
    B, L = idx.shape
    idx = idx.long()
    inside = (idx >= 0) & (idx < V)
    rows = torch.cat([w, w.new_zeros(1, E)])[torch.where(inside, idx, torch.full_like(idx, V))]      # (B, L, E)
    live = (idx != pad) if exclude else torch.ones_like(inside)
    cnt = live.sum(1)
    coef = live.to(w.dtype) if psw is None else live.to(w.dtype) * psw
    amax = None
    if mode == "max":
        masked = rows.masked_fill(~live.unsqueeze(-1), float("-inf"))
        out = masked.max(dim=1)[0]
        pos = torch.arange(L).view(1, L, 1).expand(B, L, E)
        amax = torch.where(masked == out.unsqueeze(1), pos, torch.full_like(pos, L)).min(dim=1)[0]      # the FIRST one
        out = torch.where((cnt > 0).unsqueeze(1), out, torch.zeros_like(out))
    else:
        out = (rows * coef.unsqueeze(-1)).sum(1)
        if mode == "mean":
            scale = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1).to(w.dtype), torch.zeros(B, dtype=w.dtype))
            out = out * scale.unsqueeze(1)
    if gout is None:
        return out, None, None
    # d out[b, e] / d rows[b, l, e]
    if mode == "max":
        d = (torch.arange(L).view(1, L, 1) == amax.unsqueeze(1)).to(w.dtype) * (cnt > 0).view(B, 1, 1).to(w.dtype)
    else:
        d = coef.unsqueeze(-1).expand(B, L, E)
        if mode == "mean":
            d = d * scale.view(B, 1, 1)
    g_rows = d * gout.unsqueeze(1)                                                             # (B, L, E)
    grad = w.new_zeros(V + 1, E).index_add_(0, torch.where(inside, idx, torch.full_like(idx, V)).reshape(-1),
                                            g_rows.reshape(B * L, E))[:V]
    if pad is not None:
        grad[pad] = 0
    dw = None
    if psw is not None:
        dw = (rows * gout.unsqueeze(1)).sum(-1) * live.to(w.dtype)
    return out, grad, dw


def embedding_bag_ref(w, idx, mode, pad, psw=None, gout=None):
    """torch's own: F.embedding_bag on the CPU with 2-D ids (padding excluded) and autograd.  ``pad=None`` with weights is
    the composition (F.embedding(idx, w) * psw[..., None]).sum(1)."""
    w = w.detach().clone().requires_grad_()
    p = psw.detach().clone().requires_grad_() if psw is not None else None
    if pad is None:
        assert mode == "sum" and p is not None
        out = (F.embedding(idx.long(), w) * p.unsqueeze(-1)).sum(1)
    else:
        out = F.embedding_bag(idx.long(), w, mode=mode, padding_idx=pad, per_sample_weights=p)
    if gout is None:
        return out.detach(), None, None
    out.backward(gout)
    return out.detach(), w.grad, (p.grad if p is not None else None)

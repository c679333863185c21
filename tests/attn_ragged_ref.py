"""fp64 restatement (CPU) of functional.attn_pool_ragged / attn_pool_ragged_layer: per bag, the collapsed algebra of
tests/list_attn_ref.py on the bag's OWN rows.  Bag b holds ids[beg_b:end_b) (bounds clamped as the kernel clamps them:
bag_ragged_ref.bag_bounds); with ``exclude`` the ids equal to ``pad`` are removed; the first ``max_length`` live ids are
taken, L_b of them; X the (L_b, E) rows (an id outside the table: a zero row that takes part), c = 1 / L_b (mean) or 1:
    P_h = softmax_rows(Q_h K_h^T / sqrt(d))     pbar_h[m] = c sum_l P_h[l, m]     xt_h = sum_m pbar_h[m] X[m]
    y   = concat_h(xt_h Wv_h^T + c' bv_h) Wout^T + c' bout        c' = L_b (sum) or [L_b > 0] (mean)
An empty bag is a zero row.  Gradients come from autograd on these formulas; ``dx`` (n, E) is the gradient of every
position's row -- zero where the position is excluded, not taken or in no bag -- and the table gradient is its sum per
row with the padding row zeroed.  tests/test_attn_ragged_host.py pins this to a per-bag nn.MultiheadAttention loop."""
import math

import torch

from bag_ragged_ref import bag_bounds


def live_positions(ids, offsets, max_length, pad=None, exclude=False, include_last_offset=False):
    """per bag: the flat positions it takes (at most ``max_length``), and whether it held more live ids than that"""
    ids = ids.long().reshape(-1)
    taken, over = [], []
    for beg, end in bag_bounds(offsets, ids.numel(), include_last_offset):
        pos = [p for p in range(beg, end) if not (exclude and int(ids[p]) == pad)]
        over.append(len(pos) > max_length)
        taken.append(pos[:max_length])
    return taken, over


def ragged_attn(w, ids, offsets, in_w, in_b, out_w, out_b, H, mode, max_length, pad=None, exclude=False,
                include_last_offset=False, gout=None, gxt=None):
    """w (V, E) and the four attention parameters in one float dtype (the tests use fp64); ``pad``: the resolved padding
    row or None.  ``gout`` (B, 1, E): gradient of the layer output y; ``gxt`` (B, H, E): gradient of xt instead (the
    kernel's own output).  Returns a dict: y (B, 1, E), xt (B, H, E), cnt (B,), over (bags beyond max_length) and, with a
    gradient, dx (n, E), embedding.weight (V, E) and attention.* for the four parameters (None without a bias)."""
    V, E = w.shape
    d = E // H
    ids = ids.long().reshape(-1)
    n = ids.numel()
    taken, over = live_positions(ids, offsets, max_length, pad, exclude, include_last_offset)
    B = len(taken)
    leaves = {"w": w, "in_w": in_w, "in_b": in_b, "out_w": out_w, "out_b": out_b}
    leaves = {k: (t.detach().clone().requires_grad_() if t is not None else None) for k, t in leaves.items()}
    wl, iw, ib, ow, ob = (leaves[k] for k in ("w", "in_w", "in_b", "out_w", "out_b"))
    inside = (ids >= 0) & (ids < V)
    rows = torch.where(inside.unsqueeze(1), wl[ids.clamp(0, V - 1)], wl.new_zeros(1, E)) if n else wl.new_zeros(0, E)
    rows.retain_grad()
    xts, ys = [], []
    for pos in taken:
        L = len(pos)
        if L == 0:
            xts.append(wl.new_zeros(H, E))
            ys.append(wl.new_zeros(E))
            continue
        X = rows[torch.tensor(pos)]                                                      # (L, E)
        qk = X @ iw[:2 * E].t()
        if ib is not None:
            qk = qk + ib[:2 * E]
        q = qk[:, :E].reshape(L, H, d).transpose(0, 1)                                   # (H, L, d)
        k = qk[:, E:].reshape(L, H, d).transpose(0, 1)
        P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), dim=-1)                # (H, L, L)
        c, cb = (1.0 / L, 1.0) if mode == "mean" else (1.0, float(L))
        xt = (c * P.sum(dim=1)) @ X                                                      # (H, E)
        o = torch.einsum("he,hde->hd", xt, iw[2 * E:].reshape(H, d, E)).reshape(E)
        if ib is not None:
            o = o + cb * ib[2 * E:]
        y = o @ ow.t()
        if ob is not None:
            y = y + cb * ob
        xts.append(xt)
        ys.append(y)
    xt = torch.stack(xts) if B else wl.new_zeros(0, H, E)
    y = torch.stack(ys).unsqueeze(1) if B else wl.new_zeros(0, 1, E)
    res = {"y": y.detach(), "xt": xt.detach(), "cnt": torch.tensor([float(len(p)) for p in taken]), "over": over}
    if gout is None and gxt is None:
        return res
    loss = (y * gout.to(y.dtype)).sum() if gout is not None else (xt * gxt.to(xt.dtype)).sum()
    if loss.requires_grad and any(len(p) for p in taken):
        loss.backward()

    def grad_of(t):
        return None if t is None else (t.grad if t.grad is not None else torch.zeros_like(t))

    res["dx"] = grad_of(rows)
    gw = grad_of(wl).clone()
    if pad is not None:
        gw[pad] = 0
    res["embedding.weight"] = gw
    res["attention.in_proj_weight"], res["attention.in_proj_bias"] = grad_of(iw), grad_of(ib)
    res["attention.out_proj.weight"], res["attention.out_proj.bias"] = grad_of(ow), grad_of(ob)
    return res


def ragged_attn_with(w, ids, offsets, attention, mode, max_length, **kw):
    """the same with the parameters of an nn.MultiheadAttention, converted to the table's dtype"""
    a = attention
    cast = lambda t: None if t is None else t.detach().to(w.dtype)                       # noqa: E731
    return ragged_attn(w, ids, offsets, cast(a.in_proj_weight), cast(a.in_proj_bias), cast(a.out_proj.weight),
                       cast(a.out_proj.bias), a.num_heads, mode, max_length, **kw)


def mha_loop(w, ids, offsets, attention, mode, max_length, pad=None, exclude=False, include_last_offset=False, gout=None):
    """nn.MultiheadAttention over every bag's own rows, then sum / mean -- one call per bag, autograd for the gradients.
    Returns (y (B, 1, E), {embedding.weight, attention.*}); ``attention`` must have the table's dtype."""
    V, E = w.shape
    ids = ids.long().reshape(-1)
    taken, _ = live_positions(ids, offsets, max_length, pad, exclude, include_last_offset)
    wl = w.detach().clone().requires_grad_()
    for p in attention.parameters():
        p.grad = None
    ys = []
    for pos in taken:
        if not pos:
            ys.append(wl.new_zeros(1, E))
            continue
        seq = wl[ids[torch.tensor(pos)]].unsqueeze(1)                                    # (L, 1, E)
        o, _ = attention(seq, seq, seq)
        ys.append(o.mean(dim=0) if mode == "mean" else o.sum(dim=0))
    y = torch.stack(ys)
    grads = None
    if gout is not None:
        (y * gout).sum().backward()
        gw = wl.grad.clone()
        if pad is not None:
            gw[pad] = 0
        grads = {"embedding.weight": gw}
        grads.update({"attention." + k: p.grad for k, p in attention.named_parameters()})
    return y.detach(), grads


def pad_to(ids, offsets, L, pad, include_last_offset=False):
    """the bags as a (B, L) list padded with ``pad`` (every bag must fit), and the (B, L) key-padding mask (True = padding)"""
    ids = ids.long().reshape(-1)
    bounds = bag_bounds(offsets, ids.numel(), include_last_offset)
    idx = torch.full((len(bounds), L), pad, dtype=torch.int64)
    mask = torch.ones(len(bounds), L, dtype=torch.bool)
    for i, (b, e) in enumerate(bounds):
        idx[i, :e - b] = ids[b:e]
        mask[i, :e - b] = False
    return idx, mask


def parity_lengths(g, B=97, cap=64):
    """every boundary of the 16-wide tiles and of the cap in one batch, an empty first bag, then random lengths <= cap in
    an order that alternates long and short (a short bag follows a long one in the same workgroup's LDS)"""
    fixed = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64]
    rest = B - len(fixed)
    long_ = torch.randint(cap // 2, cap + 1, (rest,), generator=g).tolist()
    short = torch.randint(0, 6, (rest,), generator=g).tolist()
    return fixed + [long_[i] if i % 2 == 0 else short[i] for i in range(rest)]

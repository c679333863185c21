"""CPU restatement of functional.bag_pool_ragged with hand-written gradients, in whatever dtype the table has (the tests
use fp64): what torch.nn.functional.embedding_bag(ids, w, offsets, ...) computes for 1-D ids -- sum / mean / max, with
``padding_idx`` exclusion, ``per_sample_weights`` and ``include_last_offset`` -- plus what it does not serve: a live id
outside the table (a zero row that still counts), the weighted sum without a padding row being excluded, offsets that are
out of range or decrease (clamped to [0, n]; a bag whose end lies before its begin is empty), and the dense table gradient
with the padding row zeroed.  tests/test_bag_ragged_host.py pins it to F.embedding_bag + autograd."""
import torch
import torch.nn.functional as F


def bag_bounds(offsets, n, include_last_offset=False):
    """[(begin, end)] of every bag, clamped to [0, n] as the kernel clamps them"""
    off = [int(o) for o in offsets.tolist()]
    B = len(off) - 1 if include_last_offset else len(off)
    out = []
    for b in range(B):
        beg = off[b]
        end = off[b + 1] if b + 1 < len(off) else n
        beg, end = min(max(beg, 0), n), min(max(end, 0), n)
        out.append((beg, max(beg, end)))
    return out


def bag_owner(offsets, n, include_last_offset=False):
    """bag_of (n,): the last b with offsets[b] <= p, provided p < end_b; else -1 (torch.bucketize-style arithmetic, for
    offsets that do not decrease)"""
    off = offsets.long()
    B = off.numel() - 1 if include_last_offset else off.numel()
    p = torch.arange(n)
    if B == 0:
        return torch.full((n,), -1, dtype=torch.int64)
    b = torch.bucketize(p, off[:B], right=True) - 1                 # the number of offsets <= p, minus one
    end = torch.cat([off[1:], torch.tensor([n])])[:B] if not include_last_offset else off[1:B + 1]
    ok = (b >= 0) & (p < end[b.clamp_min(0)])
    return torch.where(ok, b, torch.full_like(b, -1))


def ragged_bag(w, ids, offsets, mode, pad=None, exclude=False, psw=None, gout=None, include_last_offset=False):
    """w (V, E), ids (n,) int, offsets int, pad: resolved padding row or None, psw (n,) or None, gout (B, E) or None.
    Returns (out (B, E), grad_w (V, E) or None, dw (n,) or None); the max gives its gradient to the FIRST of equal rows."""
    V, E = w.shape
    ids = ids.long().reshape(-1)
    n = ids.numel()
    bounds = bag_bounds(offsets, n, include_last_offset)
    B = len(bounds)
    out = w.new_zeros(B, E)
    grad = w.new_zeros(V, E) if gout is not None else None
    dw = w.new_zeros(n) if (gout is not None and psw is not None) else None
    for b, (beg, end) in enumerate(bounds):
        pos = [p for p in range(beg, end) if not (exclude and int(ids[p]) == pad)]
        if not pos:
            continue
        pos_t = torch.tensor(pos)
        r = ids[pos_t]
        inside = (r >= 0) & (r < V)
        rows = torch.where(inside.unsqueeze(1), w[r.clamp(0, V - 1)], w.new_zeros(1, E))      # (len, E)
        if mode == "max":
            out[b] = rows.max(dim=0)[0]
            hit = rows == out[b].unsqueeze(0)
            first = torch.where(hit, torch.arange(len(pos)).unsqueeze(1), torch.tensor(len(pos))).min(dim=0)[0]
            d = (torch.arange(len(pos)).unsqueeze(1) == first.unsqueeze(0)).to(w.dtype)            # (len, E)
        else:
            coef = torch.ones(len(pos), dtype=w.dtype) if psw is None else psw[pos_t].to(w.dtype)
            out[b] = (rows * coef.unsqueeze(1)).sum(0)
            if mode == "mean":
                out[b] = out[b] / len(pos)
                coef = coef / len(pos)
            d = coef.unsqueeze(1).expand(len(pos), E)
        if gout is not None:
            g_rows = d * gout[b].unsqueeze(0)
            grad.index_add_(0, r[inside], g_rows[inside])
            if dw is not None:
                dw[pos_t] = (rows * gout[b].unsqueeze(0)).sum(1)
    if grad is not None and pad is not None:
        grad[pad] = 0
    return out, grad, dw


def embedding_bag_ref(w, ids, offsets, mode, pad=None, psw=None, gout=None, include_last_offset=False):
    """torch's own: F.embedding_bag on the CPU with 1-D ids and offsets, and autograd"""
    w = w.detach().clone().requires_grad_()
    p = psw.detach().clone().requires_grad_() if psw is not None else None
    out = F.embedding_bag(ids.long().reshape(-1), w, offsets.long(), mode=mode, padding_idx=pad, per_sample_weights=p,
                          include_last_offset=include_last_offset)
    if gout is None:
        return out.detach(), None, None
    out.backward(gout)
    return out.detach(), w.grad, (p.grad if p is not None else None)


def pad_bags(ids, offsets, pad, include_last_offset=False, psw=None):
    """the same bags as a (B, L) list padded with ``pad`` to the longest bag (L >= 1), and the weights laid out alike"""
    ids = ids.long().reshape(-1)
    bounds = bag_bounds(offsets, ids.numel(), include_last_offset)
    L = max(1, max((e - b for b, e in bounds), default=1))
    idx = torch.full((len(bounds), L), pad, dtype=torch.int64)
    wts = torch.ones(len(bounds), L, dtype=psw.dtype) if psw is not None else None
    for i, (b, e) in enumerate(bounds):
        idx[i, :e - b] = ids[b:e]
        if psw is not None:
            wts[i, :e - b] = psw[b:e]
    return idx, wts


# ---------------------------------------------------------------------------------------------- shared test batches
def _pow2_floor(c):
    return 0 if c <= 0 else 1 << (int(c).bit_length() - 1)


def bags_from_lengths(g, lengths, V, pad, trailing=0, sprinkle=0.0, all_pad=()):
    """ids (n,) other than ``pad`` in [0, V) for bags of the given lengths plus ``trailing`` ids behind the last bag;
    ``sprinkle``: that share of the positions is set to ``pad``; the bags listed in ``all_pad`` hold nothing else.
    Returns (ids, offsets (B + 1,) int64 -- the last one closes the last bag)."""
    lengths = [int(x) for x in lengths]
    offsets = torch.tensor([0] + lengths).cumsum(0)
    n = int(offsets[-1]) + trailing
    ids = torch.randint(0, V - 1, (n,), generator=g)
    ids = ids + (ids >= pad).long()
    if sprinkle > 0:
        ids[torch.rand(n, generator=g) < sprinkle] = pad
    for b in all_pad:
        ids[int(offsets[b]):int(offsets[b + 1])] = pad
    return ids, offsets


def boundary_lengths(g, T, B=37):
    """every boundary of the forward in one batch: empty first and last fixed bags, the walks' 4 and 8 rows in flight, both
    sides of the long-bag threshold T, a bag of several strides of a wave; random lengths <= 12 up to B bags"""
    fixed = [0, 1, 3, 4, 5, 7, 8, 9, T - 1, T, T + 1, 2 * T + 3, 0]
    return fixed + torch.randint(0, 13, (B - len(fixed),), generator=g).tolist()


def pow2_live(ids, offsets, pad):
    """the same bags with every live count cut down to a power of two: live positions past it are set to ``pad``"""
    ids = ids.clone()
    for b in range(offsets.numel() - 1):
        seen, keep = 0, _pow2_floor(int((ids[int(offsets[b]):int(offsets[b + 1])] != pad).sum()))
        for p in range(int(offsets[b]), int(offsets[b + 1])):
            if int(ids[p]) != pad:
                seen += 1
                if seen > keep:
                    ids[p] = pad
    return ids


def pow2_lengths(ids, offsets):
    """the same bags cut down to a power-of-two LENGTH (ids past it dropped), for the mean over every position"""
    parts, lens = [], []
    for b in range(offsets.numel() - 1):
        beg, end = int(offsets[b]), int(offsets[b + 1])
        keep = _pow2_floor(end - beg)
        parts.append(ids[beg:beg + keep])
        lens.append(keep)
    parts.append(ids[int(offsets[-1]):])                          # the ids behind the last bag stay
    return torch.cat(parts), torch.tensor([0] + lens).cumsum(0)

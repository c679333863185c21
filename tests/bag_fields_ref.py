"""CPU restatement of functional.bag_pool_fields with hand-written gradients, in whatever dtype the table has (the tests use
fp64): F multi-valued fields over one table of sum(field_sizes) rows, ``values`` (n,) RAW per-field ids, ``offsets``
(F*B + 1,) field-major -- bag j = f*B + b is values[offsets[j]:offsets[j+1]] -- pooled to out[b, f].  Field f is
bag_ragged_ref.ragged_bag on the field's table slice, the whole values vector and the field's B + 1 offsets (absolute, the
last one closing the field's last bag): an id outside [0, field_sizes[f]) is then a zero row that still counts, and offsets
out of range or decreasing are clamped as the kernel clamps them.  tests/test_bag_fields_host.py pins it to
F.embedding_bag + autograd per field.  Below: the batches the host and the GPU tests share."""
import torch
import torch.nn.functional as F

from bag_ragged_ref import pow2_lengths, ragged_bag


def field_starts(field_sizes):
    """(F + 1,) int64: the exclusive prefix sum of the field sizes"""
    return torch.tensor([0] + [int(s) for s in field_sizes]).cumsum(0)


def fields_bag(w, values, offsets, field_sizes, mode, psw=None, gout=None):
    """w (V, E), values (n,), offsets (F*B + 1,), psw (n,) or None, gout (B, F, E) or None.
    Returns (out (B, F, E), grad_w (V, E) or None, dw (n,) or None)."""
    nf = len(field_sizes)
    fo = field_starts(field_sizes)
    assert w.shape[0] == int(fo[-1]) and (offsets.numel() - 1) % nf == 0
    B = (offsets.numel() - 1) // nf
    values = values.long().reshape(-1)
    out = w.new_zeros(B, nf, w.shape[1])
    grad = torch.zeros_like(w) if gout is not None else None
    dw = w.new_zeros(values.numel()) if (gout is not None and psw is not None) else None
    for f in range(nf):
        lo, hi = int(fo[f]), int(fo[f + 1])
        y, g, d = ragged_bag(w[lo:hi], values, offsets[f * B:(f + 1) * B + 1], mode, None, False, psw,
                             None if gout is None else gout[:, f], True)
        out[:, f] = y
        if g is not None:
            grad[lo:hi] = g
        if d is not None:
            dw += d
    return out, grad, dw


def embedding_bag_fields(w, values, offsets, field_sizes, mode, psw=None, gout=None):
    """torch's own, for offsets that do not decrease and ids inside their fields: F.embedding_bag per field on the field's
    table slice, its id slice and its rebased offsets, autograd for the gradients, the results stacked to (B, F, E)"""
    nf = len(field_sizes)
    fo = field_starts(field_sizes)
    B = (offsets.numel() - 1) // nf
    wl = w.detach().clone().requires_grad_()
    pl = psw.detach().clone().requires_grad_() if psw is not None else None
    ys = []
    for f in range(nf):
        off = offsets[f * B:(f + 1) * B + 1].long()
        beg, end = int(off[0]), int(off[-1])
        ys.append(F.embedding_bag(values[beg:end].long(), wl[int(fo[f]):int(fo[f + 1])], off - beg, mode=mode,
                                  per_sample_weights=None if pl is None else pl[beg:end], include_last_offset=True))
    out = torch.stack(ys, dim=1)
    if gout is None:
        return out.detach(), None, None
    out.backward(gout)
    return out.detach(), wl.grad, (pl.grad if pl is not None else None)


# ---------------------------------------------------------------------------------------------- shared test batches
def field_major_lengths(per_field):
    """per_field[f]: the B bag lengths of field f -> offsets (F*B + 1,) int64, field-major"""
    flat = [int(x) for ls in per_field for x in ls]
    return torch.tensor([0] + flat).cumsum(0)


def values_for(g, offsets, field_sizes, trailing=0):
    """random RAW ids inside their own field for every bag, plus ``trailing`` ids (of field 0's range) behind the last
    offset"""
    nf = len(field_sizes)
    B = (offsets.numel() - 1) // nf
    parts = []
    for f in range(nf):
        cnt = int(offsets[(f + 1) * B] - offsets[f * B])
        parts.append(torch.randint(0, int(field_sizes[f]), (cnt,), generator=g))
    parts.append(torch.randint(0, int(field_sizes[0]), (trailing,), generator=g))
    return torch.cat(parts)


def cut_pow2(values, offsets):
    """every bag cut down to a power-of-two LENGTH (bag_ragged_ref.pow2_lengths; the ids behind the last offset stay)"""
    return pow2_lengths(values, offsets)


def one_id_long_bags(g, values, offsets, field_sizes, longer_than=8):
    """the same bags with every bag of more than ``longer_than`` ids holding ONE id (drawn per bag) throughout"""
    nf = len(field_sizes)
    B = (offsets.numel() - 1) // nf
    values = values.clone()
    for j in range(nf * B):
        beg, end = int(offsets[j]), int(offsets[j + 1])
        if end - beg > longer_than:
            values[beg:end] = int(torch.randint(0, int(field_sizes[j // B]), (1,), generator=g))
    return values

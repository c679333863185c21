"""fp64 reference of functional.softmax_scores_loss, over operands that already hold the table dtype's values."""
import torch


def softmax_loss_ref(anchors, targets, labels, scale, g):
    """Returns a dict: z (B, Vt), lse (B), loss (B), keep (B), w (B, Vt) = g (p - onehot), dA (B, E), dT (Vt, E), fp64.
    A label outside [0, Vt) is an ignored sample: loss 0, no gradient."""
    a, t = anchors.double(), targets.double()
    z = scale * (a @ t.T)
    lse = torch.logsumexp(z, dim=1)
    keep = (labels >= 0) & (labels < t.shape[0])
    rows = torch.nonzero(keep).reshape(-1)
    loss = torch.zeros_like(lse)
    loss[rows] = lse[rows] - z[rows, labels[rows]]
    w = torch.exp(z - lse[:, None])
    w[rows, labels[rows]] -= 1.0
    w = w * (g.double() * keep)[:, None]
    return dict(z=z, lse=lse, loss=loss, keep=keep, w=w, dA=scale * (w @ t), dT=scale * (w.T @ a))


def splits(rows_stationary, rows_streamed):
    """the number of ranges the host cuts the streamed rows into (sl_splits of csrc/softmax_loss.hip)"""
    tiles = (rows_stationary + 127) // 128
    if tiles >= 256:
        return 1
    return max(1, min((512 + tiles - 1) // tiles, 64, rows_streamed // 256))

"""fp64 autograd reference of functional.softmax_scores_loss with sim / bias, over operands that already hold the table
dtype's values: scale * (a @ t.T) / (|a|.clamp_min(eps) * |t|.clamp_min(eps)) + bias, logsumexp, autograd."""
import torch

EPS = 1e-8


def softmax_loss_sim_ref(anchors, targets, labels, scale, g, sim, bias):
    """Returns a dict, fp64: s (B, Vt) the similarities, z, lse, loss, keep, w = g (p - onehot), dA, dT, dB, and what the
    bounds need: ra (B), rt (Vt) the inverse clamped norms (ones for 'dot') and pa, pt: 1.0 where the norm is above eps
    (the row has a projection term), else 0.  A label outside [0, Vt) is an ignored sample."""
    a, t = anchors.double().requires_grad_(), targets.double().requires_grad_()
    b = (torch.zeros(t.shape[0]) if bias is None else bias).double().requires_grad_()
    na, nt = torch.linalg.vector_norm(a, dim=1), torch.linalg.vector_norm(t, dim=1)
    cos = sim == 'cosine'
    s = (a @ t.T) / (na.clamp_min(EPS)[:, None] * nt.clamp_min(EPS)[None, :]) if cos else a @ t.T
    z = scale * s + b
    lse = torch.logsumexp(z, dim=1)
    keep = (labels >= 0) & (labels < t.shape[0])
    loss = torch.where(keep, lse - z.gather(1, labels.clamp(0, t.shape[0] - 1)[:, None])[:, 0], torch.zeros_like(lse))
    (loss * g.double()).sum().backward()
    with torch.no_grad():
        w = torch.exp(z - lse[:, None])
        rows = keep.nonzero().reshape(-1)
        w[rows, labels[rows]] -= 1.0
        w = w * (g.double() * keep)[:, None]
        one_a, one_t = torch.ones_like(na), torch.ones_like(nt)
        return dict(s=s.detach(), z=z.detach(), lse=lse.detach(), loss=loss.detach(), keep=keep, w=w, dA=a.grad, dT=t.grad,
                    dB=b.grad, ra=1 / na.clamp_min(EPS) if cos else one_a, rt=1 / nt.clamp_min(EPS) if cos else one_t,
                    pa=(na > EPS).double() if cos else 0 * one_a, pt=(nt > EPS).double() if cos else 0 * one_t)

"""Plain torch restatements (CPU, any float dtype) that the PersonalizedReRankingModel tests compare against:

``block``       -- ``x + nn.MultiheadAttention(x, x, x)`` for a batch-first (B, L, E) block by the per-sample formula
                   csrc/self_attn.hip computes (d = E / H):
    [Q|K|V] = X Win^T + bin          P_h = softmax_rows(Q_h K_h^T / sqrt(d))
    O = concat_h(P_h V_h)            Y = X + O Wout^T + bout
``block_mha``   -- the same through nn.MultiheadAttention on the transposed block, as the reference's forward runs it;
``model``       -- the whole model from a state_dict: position bias, input Linear, per layer
                   block -> BatchNorm1d(L) -> x + ReLU(Linear(x)) -> BatchNorm1d(L), then Linear(E, 1), flatten, softmax
                   over the list.  Batch-norm in training mode (batch statistics over (B, E) per position, biased variance
                   in the normalisation, unbiased in the running update, momentum 0.1); returns the updated statistics.
tests/test_prm_host.py pins all three to the reference's own float64 outputs and gradients (tests/golden/prm.npz)."""
import math

import torch
import torch.nn as nn

# (B, L, embed, E, H, layers) of prm.npz
PRM_SHAPES = [(6, 5, 12, 16, 2, 2), (5, 7, 24, 64, 4, 1), (7, 33, 32, 32, 1, 2), (6, 4, 10, 10, 5, 2)]
MHA_KEYS = ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
OUT_BIAS = "layers.OutputLayer.FeedForward.bias"          # its gradient is zero in exact arithmetic (softmax is shift-invariant)
OUT_WEIGHT = "layers.OutputLayer.FeedForward.weight"


def prm_tag(s):
    return "%d_%d_%d_%d_h%d_l%d" % tuple(s)


def block(x, in_w, in_b, out_w, out_b, H):
    """(B, L, E) by the per-sample formula; every argument may require grad; the biases may be None"""
    B, L, E = x.shape
    d = E // H
    qkv = x @ in_w.t()
    if in_b is not None:
        qkv = qkv + in_b
    q, k, v = (qkv[..., i * E:(i + 1) * E].reshape(B, L, H, d).transpose(1, 2) for i in range(3))      # (B, H, L, d)
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), dim=-1)
    o = (P @ v).transpose(1, 2).reshape(B, L, E)
    y = o @ out_w.t()
    if out_b is not None:
        y = y + out_b
    return x + y


def make_mha(E, H, bias=True, params=None, generator=None, dtype=torch.float32):
    """nn.MultiheadAttention(E, H) on the CPU; ``params`` to load, else (with ``generator``) weights ~ N(0, 1 / E) and
    biases ~ N(0, 0.1), as list_attn_ref.make_attention draws them"""
    a = nn.MultiheadAttention(embed_dim=E, num_heads=H, bias=bias).to(dtype)
    if params is not None:
        a.load_state_dict({k: v.detach().to(dtype) for k, v in params.items()})
    elif generator is not None:
        with torch.no_grad():
            for k, p in a.named_parameters():
                p.copy_(torch.randn(p.shape, generator=generator) * (0.1 if k.endswith("bias") else E ** -0.5))
    return a


def block_mha(x, mha):
    xt = x.transpose(0, 1)
    return x + mha(xt, xt, xt)[0].transpose(0, 1)


def block_grads(fn, x, params, gout):
    """``fn(x, *params)``: the output and the gradients of x and of every entry of ``params`` that is not None"""
    x = x.detach().clone().requires_grad_()
    ps = [None if p is None else p.detach().clone().requires_grad_() for p in params]
    y = fn(x, *ps)
    (y * gout).sum().backward()
    return y.detach(), x.grad, [None if p is None else p.grad for p in ps]


def _batch_norm_train(x, w, b, eps=1e-5):
    """BatchNorm1d(L) on (B, L, E) in training mode; returns (y, batch mean, unbiased batch variance)"""
    mean = x.mean(dim=(0, 2), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(0, 2), keepdim=True)
    n = x.shape[0] * x.shape[2]
    y = (x - mean) / torch.sqrt(var + eps) * w.view(1, -1, 1) + b.view(1, -1, 1)
    return y, mean.reshape(-1), var.reshape(-1) * n / (n - 1)


def model(sd, x, H, momentum=0.1):
    """the model's (B, L) output from its state_dict ``sd`` (tensors that may require grad) in training mode, and
    {key: updated running_mean / running_var / num_batches_tracked}"""
    p = "layers.InputLayer."
    h = (x + sd[p + "PositionEmbedding.bias"]) @ sd[p + "FeedForward.weight"].t() + sd[p + "FeedForward.bias"]
    after = {}
    i = 0
    while f"layers.EncodingLayer.Transformer_{i}.MultiHeadAttention.in_proj_weight" in sd:
        t = f"layers.EncodingLayer.Transformer_{i}."
        h = block(h, *(sd[t + "MultiHeadAttention." + k] for k in MHA_KEYS), H)
        for bn, ff in (("AttentionBatchNorm", False), ("FNNBatchNorm", True)):
            if ff:
                h = h + torch.relu(h @ sd[t + "FeedForward.FeedForward.weight"].t() + sd[t + "FeedForward.FeedForward.bias"])
            h, mean, var = _batch_norm_train(h, sd[t + bn + ".weight"], sd[t + bn + ".bias"])
            after[t + bn + ".running_mean"] = ((1 - momentum) * sd[t + bn + ".running_mean"] + momentum * mean).detach()
            after[t + bn + ".running_var"] = ((1 - momentum) * sd[t + bn + ".running_var"] + momentum * var).detach()
            after[t + bn + ".num_batches_tracked"] = sd[t + bn + ".num_batches_tracked"] + 1
        i += 1
    p = "layers.OutputLayer.FeedForward."
    return torch.softmax((h @ sd[p + "weight"].t() + sd[p + "bias"]).flatten(1), dim=1), after

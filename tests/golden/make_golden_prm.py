"""Golden vectors for PersonalizedReRankingModel (models/ltr/personalized_reranking.py), captured from the REAL reference in
the build container (same stub import recipe as make_golden.py).  CPU float64 (``model.double()``), fixed seeds,
``dropout=0.0`` (the default ``None`` raises), training mode -- so the BatchNorm1d(L) pairs use batch statistics and move
their running ones -- and non-zero attention and linear biases.
Run:  python tests/golden/make_golden_prm.py    (needs the reference checkout; writes tests/golden/prm.npz)

Per shape (B, L, embed, E, H, layers):
  model/<tag>/{input, gout, out, names, keys}, param/<key> for every state_dict entry before the step, after/<key> for
  every entry the forward + backward changed (the running statistics and their counters) and ``unchanged`` naming the
  rest (checked here to be bit-identical), grad/<key> for every parameter and grad/input;
  block/<tag>/{x, gout, y, dx, grad/<key>}: ``x + MHA(x)`` of the FIRST layer's attention alone on a random (B, L, E).
Inputs, ``gout`` and the parameters are drawn in float64 and rounded to bf16-representable values: the same numbers serve
fp32 and bf16 runs without a second rounding, and the zero low mantissa bits keep the compressed file small.
Fixtures hold data only (arrays and name lists)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, npy, save  # noqa: E402

# (B, L, embed, E, H, layers)
PRM_SHAPES = [(6, 5, 12, 16, 2, 2), (5, 7, 24, 64, 4, 1), (7, 33, 32, 32, 1, 2), (6, 4, 10, 10, 5, 2)]


def bf16_values(t):
    return t.to(torch.bfloat16).to(torch.float64)


def gen(models_mod, out):
    from torecsys.models.ltr.personalized_reranking import PersonalizedReRankingModel
    for (B, L, emb, E, H, layers) in PRM_SHAPES:
        tag = f"{B}_{L}_{emb}_{E}_h{H}_l{layers}"
        g = torch.Generator().manual_seed(9700 + B * 5 + L * 11 + emb + E + H + layers)
        torch.manual_seed(9800 + B + L + emb + E + H)
        m = PersonalizedReRankingModel(embed_size=emb, max_num_position=L, encoding_size=E, num_heads=H,
                                       num_layers=layers, dropout=0.0).double()
        m.train()
        with torch.no_grad():
            for k, p in m.named_parameters():
                if k.endswith("bias") and "BatchNorm" not in k and "PositionEmbedding" not in k:
                    p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)      # MHA zero-initialises its own
                elif "BatchNorm" in k:
                    p.add_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.1)      # gamma != 1, beta != 0
                p.copy_(bf16_values(p))
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        x = bf16_values(torch.randn(B, L, emb, generator=g, dtype=torch.float64)).requires_grad_()
        y = m(x)
        gout = bf16_values(torch.randn(B, L, generator=g, dtype=torch.float64))
        (y.rename(None) * gout).sum().backward()
        pre = f"model/{tag}"
        out[f"{pre}/input"] = npy(x)
        out[f"{pre}/gout"] = npy(gout)
        out[f"{pre}/out"] = npy(y)
        out[f"{pre}/names"] = np.array(list(y.names))
        out[f"{pre}/keys"] = np.array(list(before.keys()))
        unchanged = []
        for k, v in m.state_dict().items():
            out[f"{pre}/param/{k}"] = npy(before[k])
            if torch.equal(v, before[k]):
                unchanged.append(k)
            else:
                out[f"{pre}/after/{k}"] = npy(v)
        out[f"{pre}/unchanged"] = np.array(unchanged)
        assert all("running_" in k or "num_batches_tracked" in k for k in before if k not in unchanged)
        for k, p in m.named_parameters():
            out[f"{pre}/grad/{k}"] = npy(p.grad)
        out[f"{pre}/grad/input"] = npy(x.grad)

        # the first layer's attention alone: x + MHA(x) on the transposed block, as the model's forward runs it
        mha = m.layers["EncodingLayer"]["Transformer_0"]["MultiHeadAttention"]
        for p in mha.parameters():
            p.grad = None
        xb = bf16_values(torch.randn(B, L, E, generator=g, dtype=torch.float64)).requires_grad_()
        gb = bf16_values(torch.randn(B, L, E, generator=g, dtype=torch.float64))
        xt = xb.transpose(0, 1)
        yb = xb + mha(xt, xt, xt)[0].transpose(0, 1)
        (yb * gb).sum().backward()
        pre = f"block/{tag}"
        out[f"{pre}/x"] = npy(xb)
        out[f"{pre}/gout"] = npy(gb)
        out[f"{pre}/y"] = npy(yb)
        out[f"{pre}/dx"] = npy(xb.grad)
        for k, p in mha.named_parameters():
            out[f"{pre}/grad/{k}"] = npy(p.grad)


def main():
    _, _, models_mod = import_reference()
    d = {}
    gen(models_mod, d)
    save("prm.npz", d)


if __name__ == "__main__":
    main()

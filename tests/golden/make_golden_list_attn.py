"""Golden vectors for ListIndicesEmbedding(use_attn=True, output_method='avg_pooling') (inputs/base/list_indices_emb.py),
captured from the REAL reference in the build container (same stub import recipe as make_golden.py).  CPU fp32, fixed
seeds, attention dropout 0.  The reference's ``mean`` and ``sum`` raise, so only ``avg_pooling`` is recorded.
Run:  python tests/golden/make_golden_list_attn.py    (needs the reference checkout; writes tests/golden/list_attn.npz)

Index quirks as in make_golden_list.py: an all-padding bag, trailing padding, a repeated id, a non-zero padding row.
Fixtures hold data only (arrays and name lists)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, npy, save  # noqa: E402
from make_golden_list import make_idx  # noqa: E402

# (B, L, E, V, H, bias)
ATTN_SHAPES = [(6, 5, 16, 12, 2, True), (5, 7, 64, 20, 4, True), (4, 1, 8, 9, 1, True), (7, 33, 32, 40, 1, False),
               (6, 4, 10, 7, 5, True)]


def gen(inputs_mod, out):
    for (B, L, E, V, H, bias) in ATTN_SHAPES:
        g = torch.Generator().manual_seed(9500 + B * 5 + L * 11 + E + V + H)
        idx = make_idx(g, B, L, V)
        torch.manual_seed(9600 + B + L + E + H)
        m = inputs_mod.ListIndicesEmbedding(embed_size=E, field_size=V, output_method="avg_pooling", use_attn=True,
                                            num_heads=H, bias=bias)
        with torch.no_grad():
            m.embedding.weight[0] = torch.randn(E, generator=g)          # a non-zero padding row
            for k, p in m.attention.named_parameters():
                if k.endswith("bias"):                                   # nn.MultiheadAttention zero-initialises them
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
        y = m(idx)
        gout = torch.randn(*y.shape, generator=g)
        (y.rename(None) * gout).sum().backward()
        pre = f"{B}_{L}_{E}_{V}_h{H}_b{int(bias)}"
        out[f"{pre}/idx"] = npy(idx)
        out[f"{pre}/out"] = npy(y)
        out[f"{pre}/names"] = np.array(list(y.names))
        out[f"{pre}/gout"] = npy(gout)
        out[f"{pre}/keys"] = np.array(list(m.state_dict().keys()))
        for k, p in m.named_parameters():
            out[f"{pre}/param/{k}"] = npy(p)
            out[f"{pre}/grad/{k}"] = npy(p.grad)


def main():
    inputs_mod, _, _ = import_reference()
    d = {}
    gen(inputs_mod, d)
    save("list_attn.npz", d)


if __name__ == "__main__":
    main()

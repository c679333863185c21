"""Golden vectors for ListIndicesEmbedding (inputs/base/list_indices_emb.py), captured from the REAL reference in the build
container (same stub import recipe as make_golden.py).  CPU fp32, fixed seeds, attention dropout 0.
Run:  python tests/golden/make_golden_list.py    (needs the reference checkout; writes tests/golden/list.npz)

Every index block holds an all-padding bag, bags with trailing padding and a bag with a repeated id; table rows 3 and 4
are made EQUAL (and the largest of the table) and appear in both orders, which pins the tie rule of max pooling; the
padding row 0 is set non-zero after construction (a loaded table may hold anything there, and the forward reads it).
Fixtures hold data only (arrays and name lists)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, npy, save  # noqa: E402

LIST_SHAPES = [(6, 5, 16, 12), (4, 1, 8, 9), (5, 7, 64, 20), (6, 4, 10, 7)]      # (B, L, E, V)
LIST_CASES = [("avg_pooling", 0), ("max_pooling", 0), ("none", 0), ("avg_pooling", 1), ("max_pooling", 2)]  # (method, heads)


def case_tag(method, heads):
    return method if heads == 0 else f"attn{heads}_{method}"


def make_idx(g, B, L, V):
    idx = torch.randint(1, V, (B, L), generator=g)
    idx[0, :] = 0                                  # an all-padding bag
    if L >= 4:
        idx[1, L - 2:] = 0                         # trailing padding
        idx[2, 1] = idx[2, 0]                      # a repeated id inside a bag
        idx[3, 0], idx[3, 1] = 3, 4                # the two equal rows, in both orders
        idx[4 % B, 0], idx[4 % B, 1] = 4, 3
        idx[B - 1, L - 1] = 0
    else:
        idx[1, 0] = 3
        idx[2, 0] = 4
    return idx


def gen(inputs_mod, out):
    for (B, L, E, V) in LIST_SHAPES:
        g = torch.Generator().manual_seed(9000 + B * 5 + L * 11 + E + V)
        idx = make_idx(g, B, L, V)
        shape = f"{B}_{L}_{E}_{V}"
        out[f"{shape}/idx"] = npy(idx)
        for method, heads in LIST_CASES:
            torch.manual_seed(9100 + B + L + E + heads)
            kw = dict(use_attn=True, num_heads=heads) if heads else {}
            m = inputs_mod.ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method, **kw)
            with torch.no_grad():
                m.embedding.weight[0] = torch.randn(E, generator=g)          # a non-zero padding row
                m.embedding.weight[3] = m.embedding.weight[3].abs() + 4.0    # rows 3 and 4: equal, and the maxima
                m.embedding.weight[4] = m.embedding.weight[3]
            y = m(idx)
            gout = torch.randn(*y.shape, generator=g)
            (y.rename(None) * gout).sum().backward()
            pre = f"{shape}/{case_tag(method, heads)}"
            out[f"{pre}/out"] = npy(y)
            out[f"{pre}/names"] = np.array(list(y.names))
            out[f"{pre}/gout"] = npy(gout)
            out[f"{pre}/keys"] = np.array(list(m.state_dict().keys()))
            out[f"{pre}/attrs"] = np.array([len(m), m.field_size, m.embed_size, m.padding_idx, m.length], dtype=np.int64)
            for k, p in m.named_parameters():
                out[f"{pre}/param/{k}"] = npy(p)
                out[f"{pre}/grad/{k}"] = npy(p.grad)


def main():
    inputs_mod, _, _ = import_reference()
    d = {}
    gen(inputs_mod, d)
    save("list.npz", d)


if __name__ == "__main__":
    main()

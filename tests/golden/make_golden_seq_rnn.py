"""Golden vectors for SequenceIndicesEmbedding (inputs/base/sequence_indices_emb.py), captured from the REAL reference in
the build container (same stub import recipe as make_golden.py).  CPU fp32, fixed seeds.
Run:  python tests/golden/make_golden_seq_rnn.py    (needs the reference checkout; writes tests/golden/seq_rnn.npz
and tests/golden/seq_rnn_e64.npz)

Per shape (B, L, E, V) of seq_rnn_ref.GOLDEN_SHAPES: idx and lengths; per cell the five parameters (the cases of one cell
are built from one seed and share them: the three LSTM cases at E = 64 would otherwise hold the same 130 KiB three times);
per case (cell, output_method) of GOLDEN_CASES the output and its names, gout, the gradients of the five parameters and the
state_dict keys.  Ids are 0 from each sample's length on.  The E = 64 shape goes to a file of its own, seq_rnn_e64.npz
(seq_rnn_ref.golden_file): together the cases exceed the 1 MiB a committed file may have.  Fixtures hold data only (arrays
and name lists)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference, npy, save  # noqa: E402
from seq_rnn_ref import GOLDEN_CASES, GOLDEN_SHAPES, golden_file, golden_lengths, make_ids, shape_tag  # noqa: E402


def gen(inputs_mod, s, out):
    B, L, E, V = s
    lengths = golden_lengths(B, L, E)
    idx = make_ids(B, L, V, lengths, 4300 + B + L + E + V)
    out[f"{shape_tag(s)}/idx"] = npy(idx)
    out[f"{shape_tag(s)}/lengths"] = npy(lengths)
    for n, (cell, method) in enumerate(GOLDEN_CASES):
        tag = f"{shape_tag(s)}/{cell}_{method}"
        torch.manual_seed(4500 + B + L + E + V + len(cell) + ord(cell[0]))      # one seed per (shape, cell)
        m = inputs_mod.SequenceIndicesEmbedding(embed_size=E, field_size=V, rnn_method=cell, output_method=method)
        y = m(idx.clone(), lengths.clone())
        g = torch.Generator().manual_seed(4700 + B + L + E + n)
        gout = torch.randn(*y.shape, generator=g)
        (y.rename(None) * gout).sum().backward()
        print(f"{tag}: lengths {lengths.tolist()} out {tuple(y.shape)} {y.names}")
        out[f"{tag}/out"] = npy(y)
        out[f"{tag}/names"] = np.array(list(y.names))
        out[f"{tag}/gout"] = npy(gout)
        out[f"{tag}/keys"] = np.array(list(m.state_dict().keys()))
        for k, p in m.state_dict(keep_vars=True).items():
            pk = f"{shape_tag(s)}/{cell}/param/{k}"
            if pk in out:
                assert np.array_equal(out[pk], npy(p)), pk
            out[pk] = npy(p)
            out[f"{tag}/grad/{k}"] = npy(p.grad)


def main():
    inputs_mod, _, _ = import_reference()
    files = {}
    for s in GOLDEN_SHAPES:
        gen(inputs_mod, s, files.setdefault(golden_file(s), {}))
    for name, d in files.items():
        save(name + ".npz", d)


if __name__ == "__main__":
    main()

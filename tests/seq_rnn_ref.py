"""The plain torch restatement of SequenceIndicesEmbedding (inputs/base/sequence_indices_emb.py) that the sequence tests
compare against (CPU, any floating dtype): a step loop over t < L with a live mask t < lengths[b], one layer, one
direction, hidden size E, PyTorch's gate order and GRU form:
    rnn:  h_t = tanh(W_ih x_t + b_ih + W_hh h_{t-1} + b_hh)
    lstm: [i f g o] = W_ih x_t + b_ih + W_hh h_{t-1} + b_hh;  c_t = s(f) c_{t-1} + s(i) tanh(g);  h_t = s(o) tanh(c_t)
    gru:  r, z = s(...);  n = tanh(W_in x_t + b_in + r (W_hn h_{t-1} + b_hn));  h_t = (1 - z) n + z h_{t-1}
    'avg' -> (B, 1, E) = sum_{t < len} h_t / max(lengths)   (pad_packed_sequence pads to the batch maximum: the divisor is
             neither L nor the sample's own length);  'sum' -> the unscaled sum;  'none' -> (B, max(lengths), E), zeros
             from each sample's length on;  'max_pooling' -> (B, max(lengths), 1), the maximum over E of 'none' (what the
             reference's `in ['avg_pooling' or 'max_pooling']` makes of it).
Lengths are clamped to [0, L] (the kernels' rule; the reference raises for a length <= 0).  A row id outside [0, V) reads
as a zero row.  tests/test_seq_rnn_host.py pins the restatement to the reference's own outputs and gradients
(tests/golden/seq_rnn.npz and seq_rnn_e64.npz); the GPU tests run it in fp64 at sizes the fixture does not hold.  Also the case lists shared
by the generator (tests/golden/make_golden_seq_rnn.py) and the tests."""
import torch

CELLS = ("lstm", "gru", "rnn")
GATES = {"rnn": 1, "lstm": 4, "gru": 3}
# (B, L, E, V): shapes of seq_rnn.npz / seq_rnn_e64.npz (golden_file).  Every shape has the full L in at least one sample except (5, 7, 64, 20), whose
# longest sample has 5 steps.
GOLDEN_SHAPES = [(6, 5, 16, 12), (5, 7, 64, 20), (4, 1, 8, 9), (7, 33, 32, 40)]
# (cell, output_method) cases stored per shape
GOLDEN_CASES = [("lstm", "avg_pooling"), ("gru", "avg_pooling"), ("rnn", "avg_pooling"), ("lstm", "none"),
                ("lstm", "max_pooling")]
PARAM_KEYS = ["embedding.weight", "rnn_layers.weight_ih_l0", "rnn_layers.weight_hh_l0", "rnn_layers.bias_ih_l0",
              "rnn_layers.bias_hh_l0"]
# (B, L, E) of the GPU tests against the fp64 restatement: B around the 16- and 32-row tiles, E off the 16 grid (8, 24)
# and at the vector path's limit (128)
GPU_SHAPES = [(1, 1, 16), (15, 3, 16), (17, 5, 32), (33, 7, 64), (67, 64, 64), (5, 9, 8), (6, 4, 24), (3, 6, 128)]


def shape_tag(s):
    return "_".join(str(v) for v in s)


def golden_file(s):
    """the fixture that holds a shape of GOLDEN_SHAPES: the E = 64 shape has a file of its own (a committed file stays
    under 1 MiB)"""
    return "seq_rnn_e64" if s[2] == 64 else "seq_rnn"


def golden_lengths(B, L, E):
    """mixed lengths that include 1; the full L in sample 0 except at (5, 7, 64), where the longest is 5"""
    g = torch.Generator().manual_seed(4100 + 7 * B + 3 * L + E)
    top = 5 if (B, L, E) == (5, 7, 64) else L
    lens = torch.randint(1, top + 1, (B,), generator=g)
    lens[0] = top
    lens[B - 1] = 1
    return lens


def make_ids(B, L, V, lengths, seed):
    """ids in [1, V) at the live steps, 0 (the padding id) from each sample's length on"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(1, V, (B, L), generator=g)
    return torch.where(torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1), idx, torch.zeros_like(idx))


def make_params(cell, E, V, dtype=torch.float32, seed=0):
    """table (row 0 zero, as nn.Embedding(padding_idx=0) leaves it), w_ih, w_hh, b_ih, b_hh drawn as nn.LSTM draws them
    (uniform in +-1/sqrt(E)), rounded to ``dtype`` and returned in fp32 (values representable in ``dtype``)"""
    g = torch.Generator().manual_seed(5200 + seed + 11 * E + V)
    G, k = GATES[cell], E ** -0.5
    table = torch.randn(V, E, generator=g)
    table[0] = 0
    ps = [table] + [(2 * torch.rand(*s, generator=g) - 1) * k for s in ((G * E, E), (G * E, E), (G * E,), (G * E,))]
    return tuple(p.to(dtype).float() for p in ps)


def seq_rnn_steps(table, idx, lengths, w_ih, w_hh, b_ih, b_hh, cell):
    """(B, L, E): every h_t, zeros from each sample's (clamped) length on; differentiable in the five parameters"""
    B, L = idx.shape
    V, E = table.shape
    ok = (idx >= 0) & (idx < V)
    x = table[idx.clamp(0, V - 1)] * ok.unsqueeze(-1).to(table.dtype)
    lens = lengths.clamp(0, L)
    h = table.new_zeros(B, E)
    c = table.new_zeros(B, E)
    outs = []
    for t in range(L):
        live = (t < lens).unsqueeze(-1)
        gi = x[:, t] @ w_ih.t() + b_ih
        gh = h @ w_hh.t() + b_hh
        if cell == "rnn":
            hn = torch.tanh(gi + gh)
        elif cell == "lstm":
            i, f, g, o = (gi + gh).chunk(4, dim=1)
            cn = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            hn = torch.sigmoid(o) * torch.tanh(cn)
            c = torch.where(live, cn, c)
        elif cell == "gru":
            ir, iz, inn = gi.chunk(3, dim=1)
            hr, hz, hnn = gh.chunk(3, dim=1)
            r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
            n = torch.tanh(inn + r * hnn)
            hn = (1 - z) * n + z * h
        else:
            raise ValueError(cell)
        h = torch.where(live, hn, h)
        outs.append(torch.where(live, hn, torch.zeros_like(hn)))
    return torch.stack(outs, dim=1)


def seq_rnn(table, idx, lengths, w_ih, w_hh, b_ih, b_hh, cell, method="avg_pooling"):
    """the module's output for ``method`` (un-named): see the module docstring"""
    steps = seq_rnn_steps(table, idx, lengths, w_ih, w_hh, b_ih, b_hh, cell)
    longest = int(lengths.clamp(0, idx.shape[1]).max()) if lengths.numel() else 0
    if method in ("avg_pooling", "mean"):
        return steps.sum(dim=1, keepdim=True) / max(longest, 1)
    if method == "sum":
        return steps.sum(dim=1, keepdim=True)
    if method == "none":
        return steps[:, :longest]
    if method == "max_pooling":
        return steps[:, :longest].amax(dim=2, keepdim=True)
    raise ValueError(method)


def seq_rnn_grads(params, idx, lengths, cell, method, gout):
    """out and the gradients of (table, w_ih, w_hh, b_ih, b_hh) of the restatement, in the operands' dtype"""
    ps = [p.detach().clone().requires_grad_() for p in params]
    out = seq_rnn(ps[0], idx, lengths, *ps[1:], cell, method)
    grads = torch.autograd.grad(out, ps, gout.to(out.dtype))
    return out.detach(), grads

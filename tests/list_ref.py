"""The plain torch restatement of ListIndicesEmbedding that the list / bag tests compare against (CPU):
``F.embedding(idx, w, padding_idx)`` -> (attention) -> ``sum(1)`` / ``sum(1) / L`` / ``max(1)``.  tests/test_list_indices_host.py
pins it to the reference's own outputs and gradients (tests/golden/list.npz); the GPU tests use it at sizes the fixture
does not hold."""
import torch
import torch.nn.functional as F

LIST_SHAPES = [(6, 5, 16, 12), (4, 1, 8, 9), (5, 7, 64, 20), (6, 4, 10, 7)]      # (B, L, E, V) of list.npz
LIST_CASES = [("avg_pooling", 0), ("max_pooling", 0), ("none", 0), ("avg_pooling", 1), ("max_pooling", 2)]
POOL = {"avg_pooling": "mean", "max_pooling": "max", "mean": "mean", "sum": "sum", "none": "none"}


def case_tag(method, heads):
    return method if heads == 0 else f"attn{heads}_{method}"


def shape_tag(s):
    return "%d_%d_%d_%d" % s


def pool(block, mode):
    """(B, L, E) -> (B, 1, E) (``none``: unchanged)"""
    if mode == "none":
        return block
    if mode == "max":
        return block.max(dim=1, keepdim=True)[0]
    s = block.sum(dim=1, keepdim=True)
    return s / block.shape[1] if mode == "mean" else s


def compose(weight, idx, mode, padding_idx=None, attention=None):
    """weight (V, E) requires_grad or not; returns the pooled output"""
    block = F.embedding(idx.long(), weight, padding_idx=padding_idx)
    if attention is not None:
        seq = block.transpose(0, 1)
        seq, _ = attention(seq, seq, seq)
        block = seq.transpose(0, 1)
    return pool(block, mode)


def compose_chunked(weight, idx, mode, gout, padding_idx=None, chunk=4096, dtype=torch.float64):
    """Outputs (B, 1, E) and the dense table gradient for ``gout`` (B, 1, E) of ``compose`` (no attention), evaluated a
    chunk of samples at a time in ``dtype`` -- the (B, L, E) block of a full-size batch does not have to exist on the host
    either, and no autograd graph is kept; every sample and every table row is covered.  The gradient is the composition's,
    written out: every position of a bag receives the sample's gradient (times 1/L for the mean); for the max, the first
    position that holds the maximum of a column receives it; the padding row receives none.
    tests/test_list_indices_host.py pins this to autograd through ``compose`` and to the reference's fixture."""
    w = weight.detach().to(dtype)
    V, E = w.shape
    L = idx.shape[1]
    grad = torch.zeros(V * E, dtype=dtype)
    cols = torch.arange(E)
    outs = []
    for b0 in range(0, idx.shape[0], chunk):
        ix = idx[b0:b0 + chunk].long()
        g = gout[b0:b0 + chunk].reshape(-1, E).to(dtype)
        block = w[ix]                                                      # (c, L, E)
        if mode == "max":
            y, am = block.max(dim=1)                                       # first maximal position on ties
            rows = ix.gather(1, am)                                        # (c, E): the table row each column's gradient goes to
            grad.index_add_(0, (rows * E + cols).reshape(-1), g.reshape(-1))
        else:
            y = block.sum(dim=1)
            if mode == "mean":
                y, g = y / L, g / L
            grad.view(V, E).index_add_(0, ix.reshape(-1), g.unsqueeze(1).expand(-1, L, -1).reshape(-1, E))
        outs.append(y.unsqueeze(1))
    grad = grad.view(V, E)
    if padding_idx is not None:
        grad[padding_idx] = 0
    return torch.cat(outs), grad

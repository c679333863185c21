"""GPU parity of ListIndicesEmbedding and functional.bag_pool (csrc/bag.hip): against the reference's own outputs and
gradients (tests/golden/list.npz) and, at sizes the fixture does not hold, against the plain torch composition on the CPU
(tests/list_ref.py, pinned to the fixture by tests/test_list_indices_host.py).  Selections (``none``, the max) are
bit-exact; fp32 sums 1e-5 relative; bf16: 1e-2 relative against the composition evaluated on bf16-rounded inputs."""
import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from list_ref import LIST_CASES, LIST_SHAPES, POOL, case_tag, compose, compose_chunked, shape_tag

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
TOLBF = 1e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _zipf_bags(g, B, L, V, pad_frac):
    """(B, L) ids in [1, V): Zipf(1.05)-distributed ranks, then ``pad_frac`` of all positions set to the padding id 0 --
    as trailing padding of random length plus one all-padding bag"""
    ranks = torch.arange(1, V, dtype=torch.float64)
    p = ranks.pow(-1.05)
    idx = 1 + torch.multinomial(p / p.sum(), B * L, replacement=True, generator=g).reshape(B, L)
    if pad_frac > 0:
        keep = torch.rand(B, generator=g) * 2 * (1 - pad_frac) * L          # mean kept length (1 - pad_frac) * L
        idx = torch.where(torch.arange(L).view(1, L) < keep.view(B, 1), idx, torch.zeros_like(idx))
        idx[0] = 0
    return idx


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("shape", LIST_SHAPES)
@pytest.mark.parametrize("method,heads", LIST_CASES)
def test_list_indices_embedding_golden(golden, dev, shape, method, heads):
    from torecsys_amd.inputs import ListIndicesEmbedding
    G = golden("list")
    B, L, E, V = shape
    pre = f"{shape_tag(shape)}/{case_tag(method, heads)}"
    kw = dict(use_attn=True, num_heads=heads) if heads else {}
    m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method, **kw).to(dev)
    assert list(m.state_dict().keys()) == G(pre + "/keys")
    m.load_state_dict({k: G(f"{pre}/param/{k}") for k in G(pre + "/keys")})
    idx = G(f"{shape_tag(shape)}/idx").to(dev)
    out = m(idx)
    assert out.names == tuple(G(pre + "/names")) == ("B", "N", "E")
    y = out.rename(None)
    assert tuple(y.shape) == tuple(G(pre + "/out").shape)
    if not heads and method in ("none", "max_pooling"):
        assert torch.equal(y.cpu(), G(pre + "/out"))                       # selections: bit-exact
    else:
        assert rel_err(y.cpu(), G(pre + "/out")) <= TOL32
    (y * G(pre + "/gout").to(dev)).sum().backward()
    for k, p in m.named_parameters():
        assert rel_err(p.grad.cpu(), G(f"{pre}/grad/{k}")) <= TOL32, k
    assert float(m.embedding.weight.grad[0].abs().max()) == 0.0          # the padding row: exactly zero
    if method == "max_pooling" and not heads:
        # the tie case (table rows 3 and 4 are equal, both orders occur): only the first position takes the gradient, so
        # each of the two rows' gradients is the fixture's, not a split or a swap of them
        gw, want = m.embedding.weight.grad.cpu(), G(pre + "/grad/embedding.weight")
        assert rel_err(gw[3], want[3]) <= TOL32 and rel_err(gw[4], want[4]) <= TOL32
        assert not torch.equal(want[3], want[4])
    if not heads and method != "none":
        # the functional entry, int32 ids
        from torecsys_amd import functional as F_
        w = m.embedding.weight.detach().clone().requires_grad_()
        y2 = F_.bag_pool(w, idx.to(torch.int32), POOL[method], padding_idx=0)
        assert tuple(y2.shape) == (B, 1, E) and torch.equal(y2, y)
        (y2 * G(pre + "/gout").to(dev)).sum().backward()
        assert rel_err(w.grad.cpu(), G(pre + "/grad/embedding.weight")) <= TOL32      # (bucket order is not fixed: no bit equality)


# ------------------------------------------------------------------------------------------------ the torch composition
@pytest.mark.parametrize("L", [1, 3, 50, 300])
@pytest.mark.parametrize("E", [64, 128, 16, 8, 10])
@pytest.mark.parametrize("dtype,idt", [(torch.float32, torch.int64), (torch.float32, torch.int32),
                                       (torch.bfloat16, torch.int64), (torch.bfloat16, torch.int32)])
def test_bag_pool_against_torch_composition(dev, dtype, idt, E, L):
    """sum / mean / max on Zipf ids with 60 % padding: outputs and the whole table gradient.  L = 300 is beyond one chunk
    of the walk and puts thousands of lookups on the head rows (hot-row queue, rows of several chunks); with int32 ids
    there is no padding row, so row 0 itself (60 % of all lookups) is reduced like any hot row.  E = 10: generic path."""
    from torecsys_amd import functional as F_
    B, V = 384, 1000
    g = torch.Generator().manual_seed(1234 + L * 7 + E)
    idx = _zipf_bags(g, B, L, V, 0.6)
    w = torch.randn(V, E, generator=g).to(dtype)
    gout = torch.randn(B, 1, E, generator=g).to(dtype)
    pad = 0 if idt == torch.int64 else None
    tol = TOL32 if dtype == torch.float32 else TOLBF
    for mode in ("sum", "mean", "max"):
        want_y, want_g = compose_chunked(w.float(), idx, mode, gout.float(), padding_idx=pad)
        wd = w.to(dev).requires_grad_()
        y = F_.bag_pool(wd, idx.to(dev).to(idt), mode, padding_idx=pad)
        assert tuple(y.shape) == (B, 1, E) and y.dtype == dtype
        if mode == "max":
            assert torch.equal(y.float().cpu(), want_y.float()), mode                   # a selection: bit-exact
        else:
            assert rel_err(y.float().cpu(), want_y) <= tol, mode
        (y * gout.to(dev)).sum().backward()
        assert rel_err(wd.grad.float().cpu(), want_g) <= tol, mode
        if pad is not None:
            assert float(wd.grad[0].abs().max()) == 0.0
        else:
            assert float(wd.grad[0].abs().max()) > 0.0


@pytest.mark.parametrize("method", ["sum", "mean"])
def test_module_sum_and_mean_modes(dev, method):
    """``sum`` / ``mean`` raise in the reference; the drop-in serves what its docstring promises, (B,1,E) named B,N,E"""
    from torecsys_amd.inputs import ListIndicesEmbedding
    B, L, E, V = 64, 9, 16, 50
    g = torch.Generator().manual_seed(5)
    idx = _zipf_bags(g, B, L, V, 0.3)
    m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method).to(dev)
    w = m.embedding.weight.detach().cpu().clone()
    gout = torch.randn(B, 1, E, generator=g)
    want_y, want_g = compose_chunked(w, idx, method, gout, padding_idx=0)
    out = m(idx.to(dev))
    assert out.names == ("B", "N", "E") and tuple(out.shape) == (B, 1, E)
    assert rel_err(out.rename(None).cpu(), want_y) <= TOL32
    (out.rename(None) * gout.to(dev)).sum().backward()
    assert rel_err(m.embedding.weight.grad.cpu(), want_g) <= TOL32
    if method == "mean":
        avg = ListIndicesEmbedding(embed_size=E, field_size=V, output_method="avg_pooling").to(dev)
        avg.load_state_dict(m.state_dict())
        assert torch.equal(avg(idx.to(dev)).rename(None), out.rename(None))


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_bag_pool_full_size(dev, mode):
    """B = 65 536, L = 50, E = 64, V = 1 M, bf16: ALL outputs and the whole table gradient against the composition
    (evaluated on the host a chunk of samples at a time, nothing sampled), and the forward's peak device allocation
    stays below a quarter of the (B, L, E) block the reference forms: no block exists."""
    from torecsys_amd import functional as F_
    B, L, E, V = 65536, 50, 64, 1_000_000
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(77)
    idx = _zipf_bags(g, B, L, V, 0.3)
    w = (torch.randn(V, E, generator=g) * 0.5).to(dtype)
    gout = torch.randn(B, 1, E, generator=g).to(dtype)
    wd = w.to(dev).requires_grad_()
    idx_d, gout_d = idx.to(dev), gout.to(dev)
    F_.clear_caches()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = F_.bag_pool(wd, idx_d, mode, padding_idx=0)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    block = B * L * E * w.element_size()
    print(f"forward peak allocation {peak / 2**20:.1f} MiB, (B,L,E) block {block / 2**20:.1f} MiB")
    assert peak < block / 4
    (y * gout_d).sum().backward()
    got_y, got_g = y.detach().float().cpu(), wd.grad.float().cpu()
    want_y, want_g = compose_chunked(w.float(), idx, mode, gout.float(), padding_idx=0, chunk=2048, dtype=torch.float32)
    if mode == "max":
        assert torch.equal(got_y, want_y)
    else:
        assert rel_err(got_y, want_y) <= TOLBF
    assert tuple(got_g.shape) == (V, E)
    assert rel_err(got_g, want_g) <= TOLBF
    assert float(got_g[0].abs().max()) == 0.0


@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
def test_row_buckets_without_the_padding_id(dev, idt):
    """trs_csr_build_skip: the padding id gets an empty bucket, every other row the bucket trs_csr_build gives it"""
    from torecsys_amd import functional as F_
    B, L, V = 700, 40, 300
    idx = _zipf_bags(torch.Generator().manual_seed(9), B, L, V, 0.6).to(dev).to(idt)
    F_.clear_caches()
    full = F_.row_buckets(idx, None, V)
    skip = F_.row_buckets(idx, None, V, skip_row=0)
    assert skip is not full
    torch.cuda.synchronize()
    rs_f, rs_s = full.row_start.cpu().long(), skip.row_start.cpu().long()
    n_f, n_s = rs_f[1:] - rs_f[:-1], rs_s[1:] - rs_s[:-1]
    n_pad = int((idx == 0).sum())
    assert int(n_f[0]) == n_pad > 0 and int(n_s[0]) == 0 and torch.equal(n_f[1:], n_s[1:])
    assert int(rs_s[0]) == 0 and int(rs_s[-1]) == B * L - n_pad
    flat = idx.reshape(-1).cpu().long()
    perm = skip.perm.cpu().long()[:B * L - n_pad]
    assert int(perm.min()) >= 0 and int(perm.max()) < B * L and perm.unique().numel() == perm.numel()
    rows = torch.repeat_interleave(torch.arange(V), n_s)
    assert torch.equal(flat[perm], rows)          # every listed position holds the id of the bucket it is filed under


# ------------------------------------------------------------------------------------------------ fused optimizers
@pytest.mark.parametrize("kind", ["sgd", "adagrad"])
@pytest.mark.parametrize("method", ["avg_pooling", "sum"])
def test_fused_sparse_optimizer_equals_dense_step(dev, kind, method):
    from torecsys_amd.inputs import ListIndicesEmbedding
    from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseSGD
    B, L, E, V = 1024, 12, 16, 300
    g = torch.Generator().manual_seed(11)
    batches = [_zipf_bags(g, B, L, V, 0.4).to(dev) for _ in range(3)]
    w0 = torch.randn(V, E, generator=g)
    lr = 0.05
    res = []
    for fused in (False, True):
        m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method).to(dev)
        m.embedding.weight.data.copy_(w0)
        if fused:
            m.set_fused_optimizer(FusedSparseSGD(lr) if kind == "sgd" else FusedSparseAdagrad(lr, eps=1e-10))
            opt = None
        else:
            opt = (torch.optim.SGD(m.parameters(), lr=lr) if kind == "sgd"
                   else torch.optim.Adagrad(m.parameters(), lr=lr, eps=1e-10))
        for idx in batches:
            loss = (m(idx).rename(None) ** 2).mean()
            if opt is not None:
                opt.zero_grad()
            loss.backward()
            if opt is not None:
                opt.step()
            else:
                assert m.embedding.weight.grad is None
        res.append(m.embedding.weight.detach().cpu())
    assert rel_err(res[1], res[0]) <= TOL32
    assert not torch.equal(res[0], w0) and torch.equal(res[1][0], w0[0])      # the padding row is never updated


def test_max_pooling_with_fused_optimizer_raises(dev):
    from torecsys_amd import functional as F_
    from torecsys_amd.inputs import ListIndicesEmbedding
    from torecsys_amd.optim import FusedSparseSGD
    m = ListIndicesEmbedding(embed_size=8, field_size=10, output_method="max_pooling").to(dev)
    with pytest.raises(NotImplementedError):
        m.set_fused_optimizer(FusedSparseSGD(0.1))
    with pytest.raises(NotImplementedError):
        F_.bag_pool(m.embedding.weight, torch.zeros(2, 3, dtype=torch.long, device=dev), "max", opt=FusedSparseSGD(0.1))


# ------------------------------------------------------------------------------------------------ out-of-range ids
@pytest.mark.parametrize("E", [16, 10])
def test_out_of_range_id(dev, monkeypatch, E):
    """An id outside [0, V) contributes a zero row and no gradient; the lazy flag reports it; with CHECK_INDICES the
    call raises like nn.Embedding."""
    from torecsys_amd import functional as F_
    V = 20
    w = torch.randn(V, E, device=dev)
    bad = torch.tensor([[1, V + 5, 3, 0], [4, 4, -3, 0]], device=dev)
    w_ext = torch.cat([w, torch.zeros(1, E, device=dev)]).cpu()          # row V: what an out-of-range lookup reads as
    ref_idx = torch.where((bad < 0) | (bad >= V), torch.full_like(bad, V), bad).cpu()
    torch.cuda.synchronize()
    F_.index_errors_seen()                                   # clear
    for mode in ("sum", "mean", "max"):
        gout = torch.randn(2, 1, E)
        want_y, want_g = compose_chunked(w_ext, ref_idx, mode, gout)
        assert F_.index_errors_seen() is False
        y = F_.bag_pool(w, bad, mode)
        assert torch.equal(y.cpu(), want_y.float()) if mode == "max" else rel_err(y.cpu(), want_y) <= TOL32
        assert F_.index_errors_seen() is True
        wg = w.clone().requires_grad_()
        (F_.bag_pool(wg, bad, mode) * gout.to(dev)).sum().backward()
        torch.cuda.synchronize()
        assert rel_err(wg.grad.cpu(), want_g[:V]) <= TOL32      # nothing leaks into another row
        assert F_.index_errors_seen() is True
    monkeypatch.setattr(F_, "CHECK_INDICES", True)
    with pytest.raises(IndexError):
        F_.bag_pool(w, bad, "sum")
    monkeypatch.setattr(F_, "CHECK_INDICES", False)
    torch.cuda.synchronize()
    F_.index_errors_seen()


# ------------------------------------------------------------------------------------------------ hipGraph capture
@pytest.mark.parametrize("method", ["avg_pooling", "max_pooling"])
def test_graphed_forward_backward_matches_eager(dev, method):
    from torecsys_amd.graph import GraphedStep
    from torecsys_amd.inputs import ListIndicesEmbedding
    B, L, E, V = 512, 20, 32, 400
    g = torch.Generator().manual_seed(3)
    m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method).to(dev)
    params = list(m.parameters())
    proj = torch.randn(1, 1, E, generator=g).to(dev)
    batches = [(_zipf_bags(g, B, L, V, 0.5).to(dev), torch.randn(B, 1, generator=g).to(dev)) for _ in range(3)]

    def fn(ix, lab):
        loss = (((m(ix).rename(None) * proj).sum(-1) - lab) ** 2).mean()
        loss.backward()
        return loss

    eager = []
    for ix, lab in batches:
        for p in params:
            p.grad = None
        loss = fn(ix, lab)
        eager.append((loss.detach().clone(), m.embedding.weight.grad.clone()))
    del loss
    step = GraphedStep(fn, batches[0], params=params, warmup=2)
    for (ix, lab), (l0, g0) in zip(batches, eager):
        loss = step(ix, lab)
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), l0)
        assert rel_err(m.embedding.weight.grad.cpu(), g0.cpu()) <= TOL32


# ------------------------------------------------------------------------------------------------ composition with a model
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_deepfm_shaped_block_with_a_list_field(dev, dtype):
    """cat([MultiIndicesEmbedding(idx), ListIndicesEmbedding(bag)], dim N) -> FactorizationMachineLayer: output and both
    tables' gradients against the same composition on the CPU."""
    from oracle import cpu_ref as O
    from torecsys_amd.inputs import ListIndicesEmbedding, MultiIndicesEmbedding
    from torecsys_amd.layers import FactorizationMachineLayer
    B, L, E, V = 256, 15, 64, 200
    sizes = [30, 7, 100, 11]
    g = torch.Generator().manual_seed(21)
    idx = torch.stack([torch.randint(0, s, (B,), generator=g) for s in sizes], 1)
    bag = _zipf_bags(g, B, L, V, 0.4)
    emb = MultiIndicesEmbedding(embed_size=E, field_sizes=sizes).to(dev).to(dtype)
    lst = ListIndicesEmbedding(embed_size=E, field_size=V).to(dev).to(dtype)
    gout = torch.randn(B, E, generator=g).to(dtype)
    x = torch.cat([emb(idx.to(dev)).rename(None), lst(bag.to(dev)).rename(None)], dim=1).refine_names("B", "N", "E")
    y = FactorizationMachineLayer()(x).rename(None)
    y = y.reshape(B, E)
    (y * gout.to(dev)).sum().backward()
    # CPU: the same graph in fp32 on the (bf16-rounded) parameters
    we = emb.embedding.weight.detach().float().cpu().requires_grad_()
    wl = lst.embedding.weight.detach().float().cpu().requires_grad_()
    xe = torch.nn.functional.embedding(idx + O.field_offsets(sizes).view(1, -1), we)
    xc = torch.cat([xe, compose(wl, bag, "mean", padding_idx=0)], dim=1)
    yc = 0.5 * (xc.sum(1) ** 2 - (xc ** 2).sum(1))
    (yc * gout.float()).sum().backward()
    tol = TOL32 if dtype == torch.float32 else TOLBF
    assert rel_err(y.float().cpu(), yc) <= tol
    assert rel_err(emb.embedding.weight.grad.float().cpu(), we.grad) <= tol
    assert rel_err(lst.embedding.weight.grad.float().cpu(), wl.grad) <= tol

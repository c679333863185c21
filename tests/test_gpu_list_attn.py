"""GPU parity of ListIndicesEmbedding(use_attn=True) with sum / mean pooling through functional.attn_pool_layer
(csrc/attn_pool.hip): against the reference's own outputs and gradients (tests/golden/list_attn.npz) and, at sizes the
fixture does not hold, against nn.MultiheadAttention + pooling on the CPU (tests/list_attn_ref.py, pinned to the fixture
by tests/test_list_attn_host.py).  fp32: 1e-5 relative.  bf16: the reference is the fp32 composition on the bf16-rounded
parameters and the bound max(1e-2, 2 x e_aten), e_aten being the error of the same module with the fused path switched off
(the ATen composition in bf16) on the same inputs; the factor 2 covers a different fp32 summation order and the one extra
rounding of the pooled rows.

Worst bf16 pair measured over the grid of test_against_torch_composition: see profiles/attn_pool_kernels.md."""
import pytest
import torch

from conftest import rel_err
from list_attn_ref import ATTN_KEYS, ATTN_SHAPES, attn_tag, make_attention, mha_compose, reference_grads

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


class _Spy:
    """counts the calls of functional.attn_pool (there is no CPU fallback to hide behind)"""

    def __init__(self, monkeypatch):
        from torecsys_amd import functional as F_
        self.calls, real = 0, F_.attn_pool

        def spy(*a, **k):
            self.calls += 1
            return real(*a, **k)

        monkeypatch.setattr(F_, "attn_pool", spy)


def _module(dev, E, V, H, method, attn, w, dtype=torch.float32, **kw):
    """the module on the device holding the table ``w`` and the parameters of the CPU attention ``attn``"""
    from torecsys_amd.inputs import ListIndicesEmbedding
    m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method, use_attn=True, num_heads=H,
                             bias=attn.in_proj_bias is not None, **kw)
    sd = {"embedding.weight": w}
    sd.update({"attention." + k: p.detach() for k, p in attn.named_parameters()})
    m.load_state_dict(sd)
    return m.to(dev).to(dtype)


def _grads(m):
    return {k: p.grad for k, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("shape", ATTN_SHAPES, ids=attn_tag)
def test_fixture_parity_through_the_module(golden, dev, monkeypatch, shape):
    from torecsys_amd.inputs import ListIndicesEmbedding
    G = golden("list_attn")
    B, L, E, V, H, bias = shape
    pre = attn_tag(shape)
    spy = _Spy(monkeypatch)
    m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method="avg_pooling", use_attn=True, num_heads=H,
                             bias=bias).to(dev)
    assert list(m.state_dict().keys()) == G(pre + "/keys")
    m.load_state_dict({k: G(f"{pre}/param/{k}") for k in G(pre + "/keys")})
    out = m(G(pre + "/idx").to(dev))
    assert spy.calls == 1
    assert out.names == tuple(G(pre + "/names")) == ("B", "N", "E")
    y = out.rename(None)
    assert tuple(y.shape) == (B, 1, E)
    assert rel_err(y.cpu(), G(pre + "/out")) <= TOL32
    (y * G(pre + "/gout").to(dev)).sum().backward()
    for k, p in m.named_parameters():
        assert rel_err(p.grad.cpu(), G(f"{pre}/grad/{k}")) <= TOL32, k
    assert float(m.embedding.weight.grad[0].abs().max()) == 0.0          # the padding row: exactly zero


# ------------------------------------------------------------------------------------------------ the torch composition
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("L", [1, 5, 33, 50, 64])
@pytest.mark.parametrize("E,H", [(64, 1), (64, 4), (128, 8), (16, 2), (10, 5)])
@pytest.mark.parametrize("dtype,idt", [(torch.float32, torch.int64), (torch.float32, torch.int32),
                                       (torch.bfloat16, torch.int64), (torch.bfloat16, torch.int32)])
def test_against_torch_composition(dev, monkeypatch, dtype, idt, E, H, L, mode):
    """B = 97 (several workgroups, an odd count), Zipf ids with 60 % padding:
    the output, the table gradient and the gradients of all four attention parameters"""
    from torecsys_amd import functional as F_
    from torecsys_amd import inputs as I
    B, V = 97, 300
    g = torch.Generator().manual_seed(4321 + L * 7 + E + H)
    idx = _zipf_bags(g, B, L, V, 0.6)
    w = (torch.randn(V, E, generator=g) * 0.5).to(dtype).float()
    attn = make_attention(E, H, True, generator=g)
    with torch.no_grad():
        for p in attn.parameters():
            p.copy_(p.to(dtype).float())                                  # the rounded parameters are THE parameters
    gout = torch.randn(B, 1, E, generator=g).to(dtype).float()
    want_y, want = reference_grads(lambda w_, a: mha_compose(w_, idx, a, mode, padding_idx=0), w, attn, gout)
    want = {k: v.clone() for k, v in want.items()}
    assert F_.attn_pool_path(L, E, H, dtype) == (2 if dtype == torch.bfloat16 and E % 16 == 0 and (E // H) % 16 == 0
                                                 else 1)

    def run(fused):
        monkeypatch.setattr(I, "ATTN_POOL", fused)
        spy = _Spy(monkeypatch)
        m = _module(dev, E, V, H, mode, attn, w, dtype)
        y = m(idx.to(dev).to(idt)).rename(None)
        assert spy.calls == (1 if fused else 0)
        assert tuple(y.shape) == (B, 1, E) and y.dtype == dtype
        (y * gout.to(dev).to(dtype)).sum().backward()
        errs = {"out": rel_err(y.float().cpu(), want_y)}
        for k, p in m.named_parameters():
            errs[k] = rel_err(p.grad.float().cpu(), want[k])
        assert float(m.embedding.weight.grad[0].abs().max()) == 0.0
        return errs

    got = run(True)
    assert sorted(got) == sorted(["out", "embedding.weight"] + ATTN_KEYS)
    if dtype == torch.float32:
        for k, e in got.items():
            assert e <= TOL32, (k, e)
        return
    aten = run(False)
    for k in got:
        print(f"bf16 L={L} E={E} H={H} {mode} {k}: fused {got[k]:.3e} aten {aten[k]:.3e}")
    for k in got:
        assert got[k] <= max(TOLBF, 2 * aten[k]), (k, got[k], aten[k])


def test_several_samples_per_workgroup_and_reproducible_bits(dev, monkeypatch):
    """every persistent workgroup handles at least four samples: the per-workgroup weight-gradient partials accumulate
    across them; a second call on the same inputs gives the same bits for in_proj_weight / in_proj_bias"""
    from torecsys_amd import _abi
    L, E, H, V = 5, 16, 2, 200
    blocks = _abi.size_query("trs_attn_pool_blocks", 20000, L, E, H, _abi.TRS_F32, 1)
    B = 20000 if 20000 >= 4 * blocks else 4 * blocks + 3
    assert 1 <= blocks and B >= 4 * blocks
    g = torch.Generator().manual_seed(17)
    idx = _zipf_bags(g, B, L, V, 0.6)
    w = torch.randn(V, E, generator=g) * 0.5
    attn = make_attention(E, H, True, generator=g)
    gout = torch.randn(B, 1, E, generator=g)
    want_y, want = reference_grads(lambda w_, a: mha_compose(w_, idx, a, "mean", padding_idx=0), w, attn, gout)
    spy = _Spy(monkeypatch)
    res = []
    for _ in range(2):
        m = _module(dev, E, V, H, "avg_pooling", attn, w)
        y = m(idx.to(dev)).rename(None)
        (y * gout.to(dev)).sum().backward()
        assert rel_err(y.cpu(), want_y) <= TOL32
        for k, p in m.named_parameters():
            assert rel_err(p.grad.cpu(), want[k]) <= TOL32, k
        res.append((m.attention.in_proj_weight.grad.clone(), m.attention.in_proj_bias.grad.clone()))
    assert spy.calls == 2
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][0][:2 * E].abs().max()) > 0


def test_forward_peak_allocation(dev):
    """B = 4096, L = 50, E = 64, H = 2, bf16: everything the forward allocates -- the output and what it keeps for the
    backward included -- stays below half the (B, L, E) block"""
    from torecsys_amd import functional as F_
    B, L, E, H, V = 4096, 50, 64, 2, 5000
    g = torch.Generator().manual_seed(23)
    idx = _zipf_bags(g, B, L, V, 0.3).to(dev)
    attn = make_attention(E, H, True, generator=g)
    m = _module(dev, E, V, H, "avg_pooling", attn, torch.randn(V, E, generator=g) * 0.5, torch.bfloat16)
    m(idx)                                               # warm-up: streams, the flag, the kernels' one-time queries
    F_.clear_caches()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = m(idx)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    block = B * L * E * 2
    print(f"forward peak allocation {peak / 2**20:.2f} MiB, (B,L,E) block {block / 2**20:.2f} MiB")
    assert tuple(y.shape) == (B, 1, E) and y.requires_grad
    assert peak < block / 2


# ------------------------------------------------------------------------------------------------ out-of-range ids
def test_out_of_range_id(dev, monkeypatch):
    """An id outside [0, V) reads as a zero row and contributes no gradient elsewhere; the lazy flag reports it; with
    CHECK_INDICES the call raises like nn.Embedding."""
    from torecsys_amd import functional as F_
    V, E, H = 20, 16, 2
    g = torch.Generator().manual_seed(31)
    w = torch.randn(V, E, generator=g)
    attn = make_attention(E, H, True, generator=g)
    bad = torch.tensor([[1, V + 5, 3, 0], [4, 4, -3, 0]])
    w_ext = torch.cat([w, torch.zeros(1, E)])             # row V: what an out-of-range lookup reads as
    ref_idx = torch.where((bad < 0) | (bad >= V), torch.full_like(bad, V), bad)
    gout = torch.randn(2, 1, E, generator=g)
    ap = {k: p.detach().to(dev).requires_grad_() for k, p in attn.named_parameters()}
    torch.cuda.synchronize()
    F_.index_errors_seen()                                   # clear
    for mode in ("sum", "mean"):
        want_y, want = reference_grads(lambda w_, a: mha_compose(w_, ref_idx, a, mode), w_ext, attn, gout)
        assert F_.index_errors_seen() is False
        wd = w.to(dev).requires_grad_()
        y = F_.attn_pool_layer(wd, bad.to(dev), ap["in_proj_weight"], ap["in_proj_bias"], ap["out_proj.weight"],
                               ap["out_proj.bias"], H, mode)
        assert rel_err(y.cpu(), want_y) <= TOL32
        assert F_.index_errors_seen() is True
        (y * gout.to(dev)).sum().backward()
        torch.cuda.synchronize()
        assert rel_err(wd.grad.cpu(), want["embedding.weight"][:V]) <= TOL32      # nothing leaks into another row
        for k, p in ap.items():
            assert rel_err(p.grad.cpu(), want["attention." + k]) <= TOL32, k
            p.grad = None
        F_.index_errors_seen()
    monkeypatch.setattr(F_, "CHECK_INDICES", True)
    with pytest.raises(IndexError):
        F_.attn_pool(w.to(dev), bad.to(dev), ap["in_proj_weight"][:2 * E].detach(), None, H, "sum")
    monkeypatch.setattr(F_, "CHECK_INDICES", False)
    torch.cuda.synchronize()
    F_.index_errors_seen()


# ------------------------------------------------------------------------------------------------ fused optimizers
@pytest.mark.parametrize("kind", ["sgd", "adagrad"])
def test_fused_sparse_optimizer_equals_dense_step(dev, monkeypatch, kind):
    """three steps with the table stepped by the fused sparse optimizer inside the backward against the same steps with
    the dense torch optimizer of the same kind on the table's dense gradient; the attention parameters take plain SGD in
    both runs.  (Not Adagrad: the gradient of the key bias is mathematically zero -- softmax ignores a shift of a row of
    scores -- so what arrives is rounding noise of ~1e-9, and Adagrad divides it by its own magnitude into steps of +-lr
    whose signs no two runs share; measured 5e-2 between two runs of this test that differ only in the table's
    optimizer.)"""
    from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseSGD
    B, L, E, V, H = 1024, 12, 16, 300, 2
    g = torch.Generator().manual_seed(11)
    batches = [_zipf_bags(g, B, L, V, 0.4).to(dev) for _ in range(3)]
    w0 = torch.randn(V, E, generator=g)
    attn = make_attention(E, H, True, generator=g)
    lr = 0.05
    spy = _Spy(monkeypatch)
    res = []
    for fused in (False, True):
        m = _module(dev, E, V, H, "avg_pooling", attn, w0)
        opts = [torch.optim.SGD(m.attention.parameters(), lr=lr)]
        if fused:
            m.set_fused_optimizer(FusedSparseSGD(lr) if kind == "sgd" else FusedSparseAdagrad(lr, eps=1e-10))
        else:
            table = [m.embedding.weight]
            opts.append(torch.optim.SGD(table, lr=lr) if kind == "sgd" else torch.optim.Adagrad(table, lr=lr, eps=1e-10))
        for idx in batches:
            loss = (m(idx).rename(None) ** 2).mean()
            for opt in opts:
                opt.zero_grad()
            loss.backward()
            for opt in opts:
                opt.step()
            if fused:
                assert m.embedding.weight.grad is None
        res.append({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    assert spy.calls == 6
    for k in res[0]:
        assert rel_err(res[1][k], res[0][k]) <= TOL32, k
    assert not torch.equal(res[1]["embedding.weight"], w0)
    assert torch.equal(res[1]["embedding.weight"][0], w0[0])      # the padding row is never updated
    assert not torch.equal(res[1]["attention.in_proj_weight"], attn.in_proj_weight.detach())


# ------------------------------------------------------------------------------------------------ hipGraph capture
def test_graphed_forward_backward_matches_eager(dev, monkeypatch):
    from torecsys_amd.graph import GraphedStep
    B, L, E, V, H = 512, 20, 32, 400, 2
    g = torch.Generator().manual_seed(3)
    attn = make_attention(E, H, True, generator=g)
    m = _module(dev, E, V, H, "avg_pooling", attn, torch.randn(V, E, generator=g))
    params = list(m.parameters())
    proj = torch.randn(1, 1, E, generator=g).to(dev)
    batches = [(_zipf_bags(g, B, L, V, 0.5).to(dev), torch.randn(B, 1, generator=g).to(dev)) for _ in range(3)]
    spy = _Spy(monkeypatch)

    def fn(ix, lab):
        loss = (((m(ix).rename(None) * proj).sum(-1) - lab) ** 2).mean()
        loss.backward()
        return loss

    eager = []
    for ix, lab in batches:
        for p in params:
            p.grad = None
        loss = fn(ix, lab)
        eager.append((loss.detach().clone(), [p.grad.clone() for p in params]))
    del loss
    assert spy.calls == 3
    step = GraphedStep(fn, batches[0], params=params, warmup=2)
    for (ix, lab), (l0, g0) in zip(batches, eager):
        loss = step(ix, lab)
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), l0)
        for p, gp in zip(params, g0):
            assert rel_err(p.grad.cpu(), gp.cpu()) <= TOL32


# ------------------------------------------------------------------------------------------------ what keeps the composition
@pytest.mark.parametrize("case", ["max_pooling", "none", "dropout_training", "add_zero_attn", "L65", "switched_off"])
def test_cases_outside_the_fused_path_keep_the_composition(dev, monkeypatch, case):
    from torecsys_amd import functional as F_
    from torecsys_amd import inputs as I
    B, E, V, H = 33, 16, 50, 2
    L = 65 if case == "L65" else 9
    method = case if case in ("max_pooling", "none") else "avg_pooling"
    kw = {"dropout": 0.5} if case == "dropout_training" else {"add_zero_attn": True} if case == "add_zero_attn" else {}
    g = torch.Generator().manual_seed(41)
    idx = _zipf_bags(g, B, L, V, 0.4)
    w = torch.randn(V, E, generator=g)
    from torecsys_amd.inputs import ListIndicesEmbedding
    m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method, use_attn=True, num_heads=H, **kw)
    with torch.no_grad():
        m.embedding.weight.copy_(w)
    m = m.to(dev)
    if case == "switched_off":
        monkeypatch.setattr(I, "ATTN_POOL", False)
    spy = _Spy(monkeypatch)
    torch.manual_seed(5)
    out = m(idx.to(dev))
    assert spy.calls == 0 and out.names == ("B", "N", "E")
    # today's path, written out on the device: gather -> the module's own attention -> pooling
    torch.manual_seed(5)
    seq = F_.gather_rows(m.embedding.weight, idx.to(dev), None, 0).transpose(0, 1)
    seq, _ = m.attention(seq, seq, seq)
    blk = seq.transpose(0, 1)
    want = {"max_pooling": lambda: blk.max(dim=1, keepdim=True)[0], "none": lambda: blk}.get(
        method, lambda: blk.mean(dim=1, keepdim=True))()
    assert torch.equal(out.rename(None), want)
    if case != "dropout_training":
        cpu = m.attention.__class__(E, H, **kw)
        cpu.load_state_dict({k: v.cpu() for k, v in m.attention.state_dict().items()})
        ref = mha_compose(w, idx, cpu, {"max_pooling": "max", "none": "none"}.get(method, "mean"), padding_idx=0)
        assert rel_err(out.rename(None).cpu(), ref) <= TOL32
    else:
        m.eval()                                          # dropout is inactive in eval mode: the fused path serves it
        m(idx.to(dev))
        assert spy.calls == 1

"""GPU: fused sparse optimizers with their per-step scalars on the device (``capturable=True``): eager parity with the
by-value optimizers, hipGraph replays (unsharded and on the owner side of a large row-sharded table, which compacts its
touched rows on the device), a learning-rate change between replays, and the refusal a non-capturable Adam keeps."""
import gc
import os
import socket

import pytest
import torch
import torch.distributed as dist

from conftest import rel_err
from torecsys_amd.functional import compact_rows          # noqa: F401  (absent before this feature: collection fails)
from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseAdam, FusedSparseSGD

FusedSparseSGD(0.1, capturable=True)                      # the keyword itself: a TypeError at collection without it

pytestmark = pytest.mark.gpu

B, N, E = 700, 12, 64
FS = [40 + 5 * i for i in range(N)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pg():
    assert torch.cuda.is_available()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    yield
    dist.destroy_process_group()


def make_opt(kind, capturable, lr=None):
    if kind == "sgd":
        return FusedSparseSGD(0.05 if lr is None else lr, capturable=capturable)
    if kind == "adagrad":
        return FusedSparseAdagrad(0.05 if lr is None else lr, capturable=capturable)
    return FusedSparseAdam(0.01 if lr is None else lr, betas=(0.9, 0.999), capturable=capturable)


def batches_of(n, seed, fs=FS, b=B):
    g = torch.Generator().manual_seed(seed)
    return [torch.cat([torch.randint(0, f, (b, 1), generator=g) for f in fs], 1) for _ in range(n)]


def unsharded(W, opt, dev, dtype=torch.float32):
    from torecsys_amd.inputs import MultiIndicesEmbedding
    m = MultiIndicesEmbedding(embed_size=W.shape[1], field_sizes=FS).to(dev).to(dtype)
    m.embedding.weight.data.copy_(W)
    m.set_fused_optimizer(opt)
    return m


def fm_step(m, gb):
    """forward + backward of the loss used by test_gpu_dist.py::test_sharded_step_is_capturable"""
    from torecsys_amd.layers import FMLayer
    fm = FMLayer()

    def fn(ix):
        out = m(ix)
        loss = (out.rename(None).float() * gb).sum() + (fm(out).rename(None).float() ** 2).sum() * 1e-3
        loss.backward()
        return loss
    return fn


@pytest.mark.parametrize("kind,dtype,tol", [("sgd", torch.float32, 1e-6), ("adagrad", torch.float32, 1e-6),
                                            ("adam", torch.float32, 1e-6), ("adam", torch.bfloat16, 1e-2)])
def test_capturable_equals_by_value_eagerly(dev, kind, dtype, tol):
    """four eager steps, the step size read from device memory against passed by value.  fp32: both compute it in double
    and round once to fp32 (the device reads an fp32 learning rate), at most ~1 fp32 ulp of the UPDATE apart, which is
    itself <= lr / max|w| of the table: 1e-6 leaves an order of magnitude.  bf16 table: the project's bf16 bound."""
    g = torch.Generator().manual_seed(21)
    W = torch.randn(sum(FS), E, generator=g).to(dtype)
    gb = torch.randn(B, N, E, generator=g).to(dev)
    tables = []
    for capturable in (False, True):
        opt = make_opt(kind, capturable)
        m = unsharded(W, opt, dev, dtype)
        fn = fm_step(m, gb)
        for ix in batches_of(4, 22):
            fn(ix.to(dev))
            assert m.embedding.weight.grad is None
        tables.append(m.embedding.weight.detach().float().clone())
        if kind == "adam":
            assert opt.state_dict(m.named_parameters())["tables"]["embedding.weight"]["step"] == 4
    err = rel_err(tables[1], tables[0])
    print(f"capturable vs by-value {kind} {dtype}: rel_err {err:.3e}")
    assert err <= tol
    assert not torch.equal(tables[0], W.float().to(dev))


def test_capturable_adam_equals_torch_sparse_adam(dev):
    """as tests/test_gpu_embedding.py::test_fused_sparse_adam_equals_torch_sparse_adam, at its fp32 bound: the capturable
    FusedSparseAdam == torch.optim.SparseAdam fed the coalesced sparse gradient of the same lookups, four steps"""
    from torecsys_amd.inputs import MultiIndicesEmbedding
    g = torch.Generator().manual_seed(31)
    W = torch.randn(sum(FS), E, generator=g)
    gb = torch.randn(B, N, E, generator=g).to(dev)
    lr, betas, eps = 0.01, (0.9, 0.99), 1e-8
    off = torch.tensor([0] + list(torch.tensor(FS).cumsum(0)[:-1]), device=dev)
    fused = unsharded(W, FusedSparseAdam(lr, betas=betas, eps=eps, capturable=True), dev)
    plain = MultiIndicesEmbedding(embed_size=E, field_sizes=FS).to(dev)
    plain.embedding.weight.data.copy_(W)
    master = torch.nn.Parameter(W.to(dev).clone())
    ref_opt = torch.optim.SparseAdam([master], lr=lr, betas=betas, eps=eps)
    fn_f, fn_p = fm_step(fused, gb), fm_step(plain, gb)
    for ix in batches_of(4, 32):
        ix = ix.to(dev)
        fn_f(ix)
        plain.embedding.weight.grad = None
        fn_p(ix)
        rows = (ix + off.view(1, -1)).reshape(-1).unique()
        G = plain.embedding.weight.grad
        master.grad = torch.sparse_coo_tensor(rows.unsqueeze(0), G[rows], size=G.shape)
        ref_opt.step()
        plain.embedding.weight.data.copy_(master.data)
    err = rel_err(fused.embedding.weight.detach(), master.detach())
    print(f"capturable Adam vs torch SparseAdam: rel_err {err:.3e}")
    assert err <= 1e-5
    assert not torch.equal(master.detach().cpu(), W)


def test_capturable_adam_replays_unsharded(dev):
    """GraphedStep around lookup + FM + backward with FusedSparseAdam(capturable=True): the warm-up step is step 1, four
    replays on fresh batches are steps 2..5; after every one the table is where an eager by-value Adam leaves it, and
    the device step counter reads 5 at the end."""
    from torecsys_amd.graph import GraphedStep
    g = torch.Generator().manual_seed(41)
    W = torch.randn(sum(FS), E, generator=g)
    gb = torch.randn(B, N, E, generator=g).to(dev)
    batches = [b.to(dev) for b in batches_of(5, 42)]
    m_e = unsharded(W, make_opt("adam", False), dev)
    fn_e = fm_step(m_e, gb)
    eager = []
    for ix in batches:
        fn_e(ix)
        eager.append(m_e.embedding.weight.detach().clone())
    opt = make_opt("adam", True)
    m_g = unsharded(W, opt, dev)
    step = GraphedStep(fm_step(m_g, gb), (batches[0],), params=[], warmup=1)
    assert rel_err(m_g.embedding.weight.detach(), eager[0]) <= 1e-5          # the warm-up stepped once, the capture did not
    for k, ix in enumerate(batches[1:], 1):
        step(ix)
        torch.cuda.synchronize()
        err = rel_err(m_g.embedding.weight.detach(), eager[k])
        print(f"replayed Adam step {k + 1}: rel_err {err:.3e}")
        assert err <= 1e-5
    assert opt.state_dict(m_g.named_parameters())["tables"]["embedding.weight"]["step"] == 5
    step.release_outputs()


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_set_lr_between_replays_needs_no_recapture(dev, kind):
    """set_lr(lr / 10) between two replays: the second replay equals an eager by-value run that changed lr at the same
    point (and is far from one that did not)"""
    from torecsys_amd.graph import GraphedStep
    g = torch.Generator().manual_seed(51)
    W = torch.randn(sum(FS), E, generator=g)
    gb = torch.randn(B, N, E, generator=g).to(dev)
    batches = [b.to(dev) for b in batches_of(3, 52)]
    lr = make_opt(kind, False).lr
    eager = {}
    for change in (True, False):
        opt_e = make_opt(kind, False)
        m_e = unsharded(W, opt_e, dev)
        fn_e = fm_step(m_e, gb)
        fn_e(batches[0])
        fn_e(batches[1])
        after_1 = m_e.embedding.weight.detach().clone()
        if change:
            opt_e.set_lr(lr / 10)
        fn_e(batches[2])
        eager[change] = (after_1, m_e.embedding.weight.detach().clone())
    opt = make_opt(kind, True)
    m_g = unsharded(W, opt, dev)
    step = GraphedStep(fm_step(m_g, gb), (batches[0],), params=[], warmup=1)
    step(batches[1])
    torch.cuda.synchronize()
    assert rel_err(m_g.embedding.weight.detach(), eager[True][0]) <= 1e-5
    opt.set_lr(lr / 10)
    assert opt.lr == lr / 10
    step(batches[2])
    torch.cuda.synchronize()
    err = rel_err(m_g.embedding.weight.detach(), eager[True][1])
    print(f"replay after set_lr ({kind}): rel_err {err:.3e}")
    assert err <= 1e-5
    assert rel_err(eager[False][1], eager[True][1]) > 1e-4          # the comparison can tell the two learning rates apart
    step.release_outputs()


@pytest.mark.parametrize("capacity", [1.25, None])
@pytest.mark.parametrize("kind", ["adagrad", "adam"])
def test_large_shard_step_replays(pg, kind, capacity):
    """The body of test_gpu_dist.py::test_sharded_step_is_capturable on the LARGE-shard branch (dense_grad_max_rows=0:
    compact_rows -> row buckets over the slots -> mapped update) with a capturable Adagrad / Adam, with padding slots
    (capacity=1.25) and without: replays on fresh batches leave the table where the eager steps leave it, with other
    device work allocated and freed in between.  Both runs step once on the first batch (the warm-up of the capture)
    and restart from the initial weights with the optimizer state that step left."""
    from torecsys_amd.dist import RowShardedMultiIndicesEmbedding
    from torecsys_amd.graph import GraphedStep
    from torecsys_amd.layers import FMLayer
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    fs = [60 + 7 * i for i in range(12)]
    Bs, Ns, Es = 2048, 12, 64
    W = torch.randn(sum(fs), Es, generator=g)
    batches = [torch.cat([torch.randint(0, f, (Bs, 1), generator=g) for f in fs], 1).to(dev) for _ in range(4)]
    gb = torch.randn(Bs, Ns, Es, generator=g).to(dev)
    kw = {} if capacity is None else {"capacity": capacity}

    def make():
        m = RowShardedMultiIndicesEmbedding(embed_size=Es, field_sizes=fs, fuse_fm=True, dtype=torch.float32, device=dev,
                                            dense_grad_max_rows=0, **kw)
        m.load_full_weight(W.to(dev))
        m.set_fused_optimizer(make_opt(kind, True, lr=1e-3))
        fm = FMLayer()

        def fn(ix):
            out = m(ix)
            loss = (out.rename(None) * gb).sum() + (fm(out).rename(None) ** 2).sum() * 1e-3
            loss.backward()
            return loss
        return m, fn

    m_e, fn_e = make()
    fn_e(batches[0])
    m_e.load_full_weight(W.to(dev))
    eager = []
    for ix in batches:
        fn_e(ix)
        eager.append(m_e.embedding.weight.detach().clone())
    m_g, fn_g = make()
    step = GraphedStep(fn_g, (batches[0],), params=[], warmup=1)
    m_g.load_full_weight(W.to(dev))
    for k, (ix, w0) in enumerate(zip(batches, eager)):
        step(ix)
        torch.cuda.synchronize()
        err = rel_err(m_g.embedding.weight.detach(), w0)
        print(f"large-shard replay {kind} capacity={capacity} step {k + 1}: rel_err {err:.3e}")
        assert err <= 1e-5
        churn = [torch.full((Bs * Ns,), 2 ** 31 - 5, dtype=torch.int32, device=dev) for _ in range(4)]
        churn += [torch.randn(sum(fs), Es, device=dev).double() * 1e30 for _ in range(4)]
        torch.cuda.synchronize()
        del churn
    assert not torch.equal(m_g.embedding.weight.detach().cpu()[: W.shape[0]], W)
    step.release_outputs()


def test_by_value_adam_still_refuses_capture(dev):
    """capturable=False keeps today's behaviour: a capture that meets FusedSparseAdam raises, with the existing message"""
    from torecsys_amd import functional as F_
    from torecsys_amd.graph import GraphedStep
    g = torch.Generator().manual_seed(61)
    W = torch.randn(sum(FS), E, generator=g)
    gb = torch.randn(B, N, E, generator=g).to(dev)
    ix = batches_of(1, 62)[0].to(dev)
    m = unsharded(W, make_opt("adam", False), dev)
    fn = fm_step(m, gb)
    with pytest.raises(RuntimeError, match="FusedSparseAdam cannot be captured into a hipGraph"):
        GraphedStep(fn, (ix,), params=[], warmup=1)
    # what the failed capture left behind (autograd graph, cache entries in the capture's private pool) goes before
    # anything else uses the device
    del fn, m
    F_.clear_caches()
    gc.collect()
    torch.cuda.synchronize()

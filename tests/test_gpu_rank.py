"""GPU parity of the pair-score and ranking-loss kernels (csrc/rank.hip) and their host mirror: against the reference's
own outputs and gradients (tests/golden/rank.npz) and, at sizes the fixture does not hold, against the plain torch
composition on the CPU (tests/rank_ref.py, pinned to the fixture by tests/test_rank_host.py).  fp32: 1e-5 relative;
bf16: 1e-2 relative against the composition evaluated in fp32 on bf16-rounded inputs; the scalar loss in ``sum_err``."""
import os
import subprocess
import sys
from functools import partial

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, sum_err
from rank_ref import RANK_SHAPES, loss_cases, rank_loss_ref, shape_tag

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
V = 50


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def fused_path(monkeypatch):
    """the tests of this file are about the kernels (the composition runs in a process of its own with TRS_PAIR_SCORE=0)"""
    from torecsys_amd import functional as F_
    monkeypatch.setattr(F_, "PAIR_SCORE", True)


@pytest.fixture
def calls(monkeypatch):
    """names of the library entries called, in order"""
    from torecsys_amd import _abi, functional as F_
    seen = []
    orig = _abi.call

    def spy(name, *args):
        seen.append(name)
        return orig(name, *args)

    monkeypatch.setattr(_abi, "call", spy)
    monkeypatch.setattr(F_, "call", spy)
    return seen


def _dt(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


# ------------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("shape", RANK_SHAPES, ids=shape_tag)
def test_layers_and_models_golden(golden, dev, shape, calls):
    from harness.emb_models import MatrixFactorizationModel, StarSpaceModel
    from torecsys_amd import layers as L
    G = golden("rank")
    B, K, E = shape
    tag = shape_tag(shape)
    x = G(f"mf/{tag}/x").to(dev).requires_grad_()
    y = L.GeneralizedMatrixFactorizationLayer()(x)
    assert y.names == ("B", "O") and tuple(y.shape) == (B, 1)
    assert rel_err(y.rename(None).cpu(), G(f"mf/{tag}/out")) <= 1e-5
    x2 = G(f"mf/{tag}/x").to(dev).requires_grad_()
    y2 = MatrixFactorizationModel()(x2)
    assert not y2.has_names() and torch.equal(y2, y.rename(None))
    (y2 * G(f"mf/{tag}/gout").to(dev)).sum().backward()
    assert rel_err(x2.grad.cpu(), G(f"mf/{tag}/gx")) <= 1e-5
    for name, sim in (("ss_dot", partial(L.inner_product_similarity, dim=2)), ("ss_cos", partial(F.cosine_similarity, dim=2))):
        c, t = G(f"{name}/{tag}/context").to(dev).requires_grad_(), G(f"{name}/{tag}/target").to(dev).requires_grad_()
        y = StarSpaceModel(E, K, sim)(c, t)
        assert tuple(y.shape) == (B * (1 + K), 1)
        assert rel_err(y.cpu(), G(f"{name}/{tag}/out")) <= 1e-5, name
        (y * G(f"{name}/{tag}/gout").to(dev)).sum().backward()
        assert rel_err(c.grad.cpu(), G(f"{name}/{tag}/gcontext")) <= 1e-5, name
        assert rel_err(t.grad.cpu(), G(f"{name}/{tag}/gtarget")) <= 1e-5, name
    assert calls.count("trs_embed_pair_score_fwd") == 4 and calls.count("trs_embed_pair_score_bwd") == 3


@pytest.mark.parametrize("shape", RANK_SHAPES, ids=shape_tag)
def test_loss_classes_golden(golden, dev, shape):
    from torecsys_amd import losses as Ls
    G = golden("rank")
    tag = shape_tag(shape)
    hinge_m, adaptive_m, triplet_m = (float(v) for v in G("loss/margins"))
    pos, neg, mask = G(f"loss/{tag}/pos"), G(f"loss/{tag}/neg"), G(f"loss/{tag}/mask")
    for name, red in loss_cases():
        mod = {"bpr": lambda: Ls.BayesianPersonalizedRankingLoss(reduction=red),
               "hinge": lambda: Ls.HingeLoss(margin=hinge_m, reduction=getattr(torch, red)),
               "adaptive": lambda: Ls.AdaptiveHingeLoss(margin=adaptive_m, reduction=getattr(torch, red)),
               "triplet": lambda: Ls.TripletLoss(margin=triplet_m, reduction=red),
               "triplet0": lambda: Ls.TripletLoss(margin=0.0, reduction=red),
               "pointwise": lambda: Ls.PointwiseLogisticLoss()}[name]()
        for mname, mk in (("nomask", None), ("mask", mask)):
            key = f"loss/{name}/{tag}/{mname}/{red}"
            p, n = pos.to(dev).requires_grad_(), neg.to(dev).requires_grad_()
            val = mod(p, n, None if mk is None else mk.to(dev))
            assert val.dtype == torch.float32 and val.dim() == 0
            # every term is >= 0: the magnitude of what was summed is the loss itself
            assert sum_err(val.detach().cpu(), G(key + "/loss"), G(key + "/loss").abs()) <= 1e-5, key
            val.backward()
            assert rel_err(p.grad.cpu(), G(key + "/gpos")) <= 1e-5, key
            assert rel_err(n.grad.cpu(), G(key + "/gneg")) <= 1e-5, key


# ------------------------------------------------------------------------------------------------ the torch composition
def _tables(g, E, dtype):
    """two (V, E) tables rounded to ``dtype``, as fp32 on the CPU"""
    return [torch.randn(V, E, generator=g).to(dtype).float() for _ in range(2)]


def _ids(g, B, K, offsets, idt):
    if offsets:      # anchors in rows [3, 23), targets in rows [25, 50) of the table
        return torch.randint(0, 20, (B,), generator=g).to(idt), torch.randint(0, 25, (B, 1 + K), generator=g).to(idt), 3, 25
    return torch.randint(0, V, (B,), generator=g).to(idt), torch.randint(0, V, (B, 1 + K), generator=g).to(idt), 0, 0


def _composition(Wa, Wt, a_idx, t_idx, a_off, t_off, sim, gout, valid=True):
    """fp32 on the CPU: scores, the (B, 2 + K, E) gradient rows, the table gradient(s) (one for a shared table)"""
    E = Wa.shape[1]
    Wt_ = Wa if Wt is None else Wt
    ai, ti = a_idx.long() + a_off, t_idx.long() + t_off
    oka, okt = (ai >= 0) & (ai < Wa.shape[0]), (ti >= 0) & (ti < Wt_.shape[0])
    a = (Wa[ai.clamp(0, Wa.shape[0] - 1)] * oka.unsqueeze(-1)).unsqueeze(1).requires_grad_()
    t = (Wt_[ti.clamp(0, Wt_.shape[0] - 1)] * okt.unsqueeze(-1)).requires_grad_()
    s = (a * t).sum(dim=2) if sim == "dot" else F.cosine_similarity(a, t, dim=2)
    (s * gout).sum().backward()
    ga_rows, gt_rows = a.grad * oka.view(-1, 1, 1), t.grad * okt.unsqueeze(-1)
    block = torch.cat([ga_rows, gt_rows], dim=1)
    ga = torch.zeros_like(Wa).index_add_(0, ai.clamp(0, Wa.shape[0] - 1), ga_rows[:, 0])
    gt = torch.zeros_like(Wt_).index_add_(0, ti.clamp(0, Wt_.shape[0] - 1).reshape(-1), gt_rows.reshape(-1, E))
    return s.detach(), block, ((ga + gt,) if Wt is None else (ga, gt))


CONFIGS = [("shared", torch.int64, False), ("shared", torch.int32, True), ("two", torch.int64, True),
           ("two", torch.int32, False)]


@pytest.mark.parametrize("sim", ["dot", "cosine"])
@pytest.mark.parametrize("E", [8, 10, 16, 64, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_dt)
def test_pair_scores_against_torch_composition(dev, dtype, E, sim):
    """scores, the (B, 2 + K, E) gradient rows and the whole table gradient(s) at B in {1, 3, 257} x K in {0, 1, 5, 33}
    (K = 33: several chunks of the walk over the targets; B = 257: more than one workgroup) for one shared table or two,
    int64 or int32 ids, with and without offsets; V = 50, so rows repeat within and across samples.  E = 10 takes the
    one-thread-per-(b, j) kernels in both dtypes, every other width a lane group of 1 .. 32 lanes."""
    from torecsys_amd import functional as F_
    assert F_.pair_score_path(E, dtype) == (0 if E == 10 else 1)
    tol = TOL[dtype]
    worst = [0.0, 0.0, 0.0]
    for B in (1, 3, 257):
        for K in (0, 1, 5, 33):
            for tables, idt, offsets in CONFIGS:
                g = torch.Generator().manual_seed(1000 * B + 10 * K + E)
                Wa, Wt = _tables(g, E, dtype)
                if tables == "shared":
                    Wt = None
                a_idx, t_idx, a_off, t_off = _ids(g, B, K, offsets, idt)
                gout = torch.randn(B, 1 + K, generator=g).to(dtype).float()
                s_ref, block_ref, grads_ref = _composition(Wa, Wt, a_idx, t_idx, a_off, t_off, sim, gout)
                wa = Wa.to(dev, dtype).requires_grad_()
                wt = None if Wt is None else Wt.to(dev, dtype).requires_grad_()
                s = F_.pair_scores(wa, a_idx.to(dev), wt, t_idx.to(dev), a_off, t_off, sim)
                assert s.dtype == dtype and tuple(s.shape) == (B, 1 + K)
                (s * gout.to(dev, dtype)).sum().backward()
                block = F_.pair_scores_backward_raw(wa.detach(), a_idx.to(dev), wa.detach() if wt is None else wt.detach(),
                                                    t_idx.to(dev), gout.to(dev, dtype), a_off, t_off, sim)
                case = (B, K, tables, idt, offsets)
                errs = [rel_err(s.float().cpu(), s_ref), rel_err(block.float().cpu(), block_ref),
                        max(rel_err(w.grad.float().cpu(), r) for w, r in zip((wa, wt), grads_ref))]
                worst = [max(a, b) for a, b in zip(worst, errs)]
                assert max(errs) <= tol, (case, errs)
    assert not F_.index_errors_seen()
    print(f"pair_scores {_dt(dtype)} E={E} {sim}: worst rel_err scores {worst[0]:.2e} rows {worst[1]:.2e} table {worst[2]:.2e}")


def test_fp32_scores_of_bf16_tables(dev):
    """out_dtype=float32: the fp32 accumulator is stored unrounded, and an fp32 gradient comes back"""
    from torecsys_amd import functional as F_
    B, K, E = 33, 5, 64
    g = torch.Generator().manual_seed(5)
    Wa, _ = _tables(g, E, torch.bfloat16)
    a_idx, t_idx, _, _ = _ids(g, B, K, False, torch.int64)
    gout = torch.randn(B, 1 + K, generator=g)
    for sim in ("dot", "cosine"):
        s_ref, _, (g_ref,) = _composition(Wa, None, a_idx, t_idx, 0, 0, sim, gout)
        w = Wa.to(dev, torch.bfloat16).requires_grad_()
        s = F_.pair_scores(w, a_idx.to(dev), None, t_idx.to(dev), sim=sim, out_dtype=torch.float32)
        assert s.dtype == torch.float32
        assert rel_err(s.cpu(), s_ref) <= 1e-5
        (s * gout.to(dev)).sum().backward()
        assert rel_err(w.grad.float().cpu(), g_ref) <= 1e-2


def test_no_grad_forward_is_one_launch(dev, calls):
    """under torch.no_grad() the forward is the score kernel alone: no id matrix, no row buckets; with grad mode on the
    buckets of the (B, 2 + K) id matrix are built once, for the one walk of a shared table"""
    from torecsys_amd import functional as F_
    g = torch.Generator().manual_seed(3)
    w = torch.randn(V, 16, generator=g).to(dev).requires_grad_()
    a_idx, t_idx = torch.randint(0, V, (9,), generator=g).to(dev), torch.randint(0, V, (9, 4), generator=g).to(dev)
    with torch.no_grad():
        s0 = F_.pair_scores(w, a_idx, None, t_idx)
    assert calls == ["trs_embed_pair_score_fwd"]
    s = F_.pair_scores(w, a_idx, None, t_idx)
    s.sum().backward()
    assert torch.equal(s.detach(), s0)
    assert calls.count("trs_csr_build") == 1 and calls.count("trs_scatter_rows") == 1
    assert calls.count("trs_embed_pair_score_bwd") == 1 and "trs_gather_rows" not in calls


def test_positive_among_the_negatives_and_a_zero_row(dev):
    """a sample whose positive id also sits among its negatives (the row's gradient is the sum of both terms), and an
    all-zero target row under the cosine: the eps clamp gives a zero score and a finite gradient, as ATen's"""
    from torecsys_amd import functional as F_
    B, K, E = 4, 3, 16
    g = torch.Generator().manual_seed(9)
    W = torch.randn(V, E, generator=g)
    W[7] = 0.0
    a_idx = torch.tensor([1, 2, 3, 4])
    t_idx = torch.tensor([[5, 5, 6, 5], [7, 8, 9, 10], [11, 7, 7, 12], [13, 14, 15, 16]])
    gout = torch.randn(B, 1 + K, generator=g)
    for sim in ("dot", "cosine"):
        s_ref, block_ref, (g_ref,) = _composition(W, None, a_idx, t_idx, 0, 0, sim, gout)
        w = W.to(dev).requires_grad_()
        s = F_.pair_scores(w, a_idx.to(dev), None, t_idx.to(dev), sim=sim)
        (s * gout.to(dev)).sum().backward()
        assert rel_err(s.cpu(), s_ref) <= 1e-5
        assert float(s[1, 0]) == 0.0 and float(s[2, 1]) == 0.0
        assert torch.isfinite(w.grad).all()
        # the zero row's cosine gradient is a / (|a| eps), 1e8 times the others': compared on its own
        rest = torch.ones(V, dtype=torch.bool)
        rest[7] = False
        assert rel_err(w.grad.cpu()[rest], g_ref[rest]) <= 1e-5
        assert rel_err(w.grad.cpu()[7], g_ref[7]) <= 1e-5
        assert rel_err(w.grad.cpu()[5], g_ref[5]) <= 1e-5


@pytest.mark.parametrize("E", [16, 10])
def test_out_of_range_ids(dev, E):
    """zero score, no gradient, flag raised; every other sample as if nothing had happened"""
    from torecsys_amd import functional as F_
    B, K = 5, 3
    g = torch.Generator().manual_seed(11)
    Wa, Wt = _tables(g, E, torch.float32)
    a_idx, t_idx, _, _ = _ids(g, B, K, False, torch.int64)
    a_idx[1] = V
    t_idx[2, 2] = -1
    t_idx[4, 0] = V + 7
    gout = torch.randn(B, 1 + K, generator=g)
    F_.index_errors_seen()
    for sim in ("dot", "cosine"):
        s_ref, block_ref, grads_ref = _composition(Wa, Wt, a_idx, t_idx, 0, 0, sim, gout)
        wa, wt = Wa.to(dev).requires_grad_(), Wt.to(dev).requires_grad_()
        s = F_.pair_scores(wa, a_idx.to(dev), wt, t_idx.to(dev), sim=sim)
        assert F_.index_errors_seen()
        assert float(s[1].abs().max()) == 0.0 and float(s[2, 2]) == 0.0 and float(s[4, 0]) == 0.0
        assert rel_err(s.cpu(), s_ref) <= 1e-5
        (s * gout.to(dev)).sum().backward()
        F_.index_errors_seen()      # the bucket build reports the same ids
        block = F_.pair_scores_backward_raw(wa.detach(), a_idx.to(dev), wt.detach(), t_idx.to(dev), gout.to(dev), sim=sim)
        assert float(block[1, 0].abs().max()) == 0.0 and float(block[2, 3].abs().max()) == 0.0
        assert float(block[4, 1].abs().max()) == 0.0
        assert rel_err(block.cpu(), block_ref) <= 1e-5
        assert rel_err(wa.grad.cpu(), grads_ref[0]) <= 1e-5 and rel_err(wt.grad.cpu(), grads_ref[1]) <= 1e-5


@pytest.mark.parametrize("tables", ["shared", "two"])
@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam"])
def test_fused_optimizer_equals_dense_gradient_plus_optimizer(dev, kind, tables):
    from torecsys_amd.fused import EmbeddingPairScorer
    from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseAdam, FusedSparseSGD
    B, K, E = 257, 5, 64
    g = torch.Generator().manual_seed(17)
    a_idx, t_idx, a_off, t_off = _ids(g, B, K, tables == "shared", torch.int64)
    gout = torch.randn(B, 1 + K, generator=g).to(dev)
    Wa, Wt = _tables(g, E, torch.float32)

    def scorer():
        m = EmbeddingPairScorer(E, V, None if tables == "shared" else V, "cosine", a_off, t_off).to(dev)
        with torch.no_grad():
            m.anchor.weight.copy_(Wa)
            if m.target is not None:
                m.target.weight.copy_(Wt)
        return m

    dense, fused = scorer(), scorer()
    opt_d = {"sgd": lambda p: torch.optim.SGD(p, lr=0.1), "adagrad": lambda p: torch.optim.Adagrad(p, lr=0.1, eps=1e-10),
             "adam": lambda p: torch.optim.SparseAdam(p, lr=0.01)}[kind]
    fused.set_fused_optimizer({"sgd": lambda: FusedSparseSGD(0.1), "adagrad": lambda: FusedSparseAdagrad(0.1, eps=1e-10),
                               "adam": lambda: FusedSparseAdam(0.01)}[kind]())
    (dense(a_idx.to(dev), t_idx.to(dev)) * gout).sum().backward()
    masters = [torch.nn.Parameter(p.detach().clone()) for p in dense.parameters()]
    for m, p in zip(masters, dense.parameters()):
        m.grad = p.grad
        if kind == "adam":      # SparseAdam wants sparse gradients: the looked-up rows of the dense one
            rows = p.grad.abs().sum(1).nonzero().reshape(-1)
            m.grad = torch.sparse_coo_tensor(rows.unsqueeze(0), p.grad[rows], size=p.shape)
    opt_d(masters).step()
    (fused(a_idx.to(dev), t_idx.to(dev)) * gout).sum().backward()
    for m, pd, pf in zip(masters, dense.parameters(), fused.parameters()):
        assert pf.grad is None
        assert rel_err(pf.detach().cpu(), m.detach().cpu()) <= 1e-5
        assert not torch.equal(pf.detach(), pd.detach())          # (the dense model's own table was not stepped)


# ------------------------------------------------------------------------------------------------ the loss kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_dt)
def test_rank_loss_on_a_strided_score_matrix(dev, dtype, calls):
    """every kind, masked and not, every reduction, on columns 0 and 1 .. K of one (B, 1 + K) matrix read in place;
    B = 257: two workgroups in the partial-sum pass, the second with one live sample"""
    from torecsys_amd import functional as F_
    B, K = 257, 33
    g = torch.Generator().manual_seed(23)
    S = (torch.randn(B, 1 + K, generator=g) * 1.5).to(dtype).float()
    mask = torch.rand(B, generator=g) < 0.7
    mask[B - 1] = True
    margin = 0.7      # not a difference of two bf16 values: no hinge argument is exactly 0
    for kind in ("pointwise", "bpr", "hinge", "adaptive_hinge"):
        for mk in (None, mask):
            for red in ("sum", "mean", "sample"):
                p, n = S[:, :1].clone().requires_grad_(), S[:, 1:].clone().requires_grad_()
                ref = rank_loss_ref(p, n, kind, margin, mk, red)
                ref.backward()
                sd = S.to(dev, dtype).requires_grad_()
                val = F_.rank_loss(sd, None, kind, margin, None if mk is None else mk.to(dev), red)
                val.backward()
                case = (kind, mk is not None, red)
                # every term is >= 0: the magnitude of what was summed is the loss itself
                assert sum_err(val.detach().cpu(), ref.detach(), ref.detach().abs()) <= 1e-5, case
                g_ref = torch.cat([p.grad, n.grad], dim=1)
                assert rel_err(sd.grad.float().cpu(), g_ref) <= TOL[dtype], case
                if mk is not None:
                    assert float(sd.grad[~mk.to(dev)].abs().max()) == 0.0
                # the same through separate operands
                pd, nd = S[:, :1].to(dev, dtype).requires_grad_(), S[:, 1:].to(dev, dtype).requires_grad_()
                val2 = F_.rank_loss(pd, nd, kind, margin, None if mk is None else mk.to(dev), red)
                val2.backward()
                assert torch.equal(val2, val)
                assert torch.equal(torch.cat([pd.grad, nd.grad], dim=1), sd.grad)
    assert set(calls) == {"trs_rank_loss_fwd", "trs_rank_loss_bwd"}


def test_all_false_mask_gives_nan(dev):
    from torecsys_amd import functional as F_
    S = torch.randn(5, 4).to(dev)
    none = torch.zeros(5, dtype=torch.bool, device=dev)
    assert torch.isnan(F_.rank_loss(S, None, "hinge", 1.0, none, "sample"))
    assert float(F_.rank_loss(S, None, "hinge", 1.0, none, "sum")) == 0.0


def test_bpr_stays_finite(dev):
    """softplus form: finite where sigmoid().log() overflows"""
    from torecsys_amd import functional as F_
    p = torch.tensor([[-200.0], [200.0]], device=dev, requires_grad=True)
    n = torch.tensor([[100.0], [-100.0]], device=dev)
    val = F_.rank_loss(p, n, "bpr")
    val.backward()
    assert float(val) == 300.0 and torch.isfinite(p.grad).all()


# ------------------------------------------------------------------------------------------------ reproducible bits
@pytest.mark.parametrize("E,dtype", [(64, torch.bfloat16), (10, torch.float32)])
def test_two_runs_give_identical_bits(dev, E, dtype):
    from torecsys_amd import functional as F_
    B, K = 257, 33
    g = torch.Generator().manual_seed(29)
    W = torch.randn(V, E, generator=g).to(dev, dtype)
    a_idx, t_idx = torch.randint(0, V, (B,), generator=g).to(dev), torch.randint(0, V, (B, 1 + K), generator=g).to(dev)
    gout = torch.randn(B, 1 + K, generator=g).to(dev, dtype)
    runs = []
    for _ in range(2):
        s = F_.pair_scores_forward_raw(W, a_idx, W, t_idx, sim="cosine")
        block = F_.pair_scores_backward_raw(W, a_idx, W, t_idx, gout, sim="cosine")
        loss, denom = F_.rank_loss_forward_raw(s, None, "bpr", 1.0, None, "mean")
        gs, _ = F_.rank_loss_backward_raw(s, None, "bpr", 1.0, None, "mean", None, denom)
        runs.append((s, block, loss, gs))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ hipGraph capture
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_graphed_step_with_a_capturable_optimizer_equals_eager(dev, kind):
    """pair_scores + rank_loss + the fused sparse step captured once and replayed on fresh batches: after every replay the
    table is where the eager by-value optimizer leaves it (the warm-up is step 1)"""
    from torecsys_amd.fused import EmbeddingPairScorer
    from torecsys_amd.graph import GraphedStep
    from torecsys_amd.losses import HingeLoss
    from torecsys_amd.optim import FusedSparseAdam, FusedSparseSGD
    B, K, E = 257, 5, 64
    g = torch.Generator().manual_seed(31)
    W = torch.randn(V, E, generator=g)
    batches = [(torch.randint(0, V, (B,), generator=g).to(dev), torch.randint(0, V, (B, 1 + K), generator=g).to(dev))
               for _ in range(4)]

    def make(capturable):
        m = EmbeddingPairScorer(E, V, None, "dot").to(dev)
        with torch.no_grad():
            m.anchor.weight.copy_(W)
        m.set_fused_optimizer(FusedSparseSGD(0.05, capturable=capturable) if kind == "sgd"
                              else FusedSparseAdam(0.01, capturable=capturable))
        loss_fn = HingeLoss(margin=1.0, reduction="mean")

        def fn(a, t):
            loss = loss_fn(m(a, t), None)
            loss.backward()
            return loss
        return m, fn

    m_e, fn_e = make(False)
    eager = []
    for a, t in batches:
        loss = fn_e(a, t)
        eager.append((loss.detach().clone(), m_e.anchor.weight.detach().clone()))
    del loss
    m_g, fn_g = make(True)
    step = GraphedStep(fn_g, batches[0], params=[], warmup=1)
    assert rel_err(m_g.anchor.weight.detach(), eager[0][1]) <= 1e-5
    for k, (a, t) in enumerate(batches[1:], 1):
        loss = step(a, t)
        torch.cuda.synchronize()
        assert abs(float(loss) - float(eager[k][0])) <= 1e-5 * abs(float(eager[k][0]))
        assert rel_err(m_g.anchor.weight.detach(), eager[k][1]) <= 1e-5, k
    step.release_outputs()


# ------------------------------------------------------------------------------------------------ the composition switch
_CHILD = r"""
import sys, torch
from torecsys_amd import _abi, functional as F_
calls = []
orig = _abi.call
def spy(name, *args):
    calls.append(name)
    return orig(name, *args)
_abi.call = spy
F_.call = spy
assert F_.PAIR_SCORE is False
d = torch.load(sys.argv[1])
dev = torch.device("cuda:0")
res = {}
for sim in ("dot", "cosine"):
    w = d["W"].to(dev).requires_grad_()
    s = F_.pair_scores(w, d["a_idx"].to(dev), None, d["t_idx"].to(dev), 3, 25, sim)
    (s * d["gout"].to(dev)).sum().backward()
    res[sim] = (s.detach().cpu(), w.grad.cpu())
assert "trs_gather_rows" in calls and not any("pair_score" in c for c in calls), calls
torch.save(res, sys.argv[2])
print("PAIR-COMPOSITION OK")
"""


def test_switch_selects_the_composition(dev, tmp_path):
    """TRS_PAIR_SCORE=0 is read at import, so the composition (HIP gather + ATen) runs in a process of its own: it calls no
    pair-score entry and meets the fp32 bound"""
    B, K, E = 33, 5, 16
    g = torch.Generator().manual_seed(37)
    (W, _) = _tables(g, E, torch.float32)
    a_idx, t_idx, a_off, t_off = _ids(g, B, K, True, torch.int64)
    gout = torch.randn(B, 1 + K, generator=g)
    src, dst = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save({"W": W, "a_idx": a_idx, "t_idx": t_idx, "gout": gout}, src)
    env = dict(os.environ, TRS_PAIR_SCORE="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _CHILD, src, dst], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "PAIR-COMPOSITION OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    res = torch.load(dst)
    for sim in ("dot", "cosine"):
        s_ref, _, (g_ref,) = _composition(W, None, a_idx, t_idx, a_off, t_off, sim, gout)
        assert rel_err(res[sim][0], s_ref) <= 1e-5 and rel_err(res[sim][1], g_ref) <= 1e-5

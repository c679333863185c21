"""GPU: FusedSparseRowWiseAdagrad -- one fp32 accumulator per table row, advanced inside the bucket walk
(csrc/scatter.hip, the RW instantiations of the vector walk; include/trs_abi.h, TRS_OPT_ROWWISE).

1. the exact step at every lane-group width (powers of two throughout: torch.equal), once through the mapped entry;
2. every bucket length of scatter_ref.LADDER, three steps, against ONE float64 step within the derived rounding bounds
   of rowwise_ref.rowwise_adagrad_step;
3. the FM-folded walks (the lean fm1 kernel and the generic one), 4. the modules, 5. the sharded owner at world size 1:
   against the dense gradient of the same path + the float64 rule, at the project's tolerances for that comparison;
6. hipGraph replays of a capturable optimizer, bit for bit against eager steps, with a set_lr in between."""
import functools
import os
import socket

import pytest
import torch
import torch.distributed as dist

import rowwise_ref as RW
import scatter_ref as R
from conftest import rel_err
from torecsys_amd.optim import FusedSparseRowWiseAdagrad

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
LR = 2.0 ** -6                      # exact in fp32


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


def _tol(dtype):
    return 1e-5 if dtype == F32 else 1e-2          # the project's bounds for fused step vs dense gradient + optimizer


def _ref_step(pre_w, pre_s, G, touched, lr, eps):
    """(w', s') float64: the float64 rule from the weights and state the device held before the step"""
    w2, s2, _, _ = RW.rowwise_adagrad_step(pre_w.cpu(), pre_s.cpu(), G.cpu().double(), touched.cpu(), R.as_f32(lr),
                                           R.as_f32(eps))
    return w2, s2


# ------------------------------------------------------------------------------------------------ 1. exact step
WIDTH_CASES = [(F32, 4 << k) for k in range(7)] + [(BF16, 8 << k) for k in range(7)]


def _exact_case(E, dtype):
    """V = 300; two rows in three are looked up, once each.  Gradient row r is +-2^(r % 4) (random signs), weights are
    integers in [-2, 2], lr = 2^-6, eps = 0, state 0: mean(G^2) = 4^k, its root 2^k, G / root = +-1."""
    V = 300
    g = torch.Generator().manual_seed(900 + E)
    w = torch.randint(-2, 3, (V, E), generator=g).double()
    touched = torch.arange(V) % 3 != 2
    rows = touched.nonzero().flatten()
    rows = rows[torch.randperm(rows.numel(), generator=g)]
    sign = torch.randint(0, 2, (V, E), generator=g).double() * 2 - 1
    k = (torch.arange(V) % 4).double()
    G = sign * (2.0 ** k).view(-1, 1)
    want_w = torch.where(touched.view(-1, 1), w - LR * sign, w)
    want_s = torch.where(touched, 4.0 ** k, torch.zeros(V, dtype=torch.float64))
    assert torch.equal(want_w.to(dtype).double(), want_w) and torch.equal(G.to(dtype).double(), G)      # representable
    # and the float64 rule says the same
    ref_w, ref_s, _, _ = RW.rowwise_adagrad_step(w.to(dtype), torch.zeros(V), torch.where(touched.view(-1, 1), G, 0 * G),
                                                 touched, LR, 0.0)
    assert torch.equal(ref_w, want_w) and torch.equal(ref_s, want_s)
    return w, G, rows, touched, want_w, want_s


@pytest.mark.parametrize("dtype,E", WIDTH_CASES, ids=["%s-E%d" % ("f32" if d == F32 else "bf16", E) for d, E in WIDTH_CASES])
def test_exact_step_at_every_lane_group_width(dev, dtype, E):
    from torecsys_amd import functional as F_
    w, G, rows, touched, want_w, want_s = _exact_case(E, dtype)
    opt = FusedSparseRowWiseAdagrad(LR, eps=0.0)
    wd = w.to(dev).to(dtype).requires_grad_()
    F_.gather_rows(wd, rows.view(-1, 1).to(dev), None, opt=opt).backward(G[rows].view(-1, 1, E).to(dev).to(dtype))
    assert wd.grad is None
    s = opt.state_for(wd, wd)
    assert s.shape == (300,) and s.dtype == torch.float32
    assert torch.equal(s.cpu().double(), want_s)                       # untouched rows: still exactly 0
    assert torch.equal(wd.detach().cpu().double(), want_w)             # untouched rows: bit for bit
    assert not F_.index_errors_seen()


@pytest.mark.parametrize("dtype,E", [(F32, 16), (BF16, 64)], ids=["f32-E16", "bf16-E64"])
def test_exact_step_through_the_mapped_entry(dev, dtype, E):
    """compact row u updates TABLE row row_map[u] and its accumulator; the two entries outside [0, V) receive gradient
    rows and move nothing"""
    from torecsys_amd import functional as F_
    w, G, rows, touched, want_w, want_s = _exact_case(E, dtype)
    V = 300
    g = torch.Generator().manual_seed(77 + E)
    P = torch.randperm(V, generator=g)
    Pinv = torch.empty(V, dtype=torch.int64)
    Pinv[P] = torch.arange(V)
    row_map = torch.cat([P, torch.tensor([V + 7, -1])]).int()
    inv = torch.cat([Pinv[rows], torch.tensor([V, V + 1])])
    g_rows = torch.cat([G[rows], torch.full((2, E), 2.0, dtype=torch.float64)])
    mix = torch.randperm(inv.numel(), generator=g)
    rb = F_.row_buckets(inv[mix].int().view(-1, 1).to(dev), None, V + 2)
    table = w.to(dev).to(dtype)
    opt = FusedSparseRowWiseAdagrad(LR, eps=0.0)
    F_.scatter_rows_update_mapped(rb, table, opt, g_rows[mix].to(dev).to(dtype), row_map.to(dev))
    s = opt.state_for(table)
    assert s.shape == (V,)
    assert torch.equal(s.cpu().double(), want_s)
    assert torch.equal(table.cpu().double(), want_w)


# ------------------------------------------------------------------------------------------------ 2. every bucket length
@functools.lru_cache(maxsize=None)
def _ladder(seed):
    fs, idx = R.bucket_ladder(R.LADDER, R.LADDER_FIELDS, seed)
    rows = R.flat_rows(fs, idx)
    return fs, idx, rows, torch.bincount(rows, minlength=sum(fs))


@functools.lru_cache(maxsize=None)
def _ladder_grad(E, step, seed):
    """integer gradient of a step and its exact row sums, shared by the dtypes and modes of a width"""
    fs, idx, rows, _ = _ladder(seed)
    B, N = idx.shape
    ge8 = R.integer_case(fs, idx, E, 40 + step)["ge"]
    return ge8, R.grad_plain(rows, sum(fs), ge8, B, N), R.scatter_sum(rows, sum(fs), R.plain_terms(ge8, B, N).abs())


@pytest.mark.parametrize("capturable", [False, True], ids=["byvalue", "capturable"])
@pytest.mark.parametrize("dtype,E", [(F32, 16), (BF16, 32)], ids=["f32-E16", "bf16-E32"])
def test_steps_at_every_bucket_length(dev, dtype, E, capturable):
    """Three steps through F_.gather_rows on the bucket ladder (seeds 1, 2, 2: rows that hold state from step 1 are not
    looked up later), steps 2 and 3 with a padding row that has 257 lookups.  The gradient G the sink receives is exact
    (integer sums), so every step is checked per element against ONE float64 step from the weights and state read back
    before it, within the bounds rowwise_ref.rowwise_adagrad_step derives (+ half a bf16 unit in the last place for a bf16
    store); the demand is 1.0 x the bound.  Rows not looked up, and the padding row: weight and state bit for bit.
    Largest observed multiples: profiles/rowwise_adagrad.md."""
    from torecsys_amd import functional as F_
    fs = _ladder(1)[0]
    V = sum(fs)
    off_d = R.field_offsets(fs).to(dev)
    eps = R.as_f32(1e-10)
    opt = FusedSparseRowWiseAdagrad(LR, eps=eps, capturable=capturable)
    F_.clear_caches()
    wd = R.integer_case(fs, _ladder(1)[1], E, 5)["w"].to(dev).to(dtype).requires_grad_()
    worst = {"w": 0.0, "state": 0.0}
    stale = 0
    for step, seed in enumerate((1, 2, 2), start=1):
        _, idx, rows, counts = _ladder(seed)
        ge8, G, abs_sum = _ladder_grad(E, step, seed)
        R.assert_exact_regime(abs_sum, [ge8], dtype)
        prow = R.row_of_length(fs, idx, 0, 257) if step > 1 else -1
        touched = R.touched_rows(rows, V, prow)
        if prow >= 0:
            G = G.clone()
            G[prow] = 0
        pre_w = wd.detach().cpu().clone()
        pre_s = opt.state_for(wd, wd).cpu().clone()
        assert pre_s.shape == (V,) and pre_s.dtype == torch.float32
        if step > 1:
            stale += int((~touched & (pre_s != 0)).sum())
        F_.gather_rows(wd, idx.to(dev), off_d, padding_idx=None if prow < 0 else prow, opt=opt).backward(
            ge8.to(dev).to(dtype))
        assert wd.grad is None
        post_w, post_s = wd.detach().cpu(), opt.state_for(wd, wd).cpu()
        assert post_w.dtype == dtype and post_s.dtype == torch.float32
        assert torch.equal(post_w[~touched], pre_w[~touched]), f"step {step}: an untouched row's weight changed"
        assert torch.equal(post_s[~touched], pre_s[~touched]), f"step {step}: an untouched row's state changed"
        ref_w, ref_s, tol_w, tol_s = RW.rowwise_adagrad_step(pre_w, pre_s, G, touched, LR, eps)
        if dtype == BF16:
            tol_w = tol_w + torch.where(touched.view(-1, 1), R.bf16_half_ulp(ref_w), torch.zeros_like(tol_w))

        def multiple(name, got, ref, tol):
            got, ref, tol = got.double().reshape(V, -1), ref.reshape(V, -1), tol.reshape(V, -1)
            ratio = (got - ref).abs() / tol.clamp_min(1e-300)
            ratio = torch.where(got == ref, torch.zeros_like(ratio), ratio)
            m = float(ratio.max())
            if not m <= 1.0:
                r, col = divmod(int(ratio.argmax()), ratio.shape[1])
                raise AssertionError(f"step {step} {name}: {m:.3g} x the derived bound at row {r} ({int(counts[r])} lookups) "
                                     f"col {col}: got {float(got[r, col])!r} reference {float(ref[r, col])!r}")
            return m
        assert torch.isfinite(post_w.float()).all() and torch.isfinite(post_s).all()
        ws, ss = multiple("weight", post_w, ref_w, tol_w), multiple("sum", post_s, ref_s, tol_s)
        print(f"rowwise-boundaries step {step}: weight {ws:.3f} x bound, state {ss:.3f} x bound")
        worst["w"], worst["state"] = max(worst["w"], ws), max(worst["state"], ss)
        assert not torch.equal(post_w[touched], pre_w[touched]) and not torch.equal(post_s[touched], pre_s[touched])
    assert stale > 500, stale
    print(f"rowwise-boundaries {'capturable' if capturable else 'by-value'} {'fp32' if dtype == F32 else 'bf16'} E={E}: "
          f"weight {worst['w']:.3f} x bound, state {worst['state']:.3f} x bound")
    assert not F_.index_errors_seen()


# ------------------------------------------------------------------------------------------------ 3. the FM-folded walks
def _zipf_idx(B, fs, g):
    cols = []
    for f in fs:
        u = torch.rand(B, 1, generator=g)
        cols.append((f * u ** 6).long().clamp_(0, f - 1))          # heavy head: the queue of hot rows is used
    return torch.cat(cols, 1)


@pytest.mark.parametrize("fm_grad", ["full", "expanded"])
@pytest.mark.parametrize("dtype,E", [(F32, 16), (BF16, 64)], ids=["f32-E16", "bf16-E64"])
def test_fm_folded_walks(dev, dtype, E, fm_grad):
    """F_.embed_fm(opt=row-wise) with a full (B,E) FM gradient (the generic walk) and with an expanded (B,1) one (the lean
    fm1 kernel), two steps on Zipf-ish indices: weights and state against the dense gradient of the same call + the
    float64 rule from the weights and state held before the step"""
    from torecsys_amd import functional as F_
    B, N = 2048, 7
    g = torch.Generator().manual_seed(31 + E)
    fs = [6 + (i % 3) for i in range(N)]
    V = sum(fs)
    off = R.field_offsets(fs)
    w0 = torch.randn(V, E, generator=g).to(dtype)
    lr, eps = 0.05, 1e-10
    opt = FusedSparseRowWiseAdagrad(lr, eps=eps)
    wf = w0.to(dev).requires_grad_()
    for step in range(2):
        idx = _zipf_idx(B, fs, g)
        ge = torch.randn(B, N, E, generator=g).to(dtype).to(dev)
        gf = torch.randn(B, E if fm_grad == "full" else 1, generator=g).to(dtype).to(dev)
        gf = gf if fm_grad == "full" else gf.expand(B, E)
        touched = R.touched_rows(R.flat_rows(fs, idx), V)
        pre_w, pre_s = wf.detach().clone(), opt.state_for(wf, wf).clone()
        wr = pre_w.clone().requires_grad_()
        emb, fm, _ = F_.embed_fm(wr, idx.to(dev), off.to(dev), None, True)
        torch.autograd.backward([emb, fm], [ge, gf])
        ref_w, ref_s = _ref_step(pre_w, pre_s, wr.grad, touched, lr, eps)
        emb, fm, _ = F_.embed_fm(wf, idx.to(dev), off.to(dev), None, True, opt=opt)
        torch.autograd.backward([emb, fm], [ge, gf])
        assert wf.grad is None
        assert opt.state_for(wf, wf).shape == (V,)
        assert rel_err(wf.detach().cpu(), ref_w) <= _tol(dtype)
        assert rel_err(opt.state_for(wf, wf).cpu(), ref_s) <= _tol(dtype)
        assert bool(touched.any()) and not torch.equal(wf.detach()[touched.to(dev)], pre_w[touched.to(dev)])
    assert not F_.index_errors_seen()


# ------------------------------------------------------------------------------------------------ 4. modules
@pytest.mark.parametrize("method", ["sum", "avg_pooling"])
def test_list_indices_embedding(dev, method):
    from torecsys_amd.inputs import ListIndicesEmbedding
    B, L, E, V = 512, 12, 16, 300
    g = torch.Generator().manual_seed(11)
    idx = (V * torch.rand(B, L, generator=g) ** 3).long().clamp_(0, V - 1)
    idx = torch.where(torch.rand(B, L, generator=g) < 0.3, torch.zeros_like(idx), idx)          # padding id 0
    w0 = torch.randn(V, E, generator=g)
    lr, eps = 0.05, 1e-10
    mods = []
    for fused in (False, True):
        m = ListIndicesEmbedding(embed_size=E, field_size=V, output_method=method).to(dev)
        m.embedding.weight.data.copy_(w0)
        opt = FusedSparseRowWiseAdagrad(lr, eps=eps)
        if fused:
            m.set_fused_optimizer(opt)
        (m(idx.to(dev)).rename(None) ** 2).mean().backward()
        mods.append((m, opt))
    touched = torch.zeros(V, dtype=torch.bool)
    touched[idx.reshape(-1)] = True
    touched[0] = False
    ref_w, ref_s = _ref_step(w0, torch.zeros(V), mods[0][0].embedding.weight.grad, touched, lr, eps)
    m, opt = mods[1]
    assert m.embedding.weight.grad is None
    s = opt.state_for(m.embedding.weight, m.embedding.weight)
    assert s.shape == (V,)
    assert rel_err(m.embedding.weight.detach().cpu(), ref_w) <= _tol(F32)
    assert rel_err(s.cpu(), ref_s) <= _tol(F32)
    assert torch.equal(m.embedding.weight.detach().cpu()[0], w0[0]) and float(s[0]) == 0.0      # the padding row
    assert not torch.equal(m.embedding.weight.detach().cpu(), w0)


def test_list_indices_embedding_refusals_are_what_they_were(dev):
    from torecsys_amd import functional as F_
    from torecsys_amd.inputs import ListIndicesEmbedding
    m = ListIndicesEmbedding(embed_size=8, field_size=10, output_method="max_pooling").to(dev)
    with pytest.raises(NotImplementedError):
        m.set_fused_optimizer(FusedSparseRowWiseAdagrad(0.1))
    idx = torch.zeros(2, 3, dtype=torch.long, device=dev)
    with pytest.raises(NotImplementedError):
        F_.bag_pool(m.embedding.weight, idx, "max", opt=FusedSparseRowWiseAdagrad(0.1))
    with pytest.raises(NotImplementedError):
        F_.bag_pool(m.embedding.weight, idx, "sum", 0, FusedSparseRowWiseAdagrad(0.1), exclude_padding=True,
                    per_sample_weights=torch.ones(2, 3, device=dev))


def test_embedding_pair_scorer(dev, monkeypatch):
    from torecsys_amd import functional as F_
    from torecsys_amd.fused import EmbeddingPairScorer
    monkeypatch.setattr(F_, "PAIR_SCORE", True)
    B, K, E, V = 257, 5, 64, 50
    g = torch.Generator().manual_seed(17)
    a_idx = torch.randint(0, V, (B,), generator=g).to(dev)
    t_idx = torch.randint(0, V, (B, 1 + K), generator=g).to(dev)
    gout = torch.randn(B, 1 + K, generator=g).to(dev)
    Wa, Wt = torch.randn(V, E, generator=g), torch.randn(V, E, generator=g)
    lr, eps = 0.1, 1e-10

    def scorer():
        m = EmbeddingPairScorer(E, V, V, "dot").to(dev)
        with torch.no_grad():
            m.anchor.weight.copy_(Wa)
            m.target.weight.copy_(Wt)
        return m

    dense, fused = scorer(), scorer()
    opt = FusedSparseRowWiseAdagrad(lr, eps=eps)
    fused.set_fused_optimizer(opt)
    (dense(a_idx, t_idx) * gout).sum().backward()
    (fused(a_idx, t_idx) * gout).sum().backward()
    for W0, ids, pd, pf in ((Wa, a_idx, dense.anchor.weight, fused.anchor.weight),
                            (Wt, t_idx, dense.target.weight, fused.target.weight)):
        touched = torch.zeros(V, dtype=torch.bool)
        touched[ids.reshape(-1).cpu()] = True
        ref_w, ref_s = _ref_step(W0, torch.zeros(V), pd.grad, touched, lr, eps)
        assert pf.grad is None
        assert opt.state_for(pf, pf).shape == (V,)
        assert rel_err(pf.detach().cpu(), ref_w) <= _tol(F32)
        assert rel_err(opt.state_for(pf, pf).cpu(), ref_s) <= _tol(F32)
        assert not torch.equal(pf.detach().cpu(), W0)


def _deepfm(dev, dt, N, E, sizes):
    from harness import ctr_models as M
    from torecsys_amd.inputs import Inputs, MultiIndicesEmbedding
    torch.manual_seed(3)
    emb = MultiIndicesEmbedding(embed_size=E, field_sizes=sizes, fuse_fm=True)
    feat = MultiIndicesEmbedding(embed_size=1, field_sizes=sizes)
    emb.set_schema(["c0"])
    feat.set_schema(["c0"])
    inputs = Inputs(schema={"emb_inputs": emb, "feat_inputs": feat}).to(dev).to(dt)
    model = M.DeepFactorizationMachineModel(E, N, [64, 32], fm_dropout_p=0.0).to(dev).to(dt)
    return inputs, model, emb, feat


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_deepfm_wide_table_rowwise_first_order_table_elementwise(dev, dt):
    """the harness DeepFM: the E-wide table steps row-wise; its first-order (E = 1) table takes the element walk, where
    the rule is element-wise Adagrad on the same (V,) state.

    The comparison (fused step against the dense gradient of a second, identically seeded model + the float64 rule) is
    only meaningful where the step is a well-conditioned function of the gradient.  The first Adagrad step is
    lr * G / (rms(G) + eps): a sign-like function, order-1 sensitive to the last bits of G wherever G is a sum that
    cancels down to the size of its own rounding error or of eps.  With N(0,1) tables of E = 32 the FM logit has a
    standard deviation near 27, the sigmoid saturates, the (p - y) / B terms of a row are either ~0 or cancel to residues
    near eps = 1e-10, and the two models sum them in different orders (the bucket build files the lookups of a row with
    atomics): the first version of this test (B = 512, fields of 3 .. 1000 rows, unscaled tables) was intermittent in
    fp32 for that reason.  Here the tables are scaled by 0.05, so the logits are O(1) and every gradient term is O(1 / B),
    and every field's column holds distinct ids, so a row's gradient is ONE term and no summation order exists.  Rows
    with many lookups under the row-wise sink are the business of the ladder and FM-walk tests above, whose gradients
    are exact or far from cancellation."""
    B, N, E = 96, 7, 32
    sizes = [130, 101, 1000, 117, 400, 97, 121]
    V = sum(sizes)
    g = torch.Generator().manual_seed(0)
    ix = torch.stack([torch.randperm(s, generator=g)[:B] for s in sizes], 1)
    lab = (torch.rand(B, 1, generator=g) < 0.3).float().to(dev)
    crit = torch.nn.BCEWithLogitsLoss()
    lr, eps = 0.05, 1e-10
    res = []
    for fused in (False, True):
        inputs, model, emb, feat = _deepfm(dev, dt, N, E, sizes)
        with torch.no_grad():
            emb.embedding.weight.mul_(0.05)
            feat.embedding.weight.mul_(0.05)
        w0 = (emb.embedding.weight.detach().cpu().clone(), feat.embedding.weight.detach().cpu().clone())
        opt = FusedSparseRowWiseAdagrad(lr, eps=eps)
        if fused:
            emb.set_fused_optimizer(opt)
            feat.set_fused_optimizer(opt)
        crit(model(**inputs({"c0": ix.to(dev)})).float(), lab).backward()
        res.append((emb, feat, opt, w0))
    touched = R.touched_rows(R.flat_rows(sizes, ix), V)
    (emb_d, feat_d, _, w0), (emb_f, feat_f, opt, w0_f) = res
    assert torch.equal(w0[0], w0_f[0]) and torch.equal(w0[1], w0_f[1])          # identically seeded copies
    for md, mf, start in ((emb_d, emb_f, w0[0]), (feat_d, feat_f, w0[1])):
        pf = mf.embedding.weight
        G = md.embedding.weight.grad.float().cpu()
        # the conditioning the docstring speaks of, checked on the reference: no looked-up row's gradient is near eps
        assert float(G.double().pow(2).mean(1).sqrt()[touched].min()) > 1e4 * eps
        ref_w, ref_s = _ref_step(start, torch.zeros(V), G, touched, lr, eps)
        assert pf.grad is None
        s = opt.state_for(pf, pf)
        assert s.shape == (V,) and s.dtype == torch.float32
        assert rel_err(pf.detach().cpu(), ref_w) <= _tol(dt)
        assert rel_err(s.cpu(), ref_s) <= _tol(dt)
        assert not torch.equal(pf.detach().cpu(), start)
        assert torch.equal(pf.detach().cpu()[~touched], start[~touched]) and not bool(s.cpu()[~touched].any())


# ------------------------------------------------------------------------------------------------ 5. sharded owner
@pytest.mark.parametrize("big_shard", [False, True])
def test_sharded_owner_world1(pg, big_shard):
    """set_fused_optimizer on the row-sharded module == the same optimizer class on the unsharded module, three steps;
    ``big_shard`` forces the compact-row path (trs_scatter_rows_update_mapped); the state is one fp32 per shard row"""
    from torecsys_amd.dist import RowShardedMultiIndicesEmbedding
    from torecsys_amd.inputs import MultiIndicesEmbedding
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(6)
    fs = [40 + 5 * i for i in range(12)]
    B, N, E = 700, 12, 64
    W = torch.randn(sum(fs), E, generator=g)
    outs = []
    for sharded in (False, True):
        if sharded:
            m = RowShardedMultiIndicesEmbedding(embed_size=E, field_sizes=fs, dtype=torch.float32, device=dev,
                                                dense_grad_max_rows=0 if big_shard else 10 ** 9)
            m.load_full_weight(W.to(dev))
        else:
            m = MultiIndicesEmbedding(embed_size=E, field_sizes=fs).to(dev)
            m.embedding.weight.data.copy_(W)
        opt = FusedSparseRowWiseAdagrad(0.05)
        m.set_fused_optimizer(opt)
        gg = torch.Generator().manual_seed(7)
        for _ in range(3):
            idx = torch.cat([torch.randint(0, f, (B, 1), generator=gg) for f in fs], 1).to(dev)
            gb = torch.randn(B, N, E, generator=gg).to(dev)
            (m(idx).rename(None) * gb).sum().backward()
            assert m.embedding.weight.grad is None
        p = m.embedding.weight
        s = opt.state_for(p.data, p)
        assert s.shape == (p.shape[0],) and len(opt._state) == 1
        outs.append((p.detach().clone(), s.clone()))
    V = sum(fs)
    assert rel_err(outs[1][0][:V], outs[0][0]) <= 1e-5
    assert rel_err(outs[1][1][:V], outs[0][1]) <= 1e-5
    assert not torch.equal(outs[0][0].cpu(), W) and bool((outs[0][1] > 0).any())


# ------------------------------------------------------------------------------------------------ 6. hipGraph
def test_graphed_step_replays_bit_for_bit_and_follows_set_lr(dev):
    """GraphedStep over MultiIndicesEmbedding + FM + backward with a capturable row-wise Adagrad: the warm-up is step 1,
    three replays on fresh batches leave weights AND state torch.equal to the eager steps of an identically seeded copy;
    after set_lr(lr / 4) a fourth replay equals the eager copy that changed its rate at the same point (and differs from
    one that did not).  Every field's column is a set of distinct ids, so a row is looked up at most once per step and its
    sum has one term: the order in which the bucket build files the lookups of a row (atomics, not fixed from run to run)
    cannot enter, and bit equality is a statement about the replay alone."""
    from torecsys_amd.graph import GraphedStep
    from torecsys_amd.inputs import MultiIndicesEmbedding
    from torecsys_amd.layers import FMLayer
    B, N, E = 96, 4, 16
    fs = [130 + 7 * i for i in range(N)]
    V = sum(fs)
    g = torch.Generator().manual_seed(41)
    W = torch.randn(V, E, generator=g)
    gb = torch.randn(B, N, E, generator=g).to(dev)
    batches = [torch.stack([torch.randperm(f, generator=g)[:B] for f in fs], 1).to(dev) for _ in range(5)]
    lr = 0.05

    def make():
        m = MultiIndicesEmbedding(embed_size=E, field_sizes=fs).to(dev)
        m.embedding.weight.data.copy_(W)
        opt = FusedSparseRowWiseAdagrad(lr, capturable=True)
        m.set_fused_optimizer(opt)
        fm = FMLayer()

        def fn(ix):
            out = m(ix)
            loss = (out.rename(None) * gb).sum() + (fm(out).rename(None) ** 2).sum() * 1e-3
            loss.backward()
            return loss
        return m, opt, fn

    def snap(m, opt):
        p = m.embedding.weight
        return p.detach().clone(), opt.state_for(p, p).clone()

    eager = {}
    for change in (True, False):
        m_e, opt_e, fn_e = make()
        trail = []
        for k, ix in enumerate(batches):
            if k == 4 and change:
                opt_e.set_lr(lr / 4)
            fn_e(ix)
            trail.append(snap(m_e, opt_e))
        eager[change] = trail
    m_g, opt_g, fn_g = make()
    step = GraphedStep(fn_g, (batches[0],), params=[], warmup=1)
    for k in (1, 2, 3):
        step(batches[k])
        torch.cuda.synchronize()
        w, s = snap(m_g, opt_g)
        assert s.shape == (V,)
        assert torch.equal(w, eager[True][k][0]), f"replay {k}: weights differ from the eager step"
        assert torch.equal(s, eager[True][k][1]), f"replay {k}: state differs from the eager step"
    opt_g.set_lr(lr / 4)
    step(batches[4])
    torch.cuda.synchronize()
    w, s = snap(m_g, opt_g)
    assert torch.equal(w, eager[True][4][0]) and torch.equal(s, eager[True][4][1])
    assert not torch.equal(eager[False][4][0], eager[True][4][0])          # the comparison can tell the two rates apart
    assert m_g.embedding.weight.grad is None
    step.release_outputs()

"""GPU: ``stochastic_rounding=True`` of the fused sparse optimizers on bf16 tables, bit for bit against the numpy
restatement of the rule (tests/sr_ref.py; the rule: include/trs_abi.h).

Every case is built so that the fp32 weight the kernel holds before the store is known EXACTLY: integer weights in
[-2, 2], an update that is a multiple of lr = 2^-12 (SGD on integer gradient sums; Adagrad, row-wise Adagrad and the first
Adam step on +-2^k gradients, where the rule's quotient is +-1), every intermediate a power of two or a short dyadic
number.  The only thing left to the kernel is the rounding of that value at element i = table_row * E + column in update t
under the seed, which the reference computes from (value, i, seed, t) alone."""
import functools

import numpy as np
import pytest
import torch

import scatter_ref as R
import sr_ref as SR
from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseAdam, FusedSparseRowWiseAdagrad, FusedSparseSGD

FusedSparseSGD(0.1, stochastic_rounding=True, seed=1)        # the keywords themselves: a TypeError at collection without them

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
LR = 2.0 ** -12
SEED = 20261021
V0 = 300


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _bits(t):
    """bit patterns of a bf16 tensor, uint16 numpy of the same shape"""
    assert t.dtype == BF16
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _expected_bits(before_bits, x64, touched, seed, t):
    """before_bits (V,E) uint16; x64 (V,E) float64 torch: the exact pre-rounding weights, which must be fp32 values;
    touched (V,) bool torch.  Touched rows get sr_bf16(x, row * E + col, seed, t), the others keep their bits."""
    V, E = x64.shape
    assert torch.equal(x64.float().double(), x64), "the pre-rounding weight is not exact in fp32"
    i = np.arange(V * E, dtype=np.int64)
    new = SR.sr_bf16(x64.float().numpy().reshape(-1), i, seed, t).reshape(V, E)
    return np.where(touched.numpy().reshape(-1, 1), new, before_bits)


def _make(kind, sr, seed=SEED, capturable=False, lr=LR):
    kw = dict(stochastic_rounding=sr, seed=seed, capturable=capturable) if sr else dict(capturable=capturable)
    if kind == "sgd":
        return FusedSparseSGD(lr, **kw)
    if kind == "adagrad":
        return FusedSparseAdagrad(lr, eps=0.0, **kw)
    if kind == "rowwise":
        return FusedSparseRowWiseAdagrad(lr, eps=0.0, **kw)
    return FusedSparseAdam(lr, betas=(0.5, 0.75), eps=0.0, **kw)


def _states(opt, p):
    st = opt._entry(p.data, p)
    return {b: st[b].detach().cpu().clone() for b in opt._buffers}


# ------------------------------------------------------------------------------------- 1. every width, every optimizer
def _exact_case(E, kind):
    """V = 300; two rows in three are looked up (the first 50 of them twice under SGD, so the sums have two terms).
    Gradient row r is +-2^(r % 4) with random signs, weights are integers in [-2, 2], state 0, eps = 0.
      SGD      w' = w - lr * G_sum
      Adagrad  s = G^2, sqrt = |G|:  w' = w - lr * sign(G)          (row-wise: mean_e G^2 = 4^k, the same)
      Adam     betas (0.5, 0.75), step 1: m = G/2, v = G^2/4, sqrt(v) = |G|/2, step size lr * sqrt(1/4) / (1/2) = lr:
               w' = w - lr * sign(G)"""
    g = torch.Generator().manual_seed(900 + E)
    w = torch.randint(-2, 3, (V0, E), generator=g).double()
    touched = torch.arange(V0) % 3 != 2
    rows = touched.nonzero().flatten()
    rows = rows[torch.randperm(rows.numel(), generator=g)]
    if kind == "sgd":
        rows = torch.cat([rows, rows[:50]])[torch.randperm(rows.numel() + 50, generator=g)]
    sign = torch.randint(0, 2, (V0, E), generator=g).double() * 2 - 1
    G = sign * (2.0 ** (torch.arange(V0) % 4).double()).view(-1, 1)
    if kind == "sgd":
        Gsum = torch.zeros(V0, E, dtype=torch.float64).index_add_(0, rows, G[rows])
        x = w - LR * Gsum
    else:
        x = w - LR * sign
    return w, G, rows, touched, x


WIDTHS = [8 << k for k in range(7)] + [1, 3, 12]
KINDS = ["sgd", "adagrad", "rowwise", "adam"]
# (row-wise Adagrad has no element walk: E = 3 and 12 are refused; E = 1 runs as element-wise Adagrad)
CASES = [(k, E) for E in WIDTHS for k in KINDS if not (k == "rowwise" and E in (3, 12))]


@pytest.mark.parametrize("kind,E", CASES, ids=["%s-E%d" % c for c in CASES])
def test_bit_for_bit_at_every_width(dev, kind, E):
    from torecsys_amd import functional as F_
    w, G, rows, touched, x = _exact_case(E, kind)
    idx = rows.view(-1, 1).to(dev)
    g_rows = G[rows].view(-1, 1, E).to(dev).to(BF16)
    res = {}
    for sr in (False, True):
        opt = _make(kind, sr)
        wd = w.to(dev).to(BF16).requires_grad_()
        before = _bits(wd)
        F_.gather_rows(wd, idx, None, opt=opt).backward(g_rows)
        assert wd.grad is None
        res[sr] = (wd, _states(opt, wd))
    # the plain optimizer rounds the same exact value to nearest: the construction is what the docstring says it is
    assert torch.equal(res[False][0].detach().cpu(), torch.where(touched.view(-1, 1), x, w).float().to(BF16))
    want = _expected_bits(before, x, touched, SEED, 1)
    got = _bits(res[True][0])
    assert np.array_equal(got, want), f"{int((got != want).sum())} elements differ from the rule"
    assert np.array_equal(got[~touched.numpy()], before[~touched.numpy()])              # untouched rows: bit for bit
    for name, s in res[True][1].items():                                                # the state the plain step leaves
        assert torch.equal(s, res[False][1][name]), name
    if E >= 8:
        assert not np.array_equal(got, _bits(res[False][0]))                            # and it is not round-to-nearest
    assert not F_.index_errors_seen()


# --------------------------------------------------------------------------------------- 2. every row-finishing path
@functools.lru_cache(maxsize=None)
def _ladder():
    fs, idx = R.bucket_ladder(R.LADDER, R.LADDER_FIELDS, 1)
    return fs, idx, R.flat_rows(fs, idx)


@functools.lru_cache(maxsize=2)
def _ladder_case(E):
    fs, idx, rows = _ladder()
    B, N = idx.shape
    V = sum(fs)
    c = R.integer_case(fs, idx, E, 1000 + E)
    w = c["w"].double()
    c["G_ge"] = R.grad_plain(rows, V, c["ge"], B, N)
    c["G_fm"] = R.grad_fm(rows, V, N, w, c["gf"])
    c["G_fm1"] = R.grad_fm(rows, V, N, w, c["gf1"])
    c["touched"] = R.touched_rows(rows, V)
    return c


def _check(name, table, before, x, touched, t=1):
    want = _expected_bits(before, x, touched, SEED, t)
    got = _bits(table)
    bad = (got != want).any(1).nonzero()[0]
    assert bad.size == 0, f"{name}: {bad.size} rows differ from the rule, first {bad[:5].tolist()}"


@pytest.mark.parametrize("E", [32, 10], ids=["E32-vec", "E10-elem"])
def test_bit_for_bit_on_the_bucket_ladder(dev, E):
    """SGD over scatter_ref.LADDER (0 .. 4097 lookups per row: short rows, queued single-chunk rows, multi-chunk rows and
    the finish kernel; on the element walk the queue and the split rows with their finish), then the FM-folded walks
    (lean fm1 and generic) and the mapped entry, whose table must equal the unmapped one."""
    from torecsys_amd import functional as F_
    fs, idx, rows = _ladder()
    B, N = idx.shape
    V = sum(fs)
    c = _ladder_case(E)
    touched = c["touched"]
    w64 = c["w"].double()
    F_.clear_caches()
    idx_d, off_d = idx.to(dev), R.field_offsets(fs).to(dev)
    w = c["w"].to(dev).to(BF16)
    before = _bits(w)
    ge, gf, gf1 = (c[k].to(dev).to(BF16) for k in ("ge", "gf", "gf1"))

    def opt():
        return FusedSparseSGD(LR, stochastic_rounding=True, seed=SEED)

    wd = w.clone().requires_grad_()
    F_.gather_rows(wd, idx_d, off_d, opt=opt()).backward(ge)
    _check("gather", wd, before, w64 - LR * c["G_ge"], touched)
    unmapped = _bits(wd)

    for name, gfm, G in (("fm-lean", gf1.expand(B, E), c["G_ge"] + c["G_fm1"]), ("fm-full", gf, c["G_ge"] + c["G_fm"])):
        wd = w.clone().requires_grad_()
        emb, fm, _ = F_.embed_fm(wd, idx_d, off_d, None, True, opt=opt())
        torch.autograd.backward([emb, fm], [ge, gfm])
        _check(name, wd, before, w64 - LR * G, touched)

    # mapped: compact row u updates table row row_map[u]; two entries point outside the table, one of them collects 300
    # gradient rows (queued and chunked like any hot row) and must move nothing
    g = torch.Generator().manual_seed(77 + E)
    K = B * N
    P = torch.randperm(V, generator=g)
    Pinv = torch.empty(V, dtype=torch.int64)
    Pinv[P] = torch.arange(V)
    row_map = torch.cat([P, torch.tensor([V + 7, -1])]).int()
    extra = torch.randint(-2, 3, (301, E), generator=g, dtype=torch.int8)
    inv = torch.cat([Pinv[rows], torch.full((300,), V), torch.tensor([V + 1])])
    mix = torch.randperm(K + 301, generator=g)
    g_rows = torch.cat([c["ge"].reshape(K, E), extra])[mix]
    rb = F_.row_buckets(inv[mix].int().view(-1, 1).to(dev), None, V + 2)
    table = w.clone()
    F_.scatter_rows_update_mapped(rb, table, opt(), g_rows.to(dev).to(BF16), row_map.to(dev))
    _check("mapped", table, before, w64 - LR * c["G_ge"], touched)
    assert np.array_equal(_bits(table), unmapped)
    torch.cuda.synchronize()
    assert not F_.index_errors_seen()


# ------------------------------------------------------------------------------------------ 3. the point of the feature
def test_small_updates_are_kept_in_expectation(dev):
    """A 4096 x 64 bf16 table of ones, every row looked up once per step with gradient 1, SGD, lr = 2^-12, 64 steps.
    Round to nearest: 1 - 2^-12 is stored as 1.0, every step, so the table never moves (passes before this feature too:
    it documents the loss).  Stochastic rounding: the table equals the reference iterated 64 times bit for bit, and its
    mean is within 6 sigma of 1 - 64 * 2^-12 = 1 - 2^-6.  sigma: below 1.0 the bf16 spacing is 2^-8, a step of 2^-12 moves
    a weight down by 2^-8 with probability 1/16, so the per-step, per-element variance is (1/16)(15/16) * 2^-16; over 64
    steps and 262144 elements the mean has sigma = sqrt(64 * (15/256) * 2^-16 / 262144) = 1.48e-5, 6 sigma = 8.9e-5.
    (The reference run gives 0.9843595.)"""
    from torecsys_amd import functional as F_
    Vt, E, steps = 4096, 64, 64
    idx = torch.arange(Vt, device=dev).view(-1, 1)
    g_rows = torch.ones(Vt, 1, E, dtype=BF16, device=dev)
    tables = {}
    for sr in (False, True):
        opt = FusedSparseSGD(LR, stochastic_rounding=sr, seed=SEED) if sr else FusedSparseSGD(LR)
        wd = torch.ones(Vt, E, dtype=BF16, device=dev).requires_grad_()
        for _ in range(steps):
            F_.gather_rows(wd, idx, None, opt=opt).backward(g_rows)
        tables[sr] = wd
    assert bool((tables[False].detach() == 1.0).all())

    i = np.arange(Vt * E, dtype=np.int64)
    ref = np.ones(Vt * E, dtype=np.float32)
    for t in range(1, steps + 1):
        x = (ref.astype(np.float64) - LR)
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
        ref = SR.bf16_bits_to_f32(SR.sr_bf16(x.astype(np.float32), i, SEED, t))
    got = _bits(tables[True]).reshape(-1)
    assert np.array_equal(got, SR.f32_to_bf16_bits_exact(ref))
    sigma = (steps * (1 / 16) * (15 / 16) * 2.0 ** -16 / (Vt * E)) ** 0.5
    assert 8.8e-5 < 6 * sigma < 8.9e-5
    mean = float(tables[True].detach().double().mean())
    print(f"mean after {steps} steps: {mean:.7f} (1 - 2^-6 = {1 - 2.0 ** -6:.7f}, 6 sigma = {6 * sigma:.2e})")
    assert abs(mean - (1 - 2.0 ** -6)) <= 8.9e-5
    assert opt.state_dict()["tables"]["table0"]["sr_t"] == steps


# ------------------------------------------------------------------------------------------------ 4. bit-stream control
def test_seed_and_counter_select_the_bits(dev):
    from torecsys_amd import functional as F_
    E = 64
    w, G, rows, touched, x = _exact_case(E, "adagrad")
    idx = rows.view(-1, 1).to(dev)
    g_rows = G[rows].view(-1, 1, E).to(dev).to(BF16)
    w0 = w.to(dev).to(BF16)

    def run(opt, wd=None):
        wd = w0.clone().requires_grad_() if wd is None else wd
        F_.gather_rows(wd, idx, None, opt=opt).backward(g_rows)
        return wd

    a = run(_make("sgd", True, seed=5))
    b = run(_make("sgd", True, seed=5))
    c = run(_make("sgd", True, seed=6))
    assert np.array_equal(_bits(a), _bits(b))                      # same seed, same counter: the same table
    assert not np.array_equal(_bits(a), _bits(c))                  # another seed
    # updates t and t + 1 of one table on identical inputs
    opt = _make("sgd", True, seed=5)
    wd = run(opt)
    first = _bits(wd).copy()
    assert np.array_equal(first, _bits(a))
    with torch.no_grad():
        wd.copy_(w0)
    second = _bits(run(opt, wd))
    assert not np.array_equal(first, second)
    xs = w - LR * G * touched.view(-1, 1)
    assert np.array_equal(second, _expected_bits(_bits(w0), xs, touched, 5, 2))


# -------------------------------------------------------------------------------------------------------- 5. capturable
def test_graph_replays_draw_fresh_bits(dev):
    """GraphedStep over lookup + backward with a capturable SGD and stochastic rounding.  The warm-up step is undone
    (table restored, device counter set back to 0), then three replays on three batches are updates 1, 2, 3: they equal
    three eager by-value steps of a fresh optimizer bit for bit, and the counter reads 3.  Every batch looks a row up at
    most once, so the order in which the bucket build files lookups cannot enter."""
    from torecsys_amd import functional as F_
    from torecsys_amd.graph import GraphedStep
    E, Bt = 32, 96
    g = torch.Generator().manual_seed(55)
    W = torch.randint(-2, 3, (V0, E), generator=g).to(BF16).to(dev)
    gb = torch.randint(-2, 3, (Bt, 1, E), generator=g).to(BF16).to(dev)
    batches = [torch.randperm(V0, generator=g)[:Bt].view(-1, 1).to(dev) for _ in range(4)]

    def make(capturable):
        p = torch.nn.Parameter(W.clone())
        opt = FusedSparseSGD(LR, capturable=capturable, stochastic_rounding=True, seed=SEED)

        def fn(ix):
            out = F_.gather_rows(p, ix, None, opt=opt)
            out.backward(gb)
            return out.detach().float().sum()
        return p, opt, fn

    p_e, opt_e, fn_e = make(False)
    trail = []
    for ix in batches[1:]:
        fn_e(ix)
        trail.append(_bits(p_e).copy())
    assert not np.array_equal(trail[0], trail[1])

    p_g, opt_g, fn_g = make(True)
    step = GraphedStep(fn_g, (batches[0],), params=[], warmup=1)
    torch.cuda.synchronize()
    counter = opt_g.next_update(p_g.data, p_g)[1]
    assert counter.dtype == torch.int64 and int(counter) == 1          # the warm-up was update 1
    with torch.no_grad():
        p_g.copy_(W)
        counter.zero_()
    for k, ix in enumerate(batches[1:]):
        step(ix)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(p_g), trail[k]), f"replay {k + 1} differs from eager update {k + 1}"
    assert int(counter) == 3
    assert opt_g.state_dict([("p", p_g)])["tables"]["p"]["sr_t"] == 3
    assert p_g.grad is None
    step.release_outputs()


def test_by_value_counter_refuses_capture(dev):
    """capturable=False passes the update number by value: a captured launch would draw the same bits at every replay, so
    the capture raises (as a by-value FusedSparseAdam does)"""
    import gc
    from torecsys_amd import functional as F_
    from torecsys_amd.graph import GraphedStep
    E = 32
    p = torch.nn.Parameter(torch.ones(V0, E, dtype=BF16, device=dev))
    gb = torch.ones(64, 1, E, dtype=BF16, device=dev)
    ix = torch.arange(64, device=dev).view(-1, 1)
    opt = FusedSparseSGD(LR, stochastic_rounding=True, seed=SEED)

    def fn(ix):
        out = F_.gather_rows(p, ix, None, opt=opt)
        out.backward(gb)
        return out.detach().float().sum()
    with pytest.raises(RuntimeError, match="capturable=True"):
        GraphedStep(fn, (ix,), params=[], warmup=1)
    # what the failed capture left behind goes before anything else uses the device
    del fn
    F_.clear_caches()
    gc.collect()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- 6. fp32 tables
@pytest.mark.parametrize("kind", KINDS)
def test_fp32_table_ignores_the_option(dev, kind):
    """random fp32 weights and gradients, two steps; every row is looked up at most once per step, so its sum has one term
    and the order in which the bucket build files lookups cannot enter: weights and state are torch.equal to the plain
    optimizer's, and the table's update counter never moved (the plain entry ran)"""
    from torecsys_amd import functional as F_
    E = 16
    g = torch.Generator().manual_seed(61)
    w = torch.randn(V0, E, generator=g)
    batches = [(torch.randperm(V0, generator=g)[:200].view(-1, 1).to(dev), torch.randn(200, 1, E, generator=g).to(dev))
               for _ in range(2)]
    out = []
    for sr in (False, True):
        opt = _make(kind, sr, lr=0.05)
        wd = w.to(dev).requires_grad_()
        for idx, g_rows in batches:
            F_.gather_rows(wd, idx, None, opt=opt).backward(g_rows)
        out.append((wd.detach().cpu(), _states(opt, wd), opt))
    assert torch.equal(out[0][0], out[1][0]) and not torch.equal(out[0][0], w)
    for name in out[0][1]:
        assert torch.equal(out[0][1][name], out[1][1][name]), name
    assert out[1][2].stochastic_rounding and out[1][2].state_dict()["tables"]["table0"]["sr_t"] == 0


# ---------------------------------------------------------------------------------------------------------- 7. modules
def _neighbours_ok(got_bits, x32):
    """every stored bf16 is one of the two bf16 neighbours of the fp32 value (the value itself where it is a bf16 value)"""
    u = x32.view(np.uint32)
    down = (u >> 16).astype(np.uint16)
    up = (down.astype(np.uint32) + (u & 0xffff != 0)).astype(np.uint16)
    return (got_bits == down) | (got_bits == up)


@pytest.mark.parametrize("module", ["multi", "list-sum"])
def test_modules_take_the_option_through_set_fused_optimizer(dev, module):
    """MultiIndicesEmbedding and ListIndicesEmbedding(sum) under FusedSparseRowWiseAdagrad(stochastic_rounding=True): the
    same step on an fp32 copy of the table (bf16-valued weights, integer output gradients: the row sums, their mean square
    and the accumulator are exact and equal in both) leaves the fp32 weight x; every updated bf16 weight must be one of
    the two bf16 neighbours of x, rows nobody looked up keep their bits, and the state equals the fp32 copy's."""
    from torecsys_amd.inputs import ListIndicesEmbedding, MultiIndicesEmbedding
    g = torch.Generator().manual_seed(71)
    E = 16
    if module == "multi":
        fs = [60 + 7 * i for i in range(4)]
        V = sum(fs)
        idx = torch.cat([torch.randint(0, f, (128, 1), generator=g) for f in fs], 1)
        gout = torch.randint(-2, 3, (128, len(fs), E), generator=g)
        off = R.field_offsets(fs)
        touched = R.touched_rows((idx + off.view(1, -1)).reshape(-1), V)

        def build(dt):
            return MultiIndicesEmbedding(embed_size=E, field_sizes=fs).to(dev).to(dt)
    else:
        V = 300
        idx = torch.randint(0, V, (128, 6), generator=g)
        idx = torch.where(torch.rand(128, 6, generator=g) < 0.3, torch.zeros_like(idx), idx)          # padding id 0
        gout = torch.randint(-2, 3, (128, E), generator=g)
        touched = R.touched_rows(idx.reshape(-1), V, padding_row=0)

        def build(dt):
            return ListIndicesEmbedding(embed_size=E, field_size=V, output_method="sum").to(dev).to(dt)
    W = torch.randn(V, E, generator=g).to(BF16)
    res = {}
    for dt in (F32, BF16):
        m = build(dt)
        m.embedding.weight.data.copy_(W)
        opt = FusedSparseRowWiseAdagrad(0.05, eps=1e-10, stochastic_rounding=True, seed=SEED)
        m.set_fused_optimizer(opt)
        (m(idx.to(dev)).rename(None) * gout.to(dev).to(dt)).sum().backward()
        p = m.embedding.weight
        assert p.grad is None
        res[dt] = (p.detach().clone(), opt.state_for(p, p).detach().cpu().clone())
    x32 = res[F32][0].cpu().numpy()
    got = _bits(res[BF16][0])
    ok = _neighbours_ok(got, x32)
    assert ok.all(), f"{int((~ok).sum())} weights are no bf16 neighbour of the fp32 step"
    tn = touched.numpy()
    assert np.array_equal(got[~tn], _bits(W)[~tn])
    assert torch.equal(res[BF16][1], res[F32][1]) and bool((res[F32][1][touched] > 0).any())
    rne = _bits(res[F32][0].to(BF16))
    assert not np.array_equal(got[tn], rne[tn])                        # some weights went the other way

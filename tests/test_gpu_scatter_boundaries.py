"""The bucket walk of csrc/scatter.hip at its thresholds, with EXACT sums.

Every case runs on one bucket ladder (scatter_ref.LADDER, N = 3 fields, B = 23 000): in every field one row receives
exactly 0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 2304,
2305, 4096 and 4097 lookups -- both sides of LONG_ROW (64), LONG_CHUNK (256: 2304 / 2305 / 4096 / 4097 lookups = 9 / 10 /
16 / 17 chunks, the finish kernel adds partials eight at a time), LONG_ROW_ELEM (32) and ELEM_SPLIT (2048).  Tables and
gradients hold integers from {-2..2}, so every term (g, g*S with |S| <= 6, w * sum g) and every partial sum is an integer
far below 2**24: the kernels' fp32 accumulators hold the true sum on any path and in any order, the staged [g*S | g] rows
are exact in bf16, and the only rounding is the final store (round to nearest even, like at::BFloat16).  The expected
gradient is therefore the float64 reference rounded once and the assertion is torch.equal over the whole table -- one
lookup lost, doubled or misplaced anywhere changes an integer.  The exactness conditions are asserted on the reference
before anything is compared (scatter_ref.assert_exact_regime)."""
import functools

import pytest
import torch

import scatter_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
# one row width per instantiation of the vector path (LOG2L = 0, 1, 2, 4, 6: 16-byte vectors per row) and the widths of
# the element path (rows that are not a power-of-two count of 16-byte vectors); ordered by E so the two dtypes of a
# width share the cached reference
WIDTHS = sorted([(F32, E, "vec") for E in (4, 8, 16, 64, 256)] + [(BF16, E, "vec") for E in (8, 16, 32, 128, 512)]
                + [(F32, E, "elem") for E in (1, 10, 12, 96)] + [(BF16, E, "elem") for E in (1, 10, 24, 96)],
                key=lambda t: (t[1], t[0] == BF16))
WIDTH_IDS = ["%s-E%d-%s" % ("f32" if d == F32 else "bf16", E, p) for d, E, p in WIDTHS]
SGD_LR = 0.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _ladder(seed):
    fs, idx = R.bucket_ladder(R.LADDER, R.LADDER_FIELDS, seed)
    rows = R.flat_rows(fs, idx)
    return fs, idx, rows, torch.bincount(rows, minlength=sum(fs))


@functools.lru_cache(maxsize=2)
def _case(E, seed=1):
    """integer operands of width E on ladder ``seed`` and the float64 references they share (both dtypes of a width)"""
    fs, idx, rows, _ = _ladder(seed)
    B, N = idx.shape
    V = sum(fs)
    c = R.integer_case(fs, idx, E, 1000 * seed + E)
    w = c["w"].double()
    c["G_ge"] = R.grad_plain(rows, V, c["ge"], B, N)
    c["G_gs"] = R.grad_plain(rows, V, c["gs"], B, N)
    c["G_fm"] = R.grad_fm(rows, V, N, w, c["gf"])
    c["G_fm1"] = R.grad_fm(rows, V, N, w, c["gf1"])
    c["G_first"] = R.grad_first(rows, V, c["g1"])
    c["S"] = R.fm_sum(rows, N, w)
    # the most any element's accumulator can see: embedding gradient and FM terms of the same lookups together
    c["worst"] = (R.scatter_sum(rows, V, R.plain_terms(c["ge"], B, N).abs())
                  + torch.maximum(R.scatter_sum(rows, V, R.fm_terms_abs(rows, N, w, c["gf"])),
                                  R.scatter_sum(rows, V, R.fm_terms_abs(rows, N, w, c["gf1"]))))
    return c


def _assert_exact(c, dtype):
    S = c["S"]
    R.assert_exact_regime(c["worst"], [c["gf"].double() * S, c["gf1"].double() * S, c["w"], c["ge"], c["gs"], c["g1"]],
                          dtype)
    R.assert_exact_regime(R.scatter_sum(_ladder(1)[2], c["w"].shape[0], c["g1"].double().reshape(-1, 1).abs()), [], dtype)


class _Fails:
    """collects every source that misses, so one run names them all; each with the bucket lengths of the wrong rows"""

    def __init__(self, counts):
        self.msgs, self.counts = [], counts

    def check(self, name, got, want64, dtype):
        want = R.rounded(want64, dtype)
        got = got.detach().cpu()
        if got.dtype != dtype or got.shape != want.shape:
            self.msgs.append(f"{name}: got {got.dtype} {tuple(got.shape)}, expected {dtype} {tuple(want.shape)}")
            return
        if torch.equal(got, want):
            return
        bad = ~(got == want)
        rows = bad.any(1).nonzero().flatten()
        lens = sorted({int(self.counts[r]) for r in rows}) if self.counts is not None else []
        ex = []
        for r in rows[:4].tolist():
            col = int(bad[r].nonzero()[0])
            ln = int(self.counts[r]) if self.counts is not None else -1
            ex.append(f"row {r} ({ln} lookups) col {col}: got {float(got[r, col])} want {float(want[r, col])}")
        self.msgs.append(f"{name}: {rows.numel()} rows differ, bucket lengths {lens[:16]}; " + "; ".join(ex))

    def done(self):
        assert not self.msgs, "\n".join(self.msgs)


def _to(t, dev, dtype):
    return t.to(dev).to(dtype)


def _gather(F_, w, idx, off, g, **kw):
    wd = w.clone().requires_grad_()
    F_.gather_rows(wd, idx, off, **kw).backward(g)
    return wd


def _embed_fm(F_, w, idx, off, ge, gf, **kw):
    wd = w.clone().requires_grad_()
    emb, fm, _ = F_.embed_fm(wd, idx, off, None, True, **kw)
    outs, grads = ([emb, fm], [ge, gf]) if ge is not None else ([fm], [gf])
    torch.autograd.backward(outs, grads)
    return wd


@pytest.mark.parametrize("dtype,E,path", WIDTHS, ids=WIDTH_IDS)
def test_gradient_is_the_exact_sum_at_every_bucket_length(dev, dtype, E, path):
    """Every gradient source of the walk, through the public wrappers, against the rounded exact reference over the whole
    table (torch.equal):
      gather            F_.gather_rows backward                                   HAS_G
      gather-bcast      the same with an expanded (B,1,E) gradient                broadcast read (HAS_FM without fm_sum)
      fm-full           F_.embed_fm backward, (B,N,E) and full (B,E) FM gradient  HAS_G + HAS_FM
      fm-lean           the same with an expanded (B,1) FM gradient               scatter_rows_fm1_kernel<HAS_G>
      fm-only-full      FM gradient alone, (B,E)                                  HAS_G = false
      fm-only-lean      FM gradient alone, expanded (B,1)                         scatter_rows_fm1_kernel<false>
      fm-scal-N1        embed_fm on the first field alone (N = 1), expanded FM    non-lean SCAL kernel (N < 2)
      fm-scal-strided   F_.scatter_rows with a strided embedding gradient         non-lean SCAL kernel (gbs != N)
      fields            F_.embed_fm_fields, all three gradients                   trs_scatter_rows_first (HAS_F1), both tables
      fields-lean       the same with an expanded (B,1) FM gradient               HAS_F1 with one g vector per sample
      padding           padding_idx on the 257-lookup row (gather and fm-lean)    zero row, never queued
    On the element path the same sources reach scatter_rows_elem_kernel and its queue / split kernels."""
    from torecsys_amd import functional as F_
    fs, idx, rows, counts = _ladder(1)
    B, N = idx.shape
    V = sum(fs)
    c = _case(E)
    _assert_exact(c, dtype)
    F_.clear_caches()
    idx_d, off_d = idx.to(dev), R.field_offsets(fs).to(dev)
    w = _to(c["w"], dev, dtype)
    ge, gs, gf, gf1 = (_to(c[k], dev, dtype) for k in ("ge", "gs", "gf", "gf1"))
    gf1x, gsx = gf1.expand(B, E), gs.expand(B, N, E)
    assert gsx.stride(1) == 0 and (E == 1 or gf1x.stride(1) == 0)
    f = _Fails(counts)

    f.check("gather", _gather(F_, w, idx_d, off_d, ge).grad, c["G_ge"], dtype)
    f.check("gather-bcast", _gather(F_, w, idx_d, off_d, gsx).grad, c["G_gs"], dtype)
    f.check("fm-full", _embed_fm(F_, w, idx_d, off_d, ge, gf).grad, c["G_ge"] + c["G_fm"], dtype)
    f.check("fm-lean", _embed_fm(F_, w, idx_d, off_d, ge, gf1x).grad, c["G_ge"] + c["G_fm1"], dtype)
    f.check("fm-only-full", _embed_fm(F_, w, idx_d, off_d, None, gf).grad, c["G_fm"], dtype)
    f.check("fm-only-lean", _embed_fm(F_, w, idx_d, off_d, None, gf1x).grad, c["G_fm1"], dtype)

    # N = 1: the first field as a table of its own (S = w[r], so the FM term cancels exactly -- if g*S and sum g agree)
    V1 = fs[0]
    idx1 = idx[:, :1].contiguous()
    want1 = (R.scatter_sum(idx1.reshape(-1), V1, c["ge"][:, 0].double())
             + R.grad_fm(idx1.reshape(-1), V1, 1, c["w"][:V1].double(), c["gf1"]))
    f1 = _Fails(torch.bincount(idx1.reshape(-1), minlength=V1))
    f1.check("fm-scal-N1", _embed_fm(F_, w[:V1], idx1.to(dev), off_d[:1], ge[:, :1].contiguous(), gf1x).grad, want1, dtype)
    f.msgs += f1.msgs

    # a strided embedding gradient: N + 1 rows per sample, the last one (sevens) belongs to nobody
    rb = F_.row_buckets(idx_d, off_d, V)
    gpad = torch.full((B, N + 1, E), 7.0, dtype=dtype, device=dev)
    gpad[:, :N] = ge
    S_d = c["S"].to(dev).float()
    got = F_.scatter_rows(rb, w, g_rows=gpad, g_bcast=gf1.contiguous(), fm_sum=S_d, g_rows_batch_stride=N + 1)
    f.check("fm-scal-strided", got, c["G_ge"] + c["G_fm1"], dtype)

    # the companion (E = 1) table in the same walk
    w1, g1 = _to(c["w1"], dev, dtype), _to(c["g1"], dev, dtype)
    for name, gfm, Gfm in (("fields", gf, c["G_fm"]), ("fields-lean", gf1x, c["G_fm1"])):
        wd, w1d = w.clone().requires_grad_(), w1.clone().requires_grad_()
        emb, fm, first = F_.embed_fm_fields(wd, w1d, idx_d, off_d)
        torch.autograd.backward([emb, fm, first], [ge, gfm, g1])
        f.check(name + "/wide", wd.grad, c["G_ge"] + Gfm, dtype)
        f.check(name + "/first", w1d.grad, c["G_first"], dtype)

    prow = R.row_of_length(fs, idx, 0, 257)
    zero = torch.ones(V, 1, dtype=torch.float64)
    zero[prow] = 0
    f.check("padding/gather", _gather(F_, w, idx_d, off_d, ge, padding_idx=prow).grad, c["G_ge"] * zero, dtype)
    f.check("padding/fm-lean", _embed_fm(F_, w, idx_d, off_d, ge, gf1x, padding_idx=prow).grad,
            (c["G_ge"] + c["G_fm1"]) * zero, dtype)
    torch.cuda.synchronize()
    assert not F_.index_errors_seen()
    f.done()


def _misaligned(t):
    """a (V,E) view of a fresh buffer whose data_ptr sits one element behind a 16-byte boundary"""
    V, E = t.shape
    base = torch.zeros(V * E + 8, dtype=t.dtype, device=t.device)
    view = base[1:1 + V * E].view(V, E)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return base, view


@pytest.mark.parametrize("dtype,E", [(F32, 16), (BF16, 32)])
def test_misaligned_table_takes_the_element_path_exactly(dev, dtype, E):
    """E on the vector path, but the table is a view whose data_ptr is not 16-byte aligned: the FM-folded walk (which
    reads the table) and the fused SGD step (which writes it) fall to the element path -- same exact results, and
    nothing outside the view is touched."""
    from torecsys_amd import functional as F_
    from torecsys_amd.optim import FusedSparseSGD
    fs, idx, rows, counts = _ladder(1)
    B, N = idx.shape
    V = sum(fs)
    c = _case(E)
    _assert_exact(c, dtype)
    F_.clear_caches()
    idx_d, off_d = idx.to(dev), R.field_offsets(fs).to(dev)
    ge, gf, gf1 = (_to(c[k], dev, dtype) for k in ("ge", "gf", "gf1"))
    f = _Fails(counts)
    for name, gfm, want in (("fm-full", gf, c["G_ge"] + c["G_fm"]), ("fm-lean", gf1.expand(B, E), c["G_ge"] + c["G_fm1"])):
        base, view = _misaligned(_to(c["w"], dev, dtype))
        base.requires_grad_()
        wv = base[1:1 + V * E].view(V, E)
        assert wv.data_ptr() == view.data_ptr()
        emb, fm, _ = F_.embed_fm(wv, idx_d, off_d)
        torch.autograd.backward([emb, fm], [ge, gfm])
        f.check("misaligned/" + name, base.grad[1:1 + V * E].view(V, E), want, dtype)
        assert float(base.grad[0]) == 0.0 and float(base.grad[1 + V * E:].abs().max()) == 0.0
    # the companion table cannot ride in the element walk: embed_fm_fields falls back to the two tables' own walks
    base, view = _misaligned(_to(c["w"], dev, dtype))
    base.requires_grad_()
    wv = base[1:1 + V * E].view(V, E)
    w1d = _to(c["w1"], dev, dtype).requires_grad_()
    emb, fm, first = F_.embed_fm_fields(wv, w1d, idx_d, off_d)
    torch.autograd.backward([emb, fm, first], [ge, gf, _to(c["g1"], dev, dtype)])
    f.check("misaligned/fields/wide", base.grad[1:1 + V * E].view(V, E), c["G_ge"] + c["G_fm"], dtype)
    f.check("misaligned/fields/first", w1d.grad, c["G_first"], dtype)
    # fused SGD writes the misaligned table in place
    base, view = _misaligned(_to(c["w"], dev, dtype))
    wv = view.requires_grad_()
    F_.gather_rows(wv, idx_d, off_d, opt=FusedSparseSGD(SGD_LR)).backward(ge)
    assert wv.grad is None
    f.check("misaligned/sgd", wv, c["w"].double() - SGD_LR * c["G_ge"], dtype)
    assert float(base[0]) == 0.0 and float(base[1 + V * E:].abs().max()) == 0.0
    f.done()


@pytest.mark.parametrize("dtype,E,path", WIDTHS, ids=WIDTH_IDS)
def test_fused_sgd_is_the_exact_step_at_every_bucket_length(dev, dtype, E, path):
    """FusedSparseSGD(0.25): w - G/4 is exact in fp32 for these magnitudes (asserted), so the updated table is
    torch.equal to (w64 - 0.25 * G64) rounded once -- rows nobody looked up included, which must keep their bits.
    Through gather_rows, embed_fm (full and lean FM gradient), a padding row, and F_.scatter_rows_update_mapped, whose
    row_map sends the compact rows to a permutation of the table and holds out-of-table entries (one of them collects 300
    lookups, so it is queued and chunked like any hot row and must still update nothing)."""
    from torecsys_amd import functional as F_
    from torecsys_amd.optim import FusedSparseSGD
    fs, idx, rows, counts = _ladder(1)
    B, N = idx.shape
    V = sum(fs)
    c = _case(E)
    _assert_exact(c, dtype)
    F_.clear_caches()
    idx_d, off_d = idx.to(dev), R.field_offsets(fs).to(dev)
    w64 = c["w"].double()
    w = _to(c["w"], dev, dtype)
    ge, gf, gf1 = (_to(c[k], dev, dtype) for k in ("ge", "gf", "gf1"))
    f = _Fails(counts)

    def want(G):
        step = w64 - SGD_LR * G
        assert torch.equal(step.float().double(), step)          # exact in fp32: the store is the only rounding
        return step

    def opt():
        return FusedSparseSGD(SGD_LR)
    wd = _gather(F_, w, idx_d, off_d, ge, opt=opt())
    assert wd.grad is None
    f.check("sgd/gather", wd, want(c["G_ge"]), dtype)
    f.check("sgd/fm-full", _embed_fm(F_, w, idx_d, off_d, ge, gf, opt=opt()), want(c["G_ge"] + c["G_fm"]), dtype)
    f.check("sgd/fm-lean", _embed_fm(F_, w, idx_d, off_d, ge, gf1.expand(B, E), opt=opt()),
            want(c["G_ge"] + c["G_fm1"]), dtype)
    prow = R.row_of_length(fs, idx, 0, 257)
    keep = torch.ones(V, 1, dtype=torch.float64)
    keep[prow] = 0
    f.check("sgd/padding", _gather(F_, w, idx_d, off_d, ge, padding_idx=prow, opt=opt()), want(c["G_ge"] * keep), dtype)

    # mapped: compact row u updates table row row_map[u]
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
    inv = inv[mix]
    rb = F_.row_buckets(inv.int().view(-1, 1).to(dev), None, V + 2)
    table = w.clone()
    F_.scatter_rows_update_mapped(rb, table, opt(), _to(g_rows, dev, dtype), row_map.to(dev))
    f.check("sgd/mapped", table, want(c["G_ge"]), dtype)
    torch.cuda.synchronize()
    assert not F_.index_errors_seen()
    f.done()


ADAPTIVE_LR = 2.0 ** -6                     # exact in fp32, like the betas and 1 - beta below
ADAM_BETAS = (0.875, 0.984375)


@pytest.mark.parametrize("capturable", [False, True], ids=["byvalue", "capturable"])
@pytest.mark.parametrize("kind", ["adagrad", "adam"])
@pytest.mark.parametrize("dtype,E", [(F32, 16), (F32, 10), (BF16, 32), (BF16, 10)],
                         ids=["f32-E16-vec", "f32-E10-elem", "bf16-E32-vec", "bf16-E10-elem"])
def test_adagrad_and_adam_steps_at_every_bucket_length(dev, dtype, E, kind, capturable):
    """FusedSparseAdagrad / FusedSparseAdam, three steps through F_.gather_rows.  Step 1 runs on ladder seed 1, steps 2 and
    3 on seed 2 (same table, other rows), so hundreds of rows that hold non-zero state from step 1 are not looked up
    later.

    Untouched rows: weight and state (fp32 for both table dtypes) torch.equal to their values before the step.

    Touched rows: the gradient G the sink receives is exact (integer sums, see the module docstring), so each step is
    checked per element against ONE float64 step from the state the device held before it (read back exactly), fed the
    exact G.  The bound counts the fp32 roundings of sink_vec / sink_elem, u = 2**-24 each, relative to the largest
    operand of the element:
      Adagrad  s' = fma(G, G, s)                                  <= 2u * max(s, G^2, s')
      Adam     m' = m + (G - m)(1 - b1): subtract, add (1 - b1 = 2**-3 exactly)      <= 2u * max(|m|, |G|, |m'|)
               v' = v + (G^2 - v)(1 - b2): square, subtract, add; the first two are scaled by 1 - b2 = 2**-6
                                                                                      <= 2u * max(v, G^2, v')
      step     d = lr * x / (sqrt(y) + eps), w' = w - d: product, root, sum, quotient, difference
                                                                  <= 5u * max(|w|, |d|, |w'|)
      bf16     + half a bf16 unit in the last place of the reference weight, for the final store.
    Nothing is added for the error the step inherits from its freshly rounded moment.
    lr, the betas and 1 - beta are exact in fp32 and the reference uses eps and Adam's bias-corrected step size as
    rounded to fp32, so no other rounding separates the two.  Largest observed multiples of these bounds:
    profiles/scatter_boundaries.md."""
    from torecsys_amd import functional as F_
    from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseAdam
    fs = _ladder(1)[0]
    V = sum(fs)
    off_d = R.field_offsets(fs).to(dev)
    eps = R.as_f32(1e-10 if kind == "adagrad" else 1e-8)
    if kind == "adagrad":
        opt = FusedSparseAdagrad(ADAPTIVE_LR, eps=eps, capturable=capturable)
    else:
        opt = FusedSparseAdam(ADAPTIVE_LR, betas=ADAM_BETAS, eps=eps, capturable=capturable)
    assert R.as_f32(ADAPTIVE_LR) == ADAPTIVE_LR and all(R.as_f32(b) == b and R.as_f32(1 - b) == 1 - b for b in ADAM_BETAS)
    F_.clear_caches()
    w0 = R.integer_case(fs, _ladder(1)[1], E, 5)["w"]
    wd = _to(w0, dev, dtype).requires_grad_()
    names = ("sum",) if kind == "adagrad" else ("exp_avg", "exp_avg_sq")
    worst = {"w": 0.0, "state": 0.0}
    stale = 0
    for step, seed in enumerate((1, 2, 2), start=1):
        _, idx, rows, counts = _ladder(seed)
        B, N = idx.shape
        ge8 = R.integer_case(fs, idx, E, 40 + step)["ge"]
        G = R.grad_plain(rows, V, ge8, B, N)
        R.assert_exact_regime(R.scatter_sum(rows, V, R.plain_terms(ge8, B, N).abs()), [ge8], dtype)
        touched = R.touched_rows(rows, V)
        state = opt.state_for(wd, wd)
        state = (state,) if kind == "adagrad" else state
        pre_w = wd.detach().cpu().clone()
        pre_s = [s.cpu().clone() for s in state]
        if step > 1:
            stale += int((~touched & (pre_s[-1] != 0).any(1)).sum())
        F_.gather_rows(wd, idx.to(dev), off_d, opt=opt).backward(_to(ge8, dev, dtype))
        assert wd.grad is None
        post_w = wd.detach().cpu()
        post_s = [s.cpu() for s in opt.state_for(wd, wd)] if kind == "adam" else [opt.state_for(wd, wd).cpu()]
        assert all(s.dtype == torch.float32 for s in post_s) and post_w.dtype == dtype
        # rows nobody looked up this step: bit for bit
        assert torch.equal(post_w[~touched], pre_w[~touched]), f"step {step}: an untouched row's weight changed"
        for nm, a, b in zip(names, post_s, pre_s):
            assert torch.equal(a[~touched], b[~touched]), f"step {step}: an untouched row's {nm} changed"
        if kind == "adagrad":
            ref_w, ref_s, tol_w, tol_s = R.adagrad_step(pre_w, pre_s[0], G, touched, ADAPTIVE_LR, eps)
            refs, tols = [ref_s], [tol_s]
        else:
            ss = R.adam_step_size(ADAPTIVE_LR, ADAM_BETAS, step)
            ref_w, ref_m, ref_v, tol_w, tol_m, tol_v = R.lazy_adam_step(pre_w, pre_s[0], pre_s[1], G, touched, ss,
                                                                        ADAM_BETAS, eps)
            refs, tols = [ref_m, ref_v], [tol_m, tol_v]
        if dtype == BF16:
            tol_w = tol_w + torch.where(touched.view(-1, 1), R.bf16_half_ulp(ref_w), torch.zeros_like(tol_w))

        def multiple(name, got, ref, tol):
            ratio = (got.double() - ref).abs() / tol.clamp_min(1e-300)
            ratio = torch.where((got.double() == ref), torch.zeros_like(ratio), ratio)
            m = float(ratio.max())
            if not m <= 1.0:
                r, col = divmod(int(ratio.argmax()), ratio.shape[1])
                raise AssertionError(f"step {step} {name}: {m:.3g} x the derived bound at row {r} ({int(counts[r])} lookups) "
                                     f"col {col}: got {float(got[r, col])!r} reference {float(ref[r, col])!r}")
            return m
        assert torch.isfinite(post_w.float()).all()
        worst["w"] = max(worst["w"], multiple("weight", post_w, ref_w, tol_w))
        for nm, a, b, t in zip(names, post_s, refs, tols):
            worst["state"] = max(worst["state"], multiple(nm, a, b, t))
        assert not torch.equal(post_w[touched], pre_w[touched])
    assert stale > 500, stale          # rows holding state from an earlier step that a later step did not look up
    line = (f"scatter-boundaries {kind} {'capturable' if capturable else 'by-value'} "
            f"{'fp32' if dtype == F32 else 'bf16'} E={E}: weight {worst['w']:.3f} x bound, state {worst['state']:.3f} x bound")
    print(line)

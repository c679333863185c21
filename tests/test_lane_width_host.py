"""Host-side checks of tests/lane_width_ref.py (no GPU): its log2_lanes against the library's own pure path queries, each
fp64 reference against an independent formulation, and the exactness condition the GPU tests (tests/test_gpu_lane_widths.py)
rest on, checked for every op on every entry of WIDTHS with the very operands those tests use.

The condition: every term of every sum a reference is built from is a multiple of the quantum q = 1/4 (1/8 where a mean
over up to 8 positions scales the terms), and every prefix sum, taken forwards and backwards, is such a multiple with a
magnitude below 2^24 q (2^22 for q = 1/4): the 24 significant bits of fp32 then hold every partial sum.  On top of that
each sum is recomputed in fp32 in three orders -- forwards, backwards, pairwise -- and must give the bits of the fp64 sum."""
import pytest
import torch
import torch.nn.functional as F

import bag_shard_ref as S
import lane_width_ref as R
from bag_masked_ref import masked_bag
from lane_width_ref import BF16, F32, WIDTHS, width_id


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


# ------------------------------------------------------------------------------------------------ 1. the path function
def test_widths_list():
    assert len(WIDTHS) == 19 and len(set(WIDTHS)) == 19
    for dtype, E, k in WIDTHS:
        assert R.log2_lanes(E, dtype) == k, (dtype, E)
    for dtype in (F32, BF16):
        assert sorted(k for dt, _, k in WIDTHS if dt == dtype and k >= 0) == list(range(7))
    assert R.B_SECOND_TRIP << 6 > 4096 * 256


def test_log2_lanes_agrees_with_the_library(lib):
    from torecsys_amd import _abi
    from torecsys_amd import functional as F_
    cases = [(dt, E) for dt, E, _ in WIDTHS] + [(dt, E) for dt in (F32, BF16) for E in range(1, 1101)]
    lane = 0
    for dtype, E in cases:
        k = R.log2_lanes(E, dtype)
        code = _abi.TRS_F32 if dtype == F32 else _abi.TRS_BF16
        assert F_.pair_score_path(E, dtype) == (1 if k >= 0 else 0), (dtype, E)
        ws = _abi.size_query("trs_pair_score_bwd_workspace_bytes", 100, 3, E, code)
        assert (ws == 0) == (k >= 0), (dtype, E, ws)
        lane += k >= 0
    assert lane == 14 + 14          # seven widths per dtype, once in WIDTHS and once in 1 .. 1100


# ------------------------------------------------------------------------------------------------ 2. the references
PIN_WIDTHS = [16, 24]


def _real(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("E", PIN_WIDTHS)
def test_bag_ref_against_embedding_bag(E):
    g = torch.Generator().manual_seed(E)
    B, L, V = 13, 8, 20
    w, gout, idx = _real(g, V, E), _real(g, B, E), torch.randint(0, V, (B, L), generator=g)
    for mode in ("sum", "mean", "max"):
        wr = w.clone().requires_grad_()
        y = F.embedding_bag(idx, wr, mode=mode)
        y.backward(gout)
        out, grad = R.bag_ref(w, idx, mode, None, gout)
        assert _close(out, y.detach()) and _close(grad, wr.grad), mode
        _, grad_p = R.bag_ref(w, idx, mode, 3, gout)
        assert float(grad_p[3].abs().max()) == 0.0 and torch.equal(grad_p[4:], grad[4:])
    # the first position wins a tie
    w2 = torch.tensor([[1.0, 0.0], [1.0, 5.0], [1.0, 5.0]], dtype=torch.float64)
    out, grad = R.bag_ref(w2, torch.tensor([[2, 0, 1]]), "max", None, torch.tensor([[3.0, 7.0]], dtype=torch.float64))
    assert out.tolist() == [[1.0, 5.0]] and grad.tolist() == [[0.0, 0.0], [0.0, 0.0], [3.0, 7.0]]


@pytest.mark.parametrize("E", PIN_WIDTHS)
def test_embed_fm_ref_against_the_oracle(E):
    from oracle import cpu_ref as O
    g = torch.Generator().manual_seed(E + 1)
    B, N, V = 11, 5, 40
    w, fw = _real(g, V, E), _real(g, V, 1)
    idx, off = torch.randint(0, 8, (B, N), generator=g), torch.arange(N) * 8
    ge, gf, g1, gn = _real(g, B, N, E), _real(g, B, E), _real(g, B, 1), _real(g, B, N, 1)
    wr, fr = w.clone().requires_grad_(), fw.clone().requires_grad_()
    emb = O.multi_indices_embedding(wr, idx, off)
    fm = O.fm_layer(emb)
    fields = O.multi_indices_embedding(fr, idx, off)
    ((emb * ge).sum() + (fm * gf).sum()).backward()
    r = R.embed_fm_ref(w, fw, idx, off, ge, gf, g1, gn)
    assert torch.equal(r["emb"], emb.detach()) and _close(r["fm"], fm.detach()) and _close(r["grad_w"], wr.grad)
    assert torch.equal(r["fields"], fields.detach()) and _close(r["first"], fields.detach().sum(1))
    (fields.sum(1) * g1).sum().backward()
    assert _close(r["grad_fw_first"], fr.grad)
    fr.grad = None
    (O.multi_indices_embedding(fr, idx, off) * gn).sum().backward()
    assert _close(r["grad_fw_fields"], fr.grad)
    # fm_layer on the block: forward and d fm / d x
    x = emb.detach().clone().requires_grad_()
    (O.fm_layer(x) * gf).sum().backward()
    fm2, s, dx = R.fm_of_block(emb.detach(), gf)
    assert _close(fm2, fm.detach()) and _close(dx, x.grad) and _close(s, emb.detach().sum(1))


@pytest.mark.parametrize("sim", ["dot", "cosine"])
@pytest.mark.parametrize("E", PIN_WIDTHS)
def test_pair_ref_against_autograd(E, sim):
    g = torch.Generator().manual_seed(E + 2)
    B, K, V = 7, 5, 50
    for shared in (True, False):
        Wa, Wt = _real(g, V, E), (None if shared else _real(g, V, E))
        a_idx, t_idx = torch.randint(0, 20, (B,), generator=g), torch.randint(0, 25, (B, 1 + K), generator=g)
        gout = _real(g, B, 1 + K)
        wa = Wa.clone().requires_grad_()
        wt = wa if shared else Wt.clone().requires_grad_()
        a = wa[a_idx + 3].unsqueeze(1)
        a.retain_grad()
        t = wt[t_idx + 25]
        t.retain_grad()
        s = (a * t).sum(2) if sim == "dot" else F.cosine_similarity(a, t, dim=2)
        (s * gout).sum().backward()
        got_s, block, grads = R.pair_ref(Wa, Wt, a_idx, t_idx, 3, 25, sim, gout)
        assert _close(got_s, s.detach()) and _close(block, torch.cat([a.grad, t.grad], 1))
        assert _close(grads[0], wa.grad) and (shared or _close(grads[1], wt.grad))


@pytest.mark.parametrize("E", PIN_WIDTHS)
def test_ffm_ref_against_the_oracle(E):
    from oracle import cpu_ref as O
    g = torch.Generator().manual_seed(E + 3)
    B, N, fs = 9, 4, 11
    ws = [_real(g, N * fs, E) for _ in range(N)]
    idx, off, gout = torch.randint(0, fs, (B, N), generator=g), torch.arange(N) * fs, _real(g, B, N * (N - 1) // 2, E)
    wr = [w.clone().requires_grad_() for w in ws]
    y = O.ffm_layer(O.multi_indices_field_aware_embedding(wr, idx, off), N)
    y.backward(gout)
    out, grads = R.ffm_ref(ws, idx, off, gout)
    assert _close(out, y.detach())
    for got, w in zip(grads, wr):
        assert _close(got, w.grad)


@pytest.mark.parametrize("E", PIN_WIDTHS)
def test_unpermute_ref_against_the_assignment(E):
    c = R.unpermute_case(E, B=13, N=3, V=30)
    K = c["B"] * c["N"]
    s, lo, n = c["inv_pos"].long(), c["self_lo"], c["self_n"]
    want = torch.empty(K, E, dtype=torch.float64)
    for k in range(K):
        slot = int(s[k])
        if lo <= slot < lo + n:
            want[k] = c["shard"][int(c["send_ids"][slot])]
        else:
            want[k] = c["back"][slot - (n if slot >= lo + n else 0)]
    assert torch.equal(R.unpermute_ref(c["back"], c["shard"], c["inv_pos"], c["send_ids"], lo, n), want)


@pytest.mark.parametrize("E", PIN_WIDTHS)
def test_segment_refs_against_bag_shard_ref(E):
    n = 0
    for c in R.segment_cases(E):
        want, bad = S.pool_segments(c["shard"], c["n_valid"], c["ids"], c["seg_start"])
        assert not bad and torch.equal(R.segments_ref(c["shard"], c["n_valid"], c["ids"], c["seg_start"]), want.double())
        want_x, _ = S.pool_segments(c["shard"], c["n_valid"], c["ids_x"], c["seg_start"])
        assert torch.equal(R.segments_ref(c["shard"], c["n_valid"], c["ids_x"], c["seg_start"]), want_x.double())
        rows, ids_bwd = R.expand_ref(c["g_all"], c["ids_x"], c["seg_start"], c["n_valid"], c["pad_local"])
        want_rows, want_ids = S.expand_grad(c["g_all"], c["ids_x"], c["seg_start"], c["n_valid"], c["pad_local"])
        assert torch.equal(rows, want_rows) and torch.equal(ids_bwd, want_ids)
        assert int((ids_bwd == -1).sum()) >= 2 and bool((c["ids_x"] == c["pad_local"]).any())
        assert bool((c["ids_x"] >= c["n_valid"]).any())
        n += 1
    assert n == 8
    parts = torch.randint(-9, 10, (3, 5, E)).float()
    assert torch.equal(R.combine_ref(parts.double(), 0.25).float(), S.combine(parts, 0.25, torch.float32))


# ------------------------------------------------------------------------------------------------ 3. exactness
class Exact:
    """the watcher of lane_width_ref.rsum / rscatter: checks the condition of the module docstring on every sum"""

    def __init__(self):
        self.q = 0.25
        self.sums = 0
        self.largest = 0.0

    def _grid(self, x, what):
        assert bool((x / self.q == (x / self.q).round()).all()), f"{what}: not a multiple of {self.q}"
        m = float(x.abs().max()) if x.numel() else 0.0
        assert m < 2.0 ** 24 * self.q, f"{what}: magnitude {m}"
        self.largest = max(self.largest, m / self.q)

    @staticmethod
    def _seq(t):
        acc = torch.zeros_like(t[0])
        for i in range(t.shape[0]):
            acc = acc + t[i]
        return acc

    @classmethod
    def _pairwise(cls, t):
        n = t.shape[0]
        if n <= 4:
            return cls._seq(t)
        return cls._pairwise(t[: n // 2]) + cls._pairwise(t[n // 2:])

    @classmethod
    def _pairwise_scatter(cls, ids, t, V):
        n = t.shape[0]
        if n <= 64:
            return t.new_zeros(V, *t.shape[1:]).index_add_(0, ids, t)
        return cls._pairwise_scatter(ids[: n // 2], t[: n // 2], V) + cls._pairwise_scatter(ids[n // 2:], t[n // 2:], V)

    def __call__(self, terms, dest):
        self.sums += 1
        terms = terms.reshape(terms.shape[0], -1)
        if terms.shape[0] == 0:
            return
        self._grid(terms, "term")
        t32 = terms.float()
        assert torch.equal(t32.double(), terms)
        if dest is None:
            want = terms.sum(0)
            self._grid(terms.cumsum(0), "prefix sum")
            self._grid(terms.flip(0).cumsum(0), "prefix sum, backwards")
            got = (self._seq(t32), self._seq(t32.flip(0)), self._pairwise(t32))
        else:
            order = torch.argsort(dest, stable=True)
            d, t = dest[order], terms[order]
            for tt in (t, t.flip(0)):                      # prefix sums inside every destination's run, both ways
                dd = d if tt is t else d.flip(0)
                c = tt.cumsum(0)
                start = torch.ones_like(dd, dtype=torch.bool)
                start[1:] = dd[1:] != dd[:-1]
                first = torch.where(start, torch.arange(dd.numel()), torch.zeros_like(dd)).cummax(0)[0]
                self._grid(c - (c - tt)[first], "prefix sum of a scatter")
                self._grid(c, "running total")           # (the subtraction above is then exact as well)
            V = int(dest.max()) + 1
            want = terms.new_zeros(V, terms.shape[1]).index_add_(0, dest, terms)
            got = (t32.new_zeros(V, t32.shape[1]).index_add_(0, dest, t32),
                   t32.new_zeros(V, t32.shape[1]).index_add_(0, dest.flip(0), t32.flip(0)),
                   self._pairwise_scatter(dest, t32, V))
        self._grid(want, "sum")
        for x in got:
            assert torch.equal(x.double(), want), "an fp32 sum in another order differs"


def _masked_through_the_reductions(c, idx, mode, exclude, weighted):
    """masked_bag restated on rsum / rscatter (ids inside the table), and equal to it"""
    w, gout, pad = c["w"], c["gout"], c["pad"]
    psw = c["psw"] if weighted else None
    B, L = idx.shape
    rows = w[idx]
    live = (idx != pad) if exclude else torch.ones_like(idx, dtype=torch.bool)
    coef = live.double() * (psw if weighted else 1.0)
    cnt = live.sum(1)
    scale = torch.where(cnt > 0, 1.0 / cnt.clamp_min(1).double(), torch.zeros(B, dtype=torch.float64))
    want_y, want_g, want_dw = masked_bag(w, idx, mode, pad=pad, exclude=exclude, psw=psw, gout=gout)
    if mode == "max":
        masked = rows.masked_fill(~live.unsqueeze(-1), float("-inf"))
        first = (masked == masked.max(dim=1, keepdim=True)[0]).int().argmax(dim=1)
        d = (torch.arange(L).view(1, L, 1) == first.unsqueeze(1)).double() * (cnt > 0).view(B, 1, 1)
    else:
        out = R.rsum(rows * coef.unsqueeze(-1), 1)
        d = coef.unsqueeze(-1).expand(B, L, w.shape[1])
        if mode == "mean":
            out, d = out * scale.unsqueeze(1), d * scale.view(B, 1, 1)
        assert torch.equal(out, want_y)
    grad = R.rscatter(idx.reshape(-1), (d * gout.unsqueeze(1)).reshape(B * L, -1), w.shape[0])
    grad[pad] = 0
    assert torch.equal(grad, want_g)
    if weighted:
        assert torch.equal(R.rsum(rows * gout.unsqueeze(1), 2) * live, want_dw)


@pytest.mark.parametrize("width", WIDTHS, ids=width_id)
def test_every_sum_is_exact_in_fp32(width):
    dtype, E, k = width
    ex = Exact()
    with R.watching(ex):
        for c in R.bag_cases(E):
            ex.q = 0.125 if c["mode"] == "mean" else 0.25
            R.bag_ref(c["w"], c["idx"], c["mode"], c["pad"], c["gout"])
        ex.q = 0.25
        c = R.probe_bag_case(dtype, E)
        for mode in ("sum", "max"):
            R.bag_ref(c["w"], c["idx"], mode, None, c["gout"])
        if width in R.masked_widths():
            for L in R.MASKED_LENGTHS:
                c = R.masked_case(E, L)
                for mode, exclude, weighted in R.MASKED_COMBOS:
                    ex.q = 0.125 if mode == "mean" else 0.25
                    _masked_through_the_reductions(c, c["idx_mean"] if mode == "mean" else c["idx"], mode, exclude, weighted)
        ex.q = 0.25
        if width in R.HOT_WIDTHS:
            c = R.hot_case(E, k)
            for mode, exclude, weighted in (("sum", True, True), ("sum", False, True), ("max", True, False)):
                _masked_through_the_reductions(c, c["idx"], mode, exclude, weighted)
        for c in R.fm_cases(E, k):
            R.embed_fm_ref(c["w"], c["fw"], c["idx"], c["offsets"], c["g_emb"], c["g_fm"], c["g_first"], c["g_fields"])
            R.embed_fm_ref(c["w"], c["fw"], c["idx"], c["offsets"], None, c["g_fm"])
        for c in list(R.pair_cases(E)) + [R.probe_pair_case(dtype, E)]:
            R.pair_ref(c["Wa"], c["Wt"], c["a_idx"], c["t_idx"], c["a_off"], c["t_off"], "dot", c["gout"])
        for c in R.ffm_cases(E):
            R.ffm_ref(c["ws"], c["idx"], c["offsets"], c["gout"])
        c = R.unpermute_case(E)
        block = R.unpermute_ref(c["back"], c["shard"], c["inv_pos"], c["send_ids"], c["self_lo"], c["self_n"])
        R.fm_of_block(block.reshape(c["B"], c["N"], E))
        for c in R.segment_cases(E):
            parts = R.segments_ref(c["shard"], c["n_valid"], c["ids"], c["seg_start"])
            R.combine_ref(torch.stack([parts, parts, parts]), 0.25)
        if k == 6:
            c = R.second_trip_case(E)
            R.bag_ref(c["w"], c["idx"], "sum", None, c["gout"])
            _masked_through_the_reductions(dict(c, pad=0), c["idx"], "sum", False, True)
            R.embed_fm_ref(c["w"], c["fw"], c["idx"], None, None, c["gout"], c["g2"][:, :1])
            R.pair_ref(c["w"], None, c["idx"][:, 0], c["idx"], 0, 0, "dot", c["g2"])
            n = c["idx"].shape[0]
            R.segments_ref(c["w"], c["w"].shape[0], c["idx"][:, 0], torch.arange(n + 1))
    assert ex.sums > 100
    print(f"{width_id(width)}: {ex.sums} sums, largest partial sum {ex.largest:.0f} quanta (limit {2 ** 24})")

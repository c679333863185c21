"""Host checks of tests/exact_afm_ref.py: the float64 reference against the oracle and the reference project's fixtures, the
exact-domain guard and the coverage conditions over EVERY case tests/test_gpu_exact_afm.py runs, the restated dispatch
arithmetic against the text of csrc/afm.hip and trs_common.hpp, that every case list sits on the path and threshold it
claims, and what the existing tolerance test never reaches."""
import ctypes

import numpy as np
import pytest
import torch

import exact_afm_ref as R
from conftest import AFM_DROP_SHAPES, PAIR_SHAPES, rel_err
from oracle import cpu_ref as O

BF16, F32, F64 = R.BF16, R.F32, R.F64


# ---------------------------------------------------------------------------------------------------------------------
# the reference computes what the oracle and the reference project compute
# ---------------------------------------------------------------------------------------------------------------------
def _oracle(x, W1, b1, w2, b2, g_out, g_attn, keep, scale):
    xr = x.clone().requires_grad_()
    ps = [t.clone().requires_grad_() for t in (W1, b1, w2.view(1, -1), b2)]
    y, attn = O.afm_layer(xr, *ps, score_keep=keep, keep_scale=scale)
    loss = 0
    if g_out is not None:
        loss = loss + (y * g_out).sum()
    if g_attn is not None:
        loss = loss + (attn.squeeze(-1) * g_attn).sum()
    loss.backward()
    return y.detach(), attn.detach().squeeze(-1), xr.grad, [p.grad for p in ps]


@pytest.mark.parametrize("B,N,E,A,drop,mode", [(7, 2, 5, 3, 0, "both"), (5, 17, 32, 32, 0, "both"), (3, 39, 64, 16, 50, "both"),
                                               (4, 9, 24, 33, 0, "out"), (4, 9, 24, 33, 75, "attn")])
def test_reference_is_the_oracle(B, N, E, A, drop, mode):
    """Random real operands: the same float64 formula, here in chunks of samples (chunk_elems small enough to split even
    these batches, gradient-free samples in a pass of their own).  Sums of at most P = 741 terms of magnitude about 1, each
    off by 2**-53 relative: 1e-12 of the largest value is far above that and far below any real difference."""
    g = R.gen(51, B, N, E, A, drop)
    P = N * (N - 1) // 2
    x, W1, b1 = torch.randn(B, N, E, generator=g, dtype=F64), torch.randn(A, E, generator=g, dtype=F64) / E ** 0.5, torch.randn(A, generator=g, dtype=F64)
    w2, b2 = torch.randn(A, generator=g, dtype=F64), torch.randn(1, generator=g, dtype=F64)
    g_out = None if mode == "attn" else torch.randn(B, E, generator=g, dtype=F64)
    g_attn = None if mode == "out" else torch.randn(B, P, generator=g, dtype=F64)
    for gr in (g_out, g_attn):
        if gr is not None:
            gr[1] = 0                                                      # one sample without gradients
    keep = (torch.rand(B, P, generator=g) >= drop / 100.0).to(F64) if drop else None
    scale = 1.0 / (1.0 - drop / 100.0)
    y, attn, gx, gp = _oracle(x, W1, b1, w2, b2, g_out, g_attn, keep, scale)
    r = R.afm_ref(x, W1, b1, w2, b2, g_out, g_attn, keep, scale, chunk_elems=2 * P * max(E, A))
    assert rel_err(r.out, y) <= 1e-12 and rel_err(r.attn, attn) <= 1e-12 and rel_err(r.gx, gx) <= 1e-12
    for got, want in zip((r.gW1, r.gb1, r.gw2), gp):
        assert rel_err(got, want.view(got.shape)) <= 1e-12
    assert float(r.gb2.abs().max()) <= 1e-12 * B * P                      # analytically zero
    assert float(r.gx[1].abs().max()) == 0.0


def test_reference_on_exact_operands_is_the_oracle_bit_for_bit():
    """dyadic operands: every float64 sum is exact in any order, so the chunked reference and the oracle agree exactly"""
    c = R.afm_case(BF16, 12, 24, 33, 5, "low", 75, "both")
    y, attn, gx, gp = _oracle(c.x, c.W1, c.b1, c.w2, c.b2, c.g_out, c.g_attn, c.keep.to(F64), c.keep_scale)
    r = c.ref
    assert torch.equal(r.out, y) and torch.equal(r.attn, attn) and torch.equal(r.gx, gx)
    assert torch.equal(r.gW1, gp[0]) and torch.equal(r.gb1, gp[1]) and torch.equal(r.gw2, gp[2].view(-1)) and torch.equal(r.gb2, gp[3])


@pytest.mark.parametrize("shape", [PAIR_SHAPES[1], PAIR_SHAPES[5]])
def test_reference_reproduces_the_reference_projects_fixture(golden, shape):
    """afm/* of tests/golden/pairs.npz were written by the reference project in float32: the bounds tests/test_oracle_golden.py
    holds the oracle to"""
    G = golden("pairs")
    t = "_".join(str(v) for v in shape)
    d = lambda n: G(f"afm/{t}/{n}").double()                             # noqa: E731
    r = R.afm_ref(d("x"), d("W1"), d("b1"), d("W2").view(-1), d("b2"), d("gout"), d("gattn").squeeze(-1))
    assert rel_err(r.out, d("out")) <= 2e-6 and rel_err(r.attn, d("attn").squeeze(-1)) <= 2e-6
    assert rel_err(r.gx, d("gx")) <= 5e-6
    for got, n in ((r.gW1, "gW1"), (r.gb1, "gb1"), (r.gw2, "gW2")):
        assert rel_err(got, d(n).view(got.shape)) <= 1e-5, n
    assert float((r.gb2 - d("gb2").view(-1)).abs().max()) <= 1e-5


def test_reference_reproduces_the_training_mode_fixture(golden):
    """afm_drop.npz: the reference project in train() with the score mask it drew (its output dropout is applied here
    from the recorded mask, as tests/test_oracle_golden.py does); the bounds of that test"""
    G = golden("afm_drop")
    t = "_".join(str(v) for v in AFM_DROP_SHAPES[1])
    d = lambda n: G(f"{t}/{n}").double()                                 # noqa: E731
    scale = 1.0 / (1.0 - float(G(f"{t}/p")[0]))
    keep = d("score_keep")
    assert 0 < int(keep.sum()) < keep.numel()
    g_out = d("gout") * d("out_keep") * scale                            # the gradient behind the output dropout
    r = R.afm_ref(d("x"), d("W1"), d("b1"), d("W2").view(-1), d("b2"), g_out, d("gattn").squeeze(-1), keep, scale)
    assert rel_err(r.out, d("out_before_dropout")) <= 2e-6 and rel_err(r.attn, d("attn").squeeze(-1)) <= 2e-6
    assert rel_err(r.gx, d("gx")) <= 5e-6
    for got, n in ((r.gW1, "gW1"), (r.gb1, "gb1"), (r.gw2, "gW2")):
        assert rel_err(got, d(n).view(got.shape)) <= 1e-5, n


# ---------------------------------------------------------------------------------------------------------------------
# the guard and the coverage conditions over every case the GPU file runs
# ---------------------------------------------------------------------------------------------------------------------
def _guard(c):
    """no exceptions: a case that fails here is changed, not excused"""
    r, f = c.ref, c.ref.facts
    tensors = {"x": c.x, "W1": c.W1, "b1": c.b1, "w2": c.w2, "b2": c.b2, "attn": r.attn, "attn0": r.attn0, "out": r.out,
               "gx": r.gx, "gW1": r.gW1, "gb1": r.gb1, "gw2": r.gw2}
    for n in ("g_out", "g_attn"):
        if getattr(c, n) is not None:
            tensors[n] = getattr(c, n)
            assert float(getattr(c, n).abs().max()) <= 2
    R.assert_exact_domain(tensors, {})
    assert f.dl_bf16 and f.dh_bf16, "d(logit) / d(hidden) change in a bf16 round trip"
    # live logits bit-equal (``live`` is logit == row maximum), exactly K of them, the pairs the tags name; dead ones far below
    assert torch.equal(r.live, c.live) and bool((r.live.sum(1) == c.K).all())
    assert f.dead_gap >= 1024 or c.live.all()
    assert float(r.gb2.abs().max()) == 0.0
    # scores exactly 1 / K on the live pairs and 0 elsewhere; dropped scores exactly 0, kept ones keep_scale / K
    assert torch.equal(r.attn0, c.live.to(F64) / c.K)
    mult = 1.0 if c.keep is None else c.keep.to(F64) * c.keep_scale
    assert torch.equal(r.attn, r.attn0 * mult)
    if c.keep is not None:
        assert c.keep_scale in (2.0, 4.0) and bool(((c.keep == 0) & c.live).any()) and bool(((c.keep != 0) & c.live).any())
    # every unit but the penalty unit is alive in some live pair and dead in another; the penalty unit is dead in all
    assert bool((f.alive[1:] > 0).all()) and bool((f.dead[1:] > 0).all()) and int(f.alive[0]) == 0
    # samples without gradients receive none; the others do (the all-zero pattern of sample 1 can leave it without any)
    off = sorted(set(range(c.B)) - set(c.grad_samples))
    assert float(r.gx[off].abs().max() if off else 0.0) == 0.0
    assert int((r.gx[c.grad_samples].abs().amax((1, 2)) > 0).sum()) >= (len(c.grad_samples) - 1 if c.K >= 2 else len(c.grad_samples) / 2)
    assert R.covers(c)
    if c.K >= 2:
        assert bool((r.gW1[:, c.S] != 0).any(0).all()), "a column of S without a dW1 entry"
        assert float((r.gW1 != 0).double().mean()) >= 0.15
        assert c.A == 1 or (bool((r.gb1 != 0).any()) and bool((r.gw2 != 0).any()))
        assert f.dl_max > 0


ALL_LISTS = {"inst": R.AFM_INST, "sched": R.AFM_SCHED, "cap_bwd": R.AFM_CAP_BWD, "cap_fwd": R.AFM_CAP_FWD,
             "cap_generic": R.AFM_CAP_GENERIC, "generic": R.AFM_GENERIC, "unaligned": [R.UNALIGNED_CASE], "drop": R.AFM_DROP,
             "modes": R.AFM_MODES}


@pytest.mark.parametrize("name", list(ALL_LISTS))
def test_cases_are_in_the_exact_domain(name):
    cases = ALL_LISTS[name]
    fields = set()
    for case in cases:
        c = R.afm_case(*case)
        assert (c.N, c.E, c.A, c.B) == case[1:5]
        _guard(c)
        fields |= {(c.N, f) for f in c.tag.abs().sum(0).nonzero().flatten().tolist()}
    for case in cases:          # over the list: the first and the last field of every N are live in some sample
        N = case[1]
        assert (N, 0) in fields and (N, N - 1) in fields


def test_every_column_of_w1_is_nonzero_somewhere():
    """S is the low half, the odd columns or the high half: over the cases of every E, all three, and no W1 column (a
    column of the forward's A fragments, a row of the backward's W1^T fragments) that is zero in every case"""
    cols, kinds = {}, {}
    for case in R.AFM_CASES:
        c = R.afm_case(*case)
        if c.A > 1:
            cols.setdefault(c.E, set()).update(c.W1.abs().sum(0).nonzero().flatten().tolist())
            kinds.setdefault(c.E, set()).add(case[5])
    assert set(cols) == {8, 24, 30, 32, 64, 100, 128}
    for E in (32, 64, 128):                                                # the matrix-core shapes: every column
        assert kinds[E] == {"low", "odd", "high"} and cols[E] == set(range(E)), (E, sorted(set(range(E)) - cols[E]))
    for E in (8, 24, 100):
        assert kinds[E] == {"low", "odd", "high"} and len(cols[E]) >= 0.9 * E, (E, sorted(set(range(E)) - cols[E]))


def test_every_field_is_live_somewhere():
    """over all the lists every field index below 65 carries a tag in some sample (the slot cases give every PAIR per N)"""
    fields = set(range(max(N for _, N, _, _ in R.AFM_SLOT)))
    assert all(N * (N - 1) // 2 == R.slot_case(N, E, A).B for _, N, E, A in R.AFM_SLOT[:2])
    for case in R.AFM_SCHED:
        fields |= set(R.afm_case(*case).tag.abs().sum(0).nonzero().flatten().tolist())
    assert fields == set(range(65))


@pytest.mark.parametrize("dtype,N,E,A", R.AFM_SLOT, ids=R.dtype_tag)
def test_slot_cases(dtype, N, E, A):
    """attn is the identity, out[p] the product row of pair p, gx touches fields i_p and j_p alone"""
    c = R.slot_case(N, E, A)
    r = c.ref
    P = N * (N - 1) // 2
    I, J = R.pair_index(N)
    R.assert_exact_domain({"x": c.x, "out": r.out, "attn": r.attn, "gx": r.gx, "g_out": c.g_out, "g_attn": c.g_attn}, {})
    assert c.B == P and c.K == 1 and torch.equal(r.attn, torch.eye(P, dtype=F64)) and torch.equal(r.live, torch.eye(P, dtype=torch.bool))
    assert r.facts.dead_gap >= 1024 or P == 1
    p = torch.arange(P)
    assert torch.equal(r.out, c.x[p, I] * c.x[p, J])
    want = torch.zeros(P, N, E, dtype=F64)
    want[p, I], want[p, J] = c.g_out * c.x[p, J], c.g_out * c.x[p, I]
    assert torch.equal(r.gx, want)
    gs = torch.tensor(c.grad_samples)
    # (a sample whose two g_out columns meet zeros of both rows receives none)
    assert int((r.gx[gs].abs().amax((1, 2)) > 0).sum()) >= 0.7 * len(gs) and (len(gs) == P or P > 1000)
    for t in (r.gW1, r.gb1, r.gw2, r.gb2):                                # one live pair: d(logit) = 0
        assert float(t.abs().max()) == 0.0
    if N > 2:       # a slot moved by one is seen in the forward and in the backward
        assert not torch.equal(r.attn.roll(1, 1), r.attn) and not torch.equal(r.gx.roll(1, 1), r.gx)


# ---------------------------------------------------------------------------------------------------------------------
# the mirrors against the source text, and the case lists against the mirrors
# ---------------------------------------------------------------------------------------------------------------------
def test_mirrors_match_the_source_text():
    """Whoever changes one of these lines in csrc/afm.hip or trs_common.hpp must move the mirror in tests/exact_afm_ref.py and
    with it the case lists."""
    for where, line, n in R.source_sites():
        assert n == 1, (where, line, n)
    assert (R.AFM_MAX, R.AFM_TILE_MAX, R.BWD_MFMA_GRID, R.GENERIC_GRID) == (128, 112, 256, 1024)
    # the column parity of GEMM (3)'s 32-pair step starts from 0 in EVERY sample: the counter lives inside the sample loop
    with open(R.os.path.join(R.CSRC, "afm.hip")) as f:
        body = f.read()
    body = body[body.index(R._HEADS["bwd_mfma_kernel"]):]
    loop, counter, tiles = (body.index(t) for t in ("for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {", "int tiles_done = 0;",
                                                    "for (int tile = wave; tile < NT; tile += WAVES) {"))
    assert loop < counter < tiles and body.count("int tiles_done = 0;") == 1
    # figures the issue and the source comments quote
    assert R.afm_bwd_mfma_lds(65, 32, 32) == 109136 and R.bwd_mfma_ok(65, 32, 32, BF16)          # N = 65 is admitted
    assert R.bwd_schedule(39).NT == 47 and R.sched_rounds(39) * ((R.sched_width(39) + 15) // 16) == 78


def test_packed_tiles_are_the_librarys():
    """the restated greedy pass against trs_afm_pair_tiles, tile by tile, for every N it serves; the schedule of every N
    in the case lists covers each pair once with no field twice in a tile"""
    from torecsys_amd import _abi
    lib = _abi.load()
    for N in range(2, 65):
        buf = np.full(R.AFM_TILE_MAX * 16, 0xffff, dtype=np.uint16)
        nt = ctypes.c_int32(0)
        assert lib.trs_afm_pair_tiles(N, buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(nt)) == 0
        tiles, T = R.packed_tiles(N)
        assert nt.value == T, (N, nt.value, T)
        for t in range(T):
            want = [(i << 8) | j for i, j in tiles[t]] + [0xffff] * (16 - len(tiles[t]))
            assert buf[16 * t:16 * t + 16].tolist() == want, (N, t)
    for N in sorted(set(R.AFM_SCHED_N) | {c[1] for c in R.AFM_CASES} | {c[1] for c in R.AFM_SLOT}):
        if N > 65:
            continue
        seen = []
        for tile in R.schedule_tiles(N):
            prs = [e for e in tile if e is not None]
            assert len(tile) == 16 and len({f for e in prs for f in e}) == 2 * len(prs)
            seen += prs
        assert sorted(seen) == [(i, j) for i in range(N) for j in range(i + 1, N)], N


def test_case_lists_sit_on_the_paths_and_thresholds():
    path = lambda c, aligned=True: R.afm_path(c[1], c[2], c[3], c[0], aligned)      # noqa: E731
    # instantiations: all 24 forward <AT, KS>; the backward on the matrix cores exactly where A % 32 == 0 and AT KS <= 12
    inst = {(c[3], c[2]): path(c) for c in R.AFM_INST}
    assert {(p.fwd_AT, p.KS if p.KS else E // 32) for (A, E), p in inst.items()} == {(at, ks) for at in range(1, 9) for ks in (1, 2, 4)}
    assert all(p.fwd == "mfma" for p in inst.values())
    assert {k for k, p in inst.items() if p.bwd == "mfma"} == \
        {(32, 32), (32, 64), (32, 128), (64, 32), (64, 64), (96, 32), (96, 64), (128, 32)}
    assert {k for k, p in inst.items() if p.bwd == "unsupported"} == {(112, 128), (128, 128)}
    generic = {k for k, p in inst.items() if p.bwd == "generic"}
    assert generic >= {(A, E) for A in (16, 48, 80) for E in (32, 64, 128)} | {(112, 32), (112, 64), (64, 128), (96, 128), (128, 64)}
    assert {(inst[k].AMAX, inst[k].ES) for k in generic} == {(a, e) for a in (32, 64, 128) for e in (1, 2)}
    assert all(c[1] == 9 and c[4] == 5 for c in R.AFM_INST)
    # schedules at A = 32
    kinds = {c[1]: path(c).sched for c in R.AFM_SCHED if c[2] == 32}
    assert all(path(c).fwd == path(c).bwd == "mfma" for c in R.AFM_SCHED)
    assert kinds == {**{N: "rounds" for N in (2, 3, 4, 5, 16, 17, 31, 32)}, **{N: "packed" for N in (33, 39, 48, 60)},
                     61: "tpr2", 64: "tpr2", 65: "tpr3"}
    assert {path(c).sched for c in R.AFM_SCHED if c[2] == 64} == {"rounds", "packed", "tpr2"}
    assert all(R.bwd_schedule(N).NT < 4 for N in (2, 3, 4)) and R.bwd_schedule(5).NT == 5          # idle waves / one tile each
    assert R.bwd_schedule(60).T == 111 <= R.AFM_TILE_MAX and R.packed_tiles(61)[1] == 0 and len(R.packed_tiles(61)[0]) == R.AFM_TILE_MAX
    assert [R.bwd_schedule(N).T for N in (33, 39, 48)] == [33, 47, 71]                             # ceil(P / 16)
    assert (R.bwd_schedule(61).TPR, R.bwd_schedule(64).TPR, R.bwd_schedule(65).TPR) == (2, 2, 3)
    assert R.sched_width(64) == 32 and R.sched_width(65) == 33                                     # TPR = 3 from N = 65 on
    # tiles_done: waves that end a sample on an odd count (the zero-filled second half) and on an even one, in every schedule
    odd = {N: [n % 2 for n in R.wave_tiles(N)] for N in R.AFM_SCHED_N}
    for group in ((2, 3, 4, 5), (16, 17, 31, 32), (33, 39, 48, 60), (61, 64), (65,)):
        assert any(1 in odd[N] for N in group), group
    assert any(0 in odd[N] for N in R.AFM_SCHED_N)
    # a second tile of a round with empty slots (k >= H) and one cut by a dummy player, under TPR >= 2
    fill = lambda N: [sum(e is not None for e in t) for t in R.schedule_tiles(N)[:3]]      # noqa: E731
    assert fill(61) == [15, 15, 15] and R.schedule_tiles(61)[0][0] is None and R.schedule_tiles(61)[1][15] is None
    assert fill(64) == [16, 16, 16] and fill(65) == [15, 16, 1]
    # slot cases: every family, every schedule kind
    fam = [R.afm_path(N, E, A, dt) for dt, N, E, A in R.AFM_SLOT]
    assert {(p.fwd, p.bwd, p.sched) for p in fam} == {("mfma", "mfma", "rounds"), ("mfma", "mfma", "packed"), ("mfma", "mfma", "tpr2"), ("mfma", "generic", None),
                                                      ("generic", "generic", None)}
    # grid caps
    for c in R.AFM_CAP_BWD:
        assert path(c).bwd == "mfma" and 1 in [n % 2 for n in R.wave_tiles(c[1])]
    assert {(c[1], c[4]) for c in R.AFM_CAP_BWD} == {(N, B) for N in (17, 39) for B in (256, 257, 513)}
    assert {path(c).sched for c in R.AFM_CAP_BWD} == {"rounds", "packed"}
    assert [-(-B // min(B, R.BWD_MFMA_GRID)) for B in (256, 257, 513)] == [1, 2, 3]               # samples of workgroup 0
    (c,) = R.AFM_CAP_FWD
    assert path(c).fwd == "mfma" and c[4] == R.FWD_MFMA_GRID_MOST + 1 == 2049
    for c in R.AFM_CAP_GENERIC:
        assert path(c).fwd == path(c).bwd == "generic"
    assert {(c[0], c[4]) for c in R.AFM_CAP_GENERIC} == {(dt, B) for dt in (F32, BF16) for B in (1024, 1025)}
    # generic kernels: both dtypes, never the matrix cores, every AMAX x ES and the edges of the buckets
    for c in R.AFM_GENERIC:
        assert path(c).fwd == path(c).bwd == "generic", c
    for dt in (F32, BF16):
        mine = [c for c in R.AFM_GENERIC if c[0] == dt and c[1] != 128]
        assert {(path(c).AMAX, path(c).ES) for c in mine} == {(a, e) for a in (32, 64, 128) for e in (1, 2)}
        assert {c[2] for c in mine} == {8, 24, 30, 64, 100, 128} and {c[3] for c in mine} == {1, 8, 32, 33, 64, 65, 100, 128}
        assert {c[1] for c in mine} == {2, 5, 7, 39}             # 5: (E, A) = (128, 100), refused from N = 7 on
        assert R.afm_path(7, 128, 100, dt).bwd == "unsupported"
        assert any(c[2] % 4 and c[3] % 4 for c in mine)
    big = R.AFM_GENERIC[-1]
    assert R.LDS_PLAIN < R.generic_fwd_lds(*big[1:4]) <= R.LDS_MOST and R.LDS_PLAIN < R.generic_bwd_lds(*big[1:4]) <= R.LDS_MOST
    assert sum(R.generic_bwd_lds(*c[1:4]) > R.LDS_PLAIN for c in R.AFM_GENERIC) >= 3
    # the unaligned view: inside the matrix-core set of both directions, handed to the generic kernels
    c = R.UNALIGNED_CASE
    assert path(c).fwd == path(c).bwd == "mfma" and path(c, False).fwd == path(c, False).bwd == "generic"
    # dropout and the gradient options: keep_scale 2 and 4 and each absent gradient on both families
    fams = lambda cs: {(path(c).bwd, c[6], c[7]) for c in cs}              # noqa: E731
    assert fams(R.AFM_DROP) == {("mfma", 50, "both"), ("mfma", 75, "both"), ("generic", 50, "both"), ("generic", 75, "both")}
    assert fams(R.AFM_MODES) >= {(f, 0, m) for f in ("mfma", "generic") for m in ("out", "attn")}
    assert len(set(R.AFM_CASES)) == len(R.AFM_CASES)


# ---------------------------------------------------------------------------------------------------------------------
# what the existing tolerance test never reaches
# ---------------------------------------------------------------------------------------------------------------------
def test_seams_out_of_reach_of_the_tolerance_shapes():
    """tests/test_gpu_pairx.py::test_afm_vs_oracle, (B, N, E, A) in both dtypes: no N above 39, so never TPR >= 2; only
    (300, 2, 64, 32) gives a workgroup of the matrix-core backward a second sample, and at N = 2 the schedule is ONE tile:
    three waves are idle and no wave walks more than one tile before the next sample (``tiles_done`` starts from 0 in
    every sample -- test_mirrors_match_the_source_text pins that -- so what a second sample can disturb is the re-zeroed
    gradient block, the staged 32-pair step and the dW1 registers carried on); no batch reaches the forward's or the
    generic kernels' grid caps."""
    for (B, N, E, A) in R.OLD_TOLERANCE_SHAPES:
        for dt in (F32, BF16):
            p = R.afm_path(N, E, A, dt)
            assert p.sched not in ("tpr2", "tpr3") and N <= 39
            # at most one sample per workgroup in the generic kernels; in the matrix-core forward too (256 CUs x the
            # resident workgroups of each) unless (300, 2, 64, 32) ran with ONE resident workgroup per CU
            assert B <= R.GENERIC_GRID and (B <= 256 or (B, N, E, A) == (300, 2, 64, 32))
            if p.bwd == "mfma" and B > R.BWD_MFMA_GRID:
                assert (B, N) == (300, 2) and R.bwd_schedule(N).NT == 1
    packed = [(B, N) for (B, N, E, A) in R.OLD_TOLERANCE_SHAPES if R.afm_path(N, E, A, BF16).sched == "packed"]
    assert sorted(packed) == [(37, 39), (70, 34)]
    # one missing pair of 741 moves the output by 1 / 16 of one product here; in the max norm of the tolerance test the
    # same omission at random scores (1 / 741 each) is 1.3e-3 of the output's scale, under its 1e-2
    c = R.afm_case(BF16, 39, 32, 32, 5, "low", 0, "both")
    lost = c.ref.attn.clone()
    lost[0, int(c.live[0].nonzero()[0])] = 0
    I, J = R.pair_index(39)
    out = ((c.x[:, I] * c.x[:, J]) * lost.unsqueeze(-1)).sum(1)
    assert not torch.equal(R.expect(out, BF16), R.expect(c.ref.out, BF16))

"""Host checks of tests/exact_ipn_ref.py: the float64 reference against the oracle and the reference project's fixture, the
exact-domain guard over EVERY case tests/test_gpu_exact_ipn.py runs, the restated dispatch arithmetic against the text of
csrc/pair.hip, that every case list sits on the threshold it claims, and what the existing tolerance tests never reach."""
import pytest
import torch

import exact_ipn_ref as R
from conftest import LAYER_SHAPES, rel_err
from oracle import cpu_ref as O

BF16, F32, F64 = R.BF16, R.F32, R.F64


# ---------------------------------------------------------------------------------------------------------------------
# the reference computes what the oracle and the reference project compute
# ---------------------------------------------------------------------------------------------------------------------
def _oracle(x, gout):
    xr = x.clone().requires_grad_()
    y = O.inner_product_layer(xr)
    y.backward(gout)
    return y.detach(), xr.grad


@pytest.mark.parametrize("B,N,E", [(7, 2, 5), (5, 17, 32), (3, 39, 64), (2, 64, 128)])
def test_reference_is_the_oracle(B, N, E):
    """On integer operands bit for bit.  On random real data the two are the same float64 sums in another order (a
    batched matrix product here, gather / multiply / reduce and index_add in the oracle): at most 128 terms of magnitude
    about 1 per value, each off by 2**-53 relative -- 1e-13 of the largest value is a hundred times that."""
    assert [tuple(t.tolist()) for t in R.pair_index(N)] == [tuple(t.tolist()) for t in O.pair_indices(N)]
    assert torch.equal(torch.stack(R.pair_index(N)), torch.triu_indices(N, N, 1))
    c = R.ipn_case(N, E, B)
    out, dx = _oracle(c.x, c.gout)
    assert torch.equal(c.out, out) and torch.equal(c.dx, dx)
    g = R.gen(31, B, N, E)
    x = torch.randn(B, N, E, generator=g, dtype=F64)
    gout = torch.randn(B, N * (N - 1) // 2, generator=g, dtype=F64)
    out, dx = _oracle(x, gout)
    got, gdx = R.ipn_ref(x, gout)
    assert got.dtype == F64 and got.shape == out.shape and gdx.shape == dx.shape
    assert rel_err(got, out) <= 1e-13 and rel_err(gdx, dx) <= 1e-13
    Gs = R.sym(gout, N)
    assert torch.equal(Gs, Gs.transpose(1, 2)) and float(Gs.diagonal(dim1=1, dim2=2).abs().max()) == 0.0


@pytest.mark.parametrize("shape", LAYER_SHAPES)
def test_reference_reproduces_the_reference_projects_fixture(golden, shape):
    """ipn/*/out and ipn/*/gx of tests/golden/layers.npz were written by the reference project (float32 storage: 1e-6)"""
    G = golden("layers")
    tag = "_".join(str(v) for v in shape)
    out, dx = R.ipn_ref(G(f"fm/{tag}/x").double(), G(f"ipn/{tag}/gout").double())
    assert rel_err(out, G(f"ipn/{tag}/out")) <= 1e-6
    assert rel_err(dx, G(f"ipn/{tag}/gx")) <= 1e-6


def test_embed_reference_is_lookup_plus_oracle_autograd():
    c = R.embed_case(17, 32, 5, torch.int64)
    w = c.table.clone().requires_grad_()
    emb = O.multi_indices_embedding(w, c.idx, c.offsets)
    ipn = O.inner_product_layer(emb)
    ((emb * c.ge).sum() + (ipn * c.gp).sum()).backward()
    assert torch.equal(emb.detach(), c.ref.emb) and torch.equal(ipn.detach(), c.ref.out) and torch.equal(w.grad, c.ref.gtab)
    # the out-of-range form: that lookup is a zero row, nobody receives its gradient, every other value as before but the
    # pairs and gradient rows of sample 0 that touch the field
    n0 = 17 // 2
    assert float(c.oob.emb[0, n0].abs().max()) == 0.0 and torch.equal(c.oob.emb[1:], c.ref.emb[1:])
    assert torch.equal(c.oob.out[1:], c.ref.out[1:]) and not torch.equal(c.oob.out[0], c.ref.out[0])
    assert float(c.oob.rows[0, n0].abs().max()) == 0.0 and not torch.equal(c.oob.gtab, c.ref.gtab)
    assert int(c.bad[0, n0]) + int(c.offsets[n0]) >= c.V and torch.equal(c.bad[1:], c.idx[1:])


# ---------------------------------------------------------------------------------------------------------------------
# the guard over every case the GPU file runs
# ---------------------------------------------------------------------------------------------------------------------
def _guard(c):
    R.assert_exact_domain({"x": c.x, "gout": c.gout, "out": c.out, "dx": c.dx}, {"out": c.out, "dx": c.dx})
    B, N, E = c.x.shape
    assert float(c.out.abs().max()) <= E and float(c.dx.abs().max()) <= N - 1


def _plain_cases():
    return sorted(set(R.IPN_MFMA_N + R.IPN_MFMA_B + [(N, E, B) for _, N, E, B in R.IPN_TILE + R.IPN_BUDGET + R.IPN_GENERIC]
                      + [R.UNALIGNED_CASE] + [(N, E, 5) for E, Ns in R.IPN_LDS_BUCKETS for N in Ns]))


def test_plain_cases_are_in_the_exact_domain():
    big = 0.0
    for (N, E, B) in _plain_cases():
        c = R.ipn_case(N, E, B)
        _guard(c)
        big = max(big, float(c.out.abs().max()), float(c.dx.abs().max()))
        if B * N * E >= 1000:
            assert float(c.out.abs().max()) > 0 and float(c.dx.abs().max()) > 0
    assert 16 <= big <= 128                                    # the values are not degenerate either


@pytest.mark.parametrize("dtype,N,E", R.IPN_SLOT, ids=R.dtype_tag)
def test_slot_cases(dtype, N, E):
    """forward E * I_P; backward +-v_p on the two live fields of sample p and zero elsewhere"""
    c = R.slot_case(N, E)
    _guard(c)
    P = N * (N - 1) // 2
    assert c.x.shape == (P, N, E) and torch.equal(c.out, E * torch.eye(P, dtype=F64))
    want = torch.zeros(P, N, E, dtype=F64)
    p = torch.arange(P)
    want[p, c.I] = c.s.unsqueeze(1) * c.v
    want[p, c.J] = c.s.unsqueeze(1) * c.v
    assert torch.equal(c.dx, want) and set(c.v.unique().tolist()) == {-1.0, 1.0}
    assert torch.equal((c.x.abs().sum(-1) > 0).sum(1), torch.full((P,), 2))
    if N > 2:       # a slot moved by one is seen: the neighbour's result differs in the forward and in the backward
        assert not torch.equal(c.out.roll(1, 1), c.out) and not torch.equal(R.ipn_ref(c.x, c.gout.roll(1, 1))[1], c.dx)


def test_embed_cases_are_in_the_exact_domain():
    for (N, E, B, it) in R.IPN_EMBED:
        c = R.embed_case(N, E, B, it)
        assert c.idx.dtype == it and int(c.lookups.max()) <= 4
        if N >= 16:                                            # some rows collect several lookups, some none
            assert int(c.lookups.max()) >= 2 and int(c.lookups.min()) == 0
        for r in (c.ref, c.oob):
            R.assert_exact_domain({"table": c.table, "ge": c.ge, "gp": c.gp, "emb": r.emb, "ipn": r.out, "dx": r.dx,
                                   "dx + ge": r.rows, "table gradient": r.gtab}, {"table gradient": r.gtab},
                                  {"table gradient rows": r.terms})
            assert float(r.terms.max()) <= 4 * (N - 1 + 1)
        assert all(0 <= int(c.idx[:, n].max()) < c.sizes[n] for n in range(N))


# ---------------------------------------------------------------------------------------------------------------------
# the mirrors against the source text, and the case lists against the mirrors
# ---------------------------------------------------------------------------------------------------------------------
def test_mirrors_match_the_source_text():
    """Whoever changes one of these lines in csrc/pair.hip must move the mirror in tests/exact_ipn_ref.py and with it the
    case lists."""
    for fn, line, n in R.source_sites():
        assert n == 1, (fn, line, n)
    assert R.LDS_BUDGET == 80 * 1024 and R.WAVES_MAX == 4 * 256 * 8 == 8192 and R.GENERIC_ITEMS_MAX == 256 * 8192
    assert R.grid(R.WAVES_MAX) * 4 == R.WAVES_MAX == R.grid(10 ** 9) * 4 and R.grid(R.WAVES_MAX - 4) * 4 == R.WAVES_MAX - 4
    # the figures of the backward's dynamic LDS the order-dependent attribute was written up with
    lds = {(E, N): R.bwd_mfma_lds(N, E) for E in (64, 128) for N in (33, 39, 48, 49, 64)}
    assert [lds[(64, N)] for N in (33, 39, 48, 49, 64)] == [65568, 66000, 66768, 76080, 77760]
    assert [lds[(128, N)] for N in (33, 39, 48, 49, 64)] == [102432, 102864, 103632, 112944, 114624]
    assert {E: (R.tile_max_n(R.tile_fwd_lds, E), R.tile_max_n(R.tile_bwd_lds, E)) for E in (16, 64, 96, 128)} == \
        {16: (82, 60), 64: (52, 44), 96: (40, 36), 128: (32, 28)}


def test_case_lists_sit_on_the_thresholds():
    # matrix cores: every (NT, KS / KE), N on both sides of every tile edge
    paths = {(N, E): R.ipn_path(BF16, N, E) for N, E, _ in R.IPN_MFMA_N}
    assert all(p.fwd == p.bwd == "mfma" for p in paths.values())
    assert {(p.NT, p.KS, p.KE) for p in paths.values()} == {(nt, ks, 2 * ks) for nt in (1, 2, 3, 4) for ks in (1, 2, 4)}
    for E in (32, 64, 128):
        have = {N for N, e, _ in R.IPN_MFMA_N if e == E}
        assert have >= {2, 64} | {16 * t + d for t in (1, 2, 3) for d in (-1, 0, 1)} | {63}
    assert all(B == 5 and R.grid(B) == 2 for _, _, B in R.IPN_MFMA_N)
    # the grid cap and the samples a wave takes
    for NE in ((17, 32), (33, 64)):
        Bs = [B for N, E, B in R.IPN_MFMA_B if (N, E) == NE]
        assert Bs == [1, 3, 4, 8191, 8192, 8193, 16385] and R.ipn_path(BF16, *NE).fwd == "mfma"
        assert [-(-B // (4 * R.grid(B))) for B in Bs] == [1, 1, 1, 1, 1, 2, 3]          # samples of wave 0
        assert [R.grid(B) for B in Bs] == [1, 1, 1, 2048, 2048, 2048, 2048]
    assert R.ipn_path(BF16, 17, 32).NT == 2 and R.ipn_path(BF16, 33, 64).NT == 3
    # slot cases: every kernel family and every NT
    fam = [R.ipn_path(dt, N, E) for dt, N, E in R.IPN_SLOT]
    assert {(p.fwd, p.NT) for p in fam} == {("mfma", 1), ("mfma", 2), ("mfma", 3), ("mfma", 4), ("tile", None)}
    assert (F32, 41, 8) in R.IPN_SLOT and (BF16, 64, 128) in R.IPN_SLOT
    # tiles: never the matrix cores; the tile kernels in both directions wherever the LDS budget admits N (all of it at
    # E = 4 / 16; at E = 64 / 96 the largest N are already the generic kernels' in one or both directions, held to the
    # same equality); N mod 4 in full below 10; more than 64 register tiles from N = 41 on, in either dtype
    for dt, N, E, B in R.IPN_TILE:
        p = R.ipn_path(dt, N, E)
        assert p.NT is None and B == 6 and R.grid(B) == 2
        assert (p.fwd == "tile") == (N <= R.tile_max_n(R.tile_fwd_lds, E)) and (p.bwd == "tile") == (N <= R.tile_max_n(R.tile_bwd_lds, E))
        assert p.fwd == p.bwd == "tile" or (N >= 40 and E >= 64)
    for dt, E in ((F32, 4), (F32, 16), (F32, 64), (BF16, 16), (BF16, 96)):
        Ns = {N for d, N, e, _ in R.IPN_TILE if (d, e) == (dt, E)}
        assert {N % 4 for N in Ns if N < 10} == {0, 1, 2, 3} and {2, 3, 4, 5} <= Ns
        ntiles = {N: ((N + 3) // 4) * ((N + 3) // 4 + 1) // 2 for N in Ns}
        assert ntiles[40] == 55 <= 64 < 66 == ntiles[41] and ntiles[45] == 78
    for dt in (F32, BF16):
        second = [(N, E) for d, N, E, _ in R.IPN_TILE if d == dt and N >= 41 and R.ipn_path(d, N, E).fwd == "tile"]
        assert {N % 4 for N, _ in second} == {0, 1} and len(second) >= 3
        assert any(N >= 41 and R.ipn_path(d, N, E).bwd == "tile" for d, N, E, _ in R.IPN_TILE if d == dt)
    # budget: both neighbours of each direction's hand-over, on different sides
    for dt, E in ((F32, 64), (F32, 128), (BF16, 96)):
        Ns = [N for d, N, e, _ in R.IPN_BUDGET if (d, e) == (dt, E)]
        fwd = [R.ipn_path(dt, N, E).fwd for N in Ns]
        bwd = [R.ipn_path(dt, N, E).bwd for N in Ns]
        nf, nb = R.tile_max_n(R.tile_fwd_lds, E), R.tile_max_n(R.tile_bwd_lds, E)
        assert {nf, nf + 1, nb, nb + 1} == set(Ns) and nb + 1 < nf
        assert fwd == ["tile", "tile", "tile", "generic"] and bwd == ["tile", "generic", "generic", "generic"]
        assert R.tile_fwd_lds(nf, E) <= R.LDS_BUDGET < R.tile_fwd_lds(nf + 1, E)
        assert R.tile_bwd_lds(nb, E) <= R.LDS_BUDGET < R.tile_bwd_lds(nb + 1, E)
    # generic: both directions, more than one block; the last case walks past the thread count in both directions
    for dt, N, E, B in R.IPN_GENERIC:
        p = R.ipn_path(dt, N, E)
        assert p.fwd == p.bwd == "generic" and B * (N * (N - 1) // 2) > 256 and B * N * E > 256
    dt, N, E, B = R.IPN_GENERIC[-1]
    assert (dt, N, E) == (BF16, 65, 64) and not R.mfma_ok(65, 64) and R.mfma_ok(64, 64)
    assert B * (N * (N - 1) // 2) > R.GENERIC_ITEMS_MAX and B * N * E > R.GENERIC_ITEMS_MAX
    assert {(d, e) for d, _, e, _ in R.IPN_GENERIC[:-1]} == {(d, e) for d in (F32, BF16) for e in (1, 3, 10)}
    # the gather-fused entry: the matrix-core set only, every NT x KS, both index types, one case past the grid cap
    assert all(R.mfma_ok(N, E) for N, E, _, _ in R.IPN_EMBED)
    assert {((N + 15) // 16, E // 32) for N, E, _, _ in R.IPN_EMBED} == {(nt, ks) for nt in (1, 2, 3, 4) for ks in (1, 2, 4)}
    assert {(N, E, it) for N, E, B, it in R.IPN_EMBED if B > R.WAVES_MAX} == {(17, 32, torch.int32), (17, 32, torch.int64)}
    # the unaligned view: inside the matrix-core set, handed to the tiles in both directions
    N, E, _ = R.UNALIGNED_CASE
    p = R.ipn_path(BF16, N, E, aligned=False)
    assert R.mfma_ok(N, E) and p.fwd == p.bwd == "tile"
    # the LDS buckets: one (NT, KE) each, LDS strictly growing with N, above the 64 KiB below which no attribute is set
    for E, Ns in R.IPN_LDS_BUCKETS:
        assert len({(R.ipn_path(BF16, N, E).NT, R.ipn_path(BF16, N, E).KE) for N in Ns}) == 1 and list(Ns) == sorted(Ns)
        lds = [R.bwd_mfma_lds(N, E) for N in Ns]
        assert lds == sorted(set(lds)) and lds[0] > 64 * 1024
    assert len({(R.ipn_path(BF16, Ns[0], E).NT, E) for E, Ns in R.IPN_LDS_BUCKETS}) == 4


# ---------------------------------------------------------------------------------------------------------------------
# what the existing tests never reach
# ---------------------------------------------------------------------------------------------------------------------
def test_a_stale_prefetch_hand_over_is_out_of_reach_of_the_existing_cases():
    """The backward of the matrix-core kernel requests the NEXT sample of a wave while it works on the current one, and
    the hand-over of that prefetch is only exercised when a wave has a next sample: B > WAVES_MAX = 8192.  A hand-over
    that kept the old registers would write sample 0's gradient block again for sample 8192 (same wave).

    The IPN cases the suite had, (B, N, E): test_layers_bf16_vs_oracle (512, 39, 64), (300, 10, 16), (64, 7, 128),
    (33, 5, 10); test_embed_ipn_vs_oracle (1024, 10, 32), (777, 39, 64), (4096, 39, 64), (300, 17, 128), (64, 2, 64);
    the golden LAYER_SHAPES with B <= 32; the fuzz shapes with B <= 13, (4, 17, 32) and (3, 64, 32) among them; and
    test_inner_product_full_size (65536, 39, 64), the only one above 8192 samples, at (N, E) = (39, 64) alone, compared on
    48 sampled rows at 1e-2.  At (17, 32) -- NT = 2, KE = 2, another instantiation with its own register counts -- no existing case has a
    sample 8192, so nothing the suite computes changes; ``torch.equal`` on the case added here does."""
    existing = [(512, 39, 64), (300, 10, 16), (64, 7, 128), (33, 5, 10), (1024, 10, 32), (777, 39, 64), (4096, 39, 64),
                (300, 17, 128), (64, 2, 64), (4, 17, 32), (3, 64, 32)] + list(LAYER_SHAPES)
    N, E, B = 17, 32, R.WAVES_MAX + 1
    assert (N, E, B) in R.IPN_MFMA_B
    c = R.ipn_case(N, E, B)
    broken = c.dx.clone()
    broken[R.WAVES_MAX] = c.dx[0]
    assert not torch.equal(R.expect(broken, BF16), R.expect(c.dx, BF16))
    assert "first at (8192," in R.mismatch("dx", R.expect(broken, BF16), R.expect(c.dx, BF16))
    # every other sample is untouched: a test that stops at or below 8192 samples computes the same thing either way
    assert torch.equal(broken[:R.WAVES_MAX], c.dx[:R.WAVES_MAX])
    assert all(b <= R.WAVES_MAX for (b, n, e) in existing)
    inst = lambda n, e: (R.ipn_path(BF16, n, e).NT, R.ipn_path(BF16, n, e).KE)      # noqa: E731
    assert inst(39, 64) != inst(N, E)                          # nor is the full-size shape the same instantiation

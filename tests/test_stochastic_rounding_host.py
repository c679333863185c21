"""Stochastic rounding of the fused sparse optimizers, host side (no GPU): the generator's known answers, the rule of
include/trs_abi.h as the built library computes it on the CPU (trs_sr_bf16_host) against the numpy restatement
(tests/sr_ref.py) bit for bit, the unbiasedness of the restatement itself, the argument validation of the new entries, and
the optimizers' ``stochastic_rounding`` / ``seed`` arguments with their checkpoint round trip."""
import ctypes

import numpy as np
import pytest
import torch

import sr_ref as SR

from torecsys_amd import functional as F_
from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseAdam, FusedSparseRowWiseAdagrad, FusedSparseSGD

# (counter; key) -> output, Philox4x32-10
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def _host_sr(lib, x, first, seed, t):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(x.size, dtype=np.uint16)
    rc = lib.trs_sr_bf16_host(x.ctypes.data_as(ctypes.c_void_p), x.size, first, seed, t,
                              out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(lib, counter, key, want):
    got = SR.philox4x32_10(counter, key)
    assert tuple(int(w[0]) for w in got) == want
    c = (ctypes.c_uint32 * 4)(*counter)
    k = (ctypes.c_uint32 * 2)(*key)
    o = (ctypes.c_uint32 * 4)()
    assert lib.trs_philox4x32_10_host(c, k, o) == 0
    assert tuple(o) == want


# element positions on both sides of a multiple of 8 (one hash call serves 8 elements) and above 2^32 (the high counter
# word), each with an update number and a seed that use their high words too
FIRSTS = [0, 5, 8 * 1000 - 3, (1 << 32) - 5, (1 << 32) + 8 * 77 - 4, (1 << 40) + 1]
SEED_T = [(0, 1), (1, 1), (20261021, 64), ((0xdeadbeef << 32) | 0x1234567, (1 << 33) + 5)]


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("seed,t", SEED_T)
def test_host_entry_equals_the_reference_bit_for_bit(lib, first, seed, t):
    n = 4096
    g = np.random.default_rng(first % 1000 + seed % 1000)
    normal = _f32(g.integers(0x00800000, 0x7f800000, n, dtype=np.uint32) | (g.integers(0, 2, n, dtype=np.uint32) << 31))
    cases = {
        "random finite, both signs": normal,
        "negative": -np.abs(normal),
        "already bf16": _f32(g.integers(0, 0x7f80, n, dtype=np.uint32) << 16 | (g.integers(0, 2, n, dtype=np.uint32) << 31)),
        "carry into the next exponent": np.tile(_f32([0x3fffffff, 0x3fff8000, 0xbffffff0, 0x3f7fff00]), n // 4),
        "largest finite": np.tile(_f32([0x7f7fffff, 0xff7fffff, 0x7f7f0001, 0x7f7f0000]), n // 4),
        "inf and NaN": np.tile(_f32([0x7f800000, 0xff800000, 0x7fc00000, 0xffc12345, 0x7f800001, 0x7fffffff]), n // 6),
        "zeros and denormals": np.tile(_f32([0x00000000, 0x80000000, 0x00000001, 0x8000ffff, 0x007f8000, 0x00012345]),
                                       n // 6),
    }
    i0 = first
    for name, x in cases.items():
        i = i0 + np.arange(x.size, dtype=np.int64)
        got = _host_sr(lib, x, i0, seed, t)
        want = SR.sr_bf16(x, i, seed, t)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        u = x.view(np.uint32)
        down = (u >> 16).astype(np.uint16)
        if name == "already bf16":
            assert np.array_equal(got, down)                               # whatever r is
        elif name == "inf and NaN":
            assert np.array_equal(got, down)                               # pass through (truncated)
        else:
            # one of the two neighbours, away from zero only where there is a remainder; the sign never changes
            up = (down.astype(np.uint32) + (u & 0xffff != 0)).astype(np.uint16)
            assert ((got == down) | (got == up)).all(), name
            assert np.array_equal(got >> 15, down >> 15), name
        if name == "carry into the next exponent":
            assert (got[0::4] == 0x4000).any()                                      # 1.9999999 -> 2.0 (all r but 0)
            assert (got[1::4] == 0x4000).any() and (got[1::4] == 0x3fff).any()      # 1.99609375: 2.0 or 1.9921875, evenly
            assert (got[2::4] == 0xc000).any()
        if name == "largest finite":
            assert (got[0::4] == 0x7f80).any() and (got[1::4] == 0xff80).any()      # rounds up to infinity, as RNE does
            assert (got[3::4] == 0x7f7f).all()
        if name == "zeros and denormals":
            assert (got[0::6] == 0).all() and (got[1::6] == 0x8000).all()
            assert set(got[4::6].tolist()) == {0x007f, 0x0080}                   # between the last denormals and the first normal


def test_reference_is_unbiased():
    """n = 4096 * 64 elements of 1 - 2^-12 = 0x3f7ff000: the low half is 0xf000, so an element moves up to 1.0 = 0x3f80
    with probability 15/16 and down to 0x3f7f with probability 1/16.  The count of elements that end at 0x3f7f is binomial
    (n, 1/16): mean 16384, sigma = sqrt(n * 1/16 * 15/16) = 123.9, and the bound is 6 sigma = 744.  The rule is
    deterministic, so this passes or fails for good (seeds 0, 1, 20261021 give 16442, 16220, 16379)."""
    n = 4096 * 64
    x = np.full(n, 1.0 - 2.0 ** -12, dtype=np.float32)
    assert int(x.view(np.uint32)[0]) == 0x3f7ff000
    i = np.arange(n, dtype=np.int64)
    sigma = (n * (1 / 16) * (15 / 16)) ** 0.5
    assert 743 < 6 * sigma < 744
    for seed, count in ((0, 16442), (1, 16220), (20261021, 16379)):
        out = SR.sr_bf16(x, i, seed, 1)
        assert set(out.tolist()) == {0x3f7f, 0x3f80}
        low = int((out == 0x3f7f).sum())
        assert abs(low - n / 16) <= 744, (seed, low)
        assert low == count, (seed, low)


def test_sr_entries_validate_the_shared_tail_without_gpu(lib):
    """the _sr entries end in the validated optimizer tail of the plain ones: a bad tail is TRS_EINVAL with the entry's
    name in front, before any launch; every optimizer value the plain entries take (row-wise included) passes it; a mapped
    update of no rows is TRS_OK.  No call here carries a fully valid argument set with non-zero sizes."""
    from torecsys_amd import _abi
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    EINVAL, ESHAPE = -1, -3
    good = dict(optimizer=3, beta1=0.9, beta2=0.999, state=p, state2=p, table=p, row_map=p, U=5, E=16)

    def tail(a):
        return (a["optimizer"], 0.1, null, 1e-8, a["beta1"], a["beta2"], a["state"], a["state2"], p, 1 << 20, null,
                7, 1, null)

    def plain(**kw):
        a = {**good, **kw}
        return lib.trs_scatter_rows_update_sr(p, 0, null, 0, null, a["table"], p, p, 40, 10, a["E"], 4, 1, -1, *tail(a))

    def mapped(**kw):
        a = {**good, **kw}
        return lib.trs_scatter_rows_update_mapped_sr(p, a["table"], a["row_map"], p, p, 40, a["U"], 10, a["E"], 1, *tail(a))

    bad_tails = [dict(optimizer=0), dict(optimizer=4), dict(optimizer=2, state=null), dict(optimizer=3, state2=null),
                 dict(beta1=1.0), dict(beta2=-0.1), dict(table=null), dict(optimizer=16), dict(optimizer=1 | 16),
                 dict(optimizer=2 | 16, state=null), dict(optimizer=2 | 32)]
    for name, entry in (("scatter_rows_update_sr", plain), ("scatter_rows_update_mapped_sr", mapped)):
        for kw in bad_tails:
            assert entry(**kw) == EINVAL, (name, kw)
            assert _abi.last_error().startswith(name + ":"), (name, kw, _abi.last_error())
        # row-wise Adagrad passes the tail and is then refused for a width the element walk would take (bf16: 20 bytes)
        assert entry(optimizer=2 | 16, E=10) == ESHAPE, name
        assert _abi.last_error().startswith(name + ":"), (name, _abi.last_error())
    assert mapped(row_map=null) == EINVAL and _abi.last_error().startswith("scatter_rows_update_mapped_sr:")
    for opt_kw in (dict(optimizer=1, state=null, state2=null), dict(optimizer=2, state2=null), dict(),
                   dict(optimizer=2 | 16, state2=null)):
        assert mapped(U=0, **opt_kw) == 0
    assert mapped(U=0, optimizer=4) == EINVAL
    assert lib.trs_sr_advance(null, null) == EINVAL and _abi.last_error().startswith("sr_advance:")
    assert lib.trs_sr_bf16_host(null, 4, 0, 0, 1, null) == EINVAL
    assert lib.trs_sr_bf16_host(null, 0, 0, 0, 1, null) == 0
    assert lib.trs_sr_bf16_host(p, 4, -1, 0, 1, p) == EINVAL


ALL = [FusedSparseSGD, FusedSparseAdagrad, FusedSparseRowWiseAdagrad, FusedSparseAdam]


@pytest.mark.parametrize("cls", ALL)
def test_constructor_argument(cls):
    off = cls(0.1)
    assert off.stochastic_rounding is False and off.seed == 0
    on = cls(0.1, stochastic_rounding=True, seed=20261021)
    assert on.stochastic_rounding is True and on.seed == 20261021
    assert cls(0.1, stochastic_rounding=True, seed=(1 << 64) - 1).seed == (1 << 64) - 1
    for bad in (1, 0, "yes", None):
        with pytest.raises(TypeError):
            cls(0.1, stochastic_rounding=bad)
    for bad in (1.5, "7", None, True):
        with pytest.raises(TypeError):
            cls(0.1, stochastic_rounding=True, seed=bad)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            cls(0.1, stochastic_rounding=True, seed=bad)
    with pytest.raises(RuntimeError):
        off.next_update(torch.zeros(4, 8, dtype=torch.bfloat16))
    # the plain optimizer's checkpoint is what it was: no new keys
    assert sorted(off.state_dict()) == ["hyper", "tables"] and "seed" not in off.state_dict()["hyper"]


def test_update_counter_and_routing():
    """every update call on a table takes the next number, per table; a bf16 table is routed to the _sr entries with
    (seed, t, NULL), an fp32 table to the plain ones and its counter does not move"""
    opt = FusedSparseSGD(0.1, stochastic_rounding=True, seed=9)
    a = torch.nn.Parameter(torch.zeros(6, 8, dtype=torch.bfloat16))
    b = torch.nn.Parameter(torch.zeros(6, 8, dtype=torch.bfloat16))
    f = torch.nn.Parameter(torch.zeros(6, 8))
    assert opt.next_update(a.data, a) == (1, None) and opt.next_update(a.data, a) == (2, None)
    assert opt.next_update(b.data, b) == (1, None)
    seed, t, t_dev = F_._sr_args(opt, a.data, a)
    assert (seed, t) == (9, 3) and not t_dev
    assert F_._sr_args(opt, f.data, f) == ()
    assert F_._sr_args(FusedSparseSGD(0.1), a.data, a) == ()
    assert len(F_._sink_args(opt, a.data, a)) == 8                     # the plain tail is what it was
    sd = opt.state_dict([("a", a), ("b", b)])
    assert sd["tables"]["a"]["sr_t"] == 3 and sd["tables"]["b"]["sr_t"] == 1


@pytest.mark.parametrize("capturable", [False, True])
def test_state_dict_round_trip_of_seed_and_counters(capturable):
    p = torch.nn.Parameter(torch.zeros(6, 8, dtype=torch.bfloat16))
    q = torch.nn.Parameter(torch.zeros(5, 8, dtype=torch.bfloat16))
    a = FusedSparseRowWiseAdagrad(0.05, capturable=capturable, stochastic_rounding=True, seed=(7 << 40) + 3)
    if capturable:
        for _ in range(4):
            a.next_update(p.data, p)[1].add_(1)             # what trs_sr_advance does on the device
        a.next_update(q.data, q)[1].add_(1)
        assert a.next_update(p.data, p)[0] == 0 and a.next_update(p.data, p)[1].dtype == torch.int64
    else:
        for _ in range(4):
            a.next_update(p.data, p)
        a.next_update(q.data, q)
    a.state_for(p.data, p).copy_(torch.arange(6.0))
    sd = a.state_dict([("p", p), ("q", q)])
    assert sd["stochastic_rounding"] == {"seed": (7 << 40) + 3}
    assert sd["hyper"] == {"lr": 0.05, "eps": 1e-10, "initial": 0.0}
    assert sd["tables"]["p"]["sr_t"] == 4 and sd["tables"]["q"]["sr_t"] == 1
    assert sorted(sd["tables"]["p"]) == ["sr_t", "step", "sum"]

    p2 = torch.nn.Parameter(torch.zeros(6, 8, dtype=torch.bfloat16))
    q2 = torch.nn.Parameter(torch.zeros(5, 8, dtype=torch.bfloat16))
    b = FusedSparseRowWiseAdagrad(0.9, capturable=capturable)              # built without the option: the checkpoint decides
    b.load_state_dict(sd, [("p", p2), ("q", q2)])
    assert b.stochastic_rounding is True and b.seed == (7 << 40) + 3
    assert torch.equal(b.state_for(p2.data, p2), torch.arange(6.0))
    if capturable:
        t, dev = b.next_update(p2.data, p2)
        assert t == 0 and int(dev) == 4                                   # the resumed run continues at update 5
        assert int(b.next_update(q2.data, q2)[1]) == 1
    else:
        assert b.next_update(p2.data, p2) == (5, None)
        assert b.next_update(q2.data, q2) == (2, None)
    assert b.state_dict([("p", p2), ("q", q2)])["tables"]["p"]["sr_t"] == (4 if capturable else 5)

"""Host side of the deep branch's merged weight-gradient launch (csrc/wgrad_rows.hip, trs_wgrad_wide_many): the
workgroup -> (job, row range, block of the job) map that wgrad_dma2_kernel reads, walked through trs_wgrad_wide_many_map
on a box without a GPU, what the query declines, and the ctypes signatures of the new entries against
include/trs_abi.h."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trs_wgrad_wide_many_splits", "trs_wgrad_wide_many_map", "trs_wgrad_wide_many", "trs_wgrad_finish_t"]
# (M_x, ldx, N_g, ldg) per job: the benchmark's three (cur, h1 in 512-wide rows, hidden[0]) and a four-block job behind
# the first layer
DEEP = [(2496, 2496, 400, 512), (416, 512, 400, 416), (416, 416, 400, 416)]
FOUR = [(2496, 2496, 400, 512), (832, 832, 400, 416)]


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def _ia(v):
    return (ctypes.c_int32 * len(v))(*v)


def _query(lib, jobs, rows):
    cols = [_ia([j[k] for j in jobs]) for k in range(4)]
    return int(lib.trs_wgrad_wide_many_splits(len(jobs), *cols, rows)), cols


def test_signatures_agree_with_the_header(lib):
    from torecsys_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trs_abi.h")).read(), flags=re.S)
    ctype_of = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int": ctypes.c_int32, "size_t": ctypes.c_size_t}
    for name in NEW:
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} not declared"
        res, args = _abi.SIGNATURES[name]
        assert res is ctype_of[m.group(1)], name
        want = []
        for a in m.group(2).split(","):
            a = a.strip()
            want.append(ctypes.c_void_p if "*" in a or a.startswith("trs_stream_t") else ctype_of[a.split()[0]])
        assert list(args) == want, (name, args, want)
        assert hasattr(lib, name)


@pytest.mark.parametrize("jobs", [DEEP, FOUR], ids=["2496+416+416", "2496+832"])
@pytest.mark.parametrize("rows", [2048, 2688, 8192, 65536])
def test_map_covers_every_job_range_and_block_once(lib, jobs, rows):
    """16 blocks per range: S = 16, 256 workgroups, every (job, range, block) exactly once, the workgroups of a range on
    one XCD (equal block & 7) with the jobs' blocks in table order, and the ranges tile [0, rows) in whole 128-row quads"""
    out = (ctypes.c_int64 * 5)()
    S, cols = _query(lib, jobs, rows)
    assert S == 16
    grid = int(lib.trs_wgrad_wide_many_map(len(jobs), *cols, rows, 0, out))
    assert grid == 256
    blocks = [j[0] // 208 for j in jobs]
    where, ranges = {}, {}
    for b in range(grid):
        assert int(lib.trs_wgrad_wide_many_map(len(jobs), *cols, rows, b, out)) == grid
        job, slot, mb, lo, hi = (int(v) for v in out)
        assert 0 <= job < len(jobs) and 0 <= slot < S and 0 <= mb < blocks[job]
        assert (job, slot, mb) not in where, f"two workgroups on {(job, slot, mb)}"
        where[(job, slot, mb)] = b
        assert ranges.setdefault(slot, (lo, hi)) == (lo, hi)
    assert len(where) == S * sum(blocks) == 256
    end = 0
    for slot in range(S):
        lo, hi = ranges[slot]
        assert lo == end and hi >= lo + 128 and lo % 128 == 0 and hi % 128 == 0, (slot, lo, hi)
        end = hi
        wgs = [where[(job, slot, mb)] for job in range(len(jobs)) for mb in range(blocks[job])]
        assert len({b & 7 for b in wgs}) == 1, slot
        assert [b >> 3 for b in wgs] == list(range(wgs[0] >> 3, (wgs[0] >> 3) + 16)), slot      # jobs in order
        assert slot // 2 == wgs[0] & 7                                                          # two ranges per XCD
    assert end == rows
    assert int(lib.trs_wgrad_wide_many_map(len(jobs), *cols, rows, grid, out)) == 0
    assert int(lib.trs_wgrad_wide_many_map(len(jobs), *cols, rows, -1, out)) == 0


def test_other_block_counts(lib):
    """TB = 2, 4, 8: four ranges per XCD at most (S = 32); TB = 32: one"""
    for jobs, S, grid in [([DEEP[1]], 32, 64), ([DEEP[1], DEEP[2]], 32, 128), ([FOUR[1]] * 2, 32, 256),
                          ([(208 * 16, 208 * 16, 400, 416)] * 2, 8, 256)]:
        got, cols = _query(lib, jobs, 8192)
        assert got == S, jobs
        out = (ctypes.c_int64 * 5)()
        assert int(lib.trs_wgrad_wide_many_map(len(jobs), *cols, 8192, 0, out)) == grid


def test_query_refusals(lib):
    assert _query(lib, DEEP, 8192)[0] == 16
    assert _query(lib, DEEP[:2], 8192)[0] == 0                                   # TB = 14 does not divide 32
    assert _query(lib, [DEEP[0], (416, 512, 400, 420), DEEP[2]], 8192)[0] == 0   # a row stride that is no multiple of 8
    assert _query(lib, [DEEP[0], (416, 508, 400, 416), DEEP[2]], 8192)[0] == 0
    assert _query(lib, [DEEP[0], (416, 408, 400, 416), DEEP[2]], 8192)[0] == 0   # ldx under M_x
    assert _query(lib, [DEEP[0], (416, 512, 400, 392), DEEP[2]], 8192)[0] == 0   # g's second image would pass ldg
    assert _query(lib, DEEP, 8192 + 37)[0] == 0 and _query(lib, DEEP, 8192 + 64)[0] == 0      # rows % 128 != 0
    assert _query(lib, DEEP, 128 * 16)[0] == 16
    assert _query(lib, DEEP, 128 * 16 - 128)[0] == 0                             # fewer rows than one quad per range
    assert _query(lib, [DEEP[0], (208, 208, 400, 416), (208, 208, 400, 416), DEEP[2]], 8192)[0] == 0      # a single block
    assert _query(lib, DEEP + [DEEP[2]] * 2, 8192)[0] == 0                       # five jobs
    assert _query(lib, [DEEP[0], (416, 512, 512, 512), DEEP[2]], 8192)[0] == 0   # g not two blocks of 12 | 13 tiles
    assert int(lib.trs_wgrad_wide_many_splits(0, None, None, None, None, 8192)) == 0
    assert int(lib.trs_wgrad_wide_many_splits(3, None, None, None, None, 8192)) == 0


def test_entries_refuse_before_any_launch(lib):
    """return codes, no GPU needed: nothing here carries a valid argument set"""
    from torecsys_amd import _abi
    EINVAL, ESHAPE = -1, -3
    S, cols = _query(lib, DEEP, 8192)
    M, ldx, N, ldg = cols
    p3 = (ctypes.c_void_p * 3)(16, 16, 16)
    assert lib.trs_wgrad_wide_many(0, p3, ldx, p3, ldg, 8192, M, N, S, p3, None) == EINVAL
    assert lib.trs_wgrad_wide_many(5, p3, ldx, p3, ldg, 8192, M, N, S, p3, None) == EINVAL
    assert lib.trs_wgrad_wide_many(3, None, ldx, p3, ldg, 8192, M, N, S, p3, None) == EINVAL
    for S_bad in (S - 1, S + 1, 0, 21):
        assert lib.trs_wgrad_wide_many(3, p3, ldx, p3, ldg, 8192, M, N, S_bad, p3, None) == ESHAPE, S_bad
    assert lib.trs_wgrad_wide_many(3, p3, ldx, p3, ldg, 8192 + 64, M, N, S, p3, None) == ESHAPE
    assert lib.trs_wgrad_wide_many(3, (ctypes.c_void_p * 3)(16, 0, 16), ldx, p3, ldg, 8192, M, N, S, p3, None) == EINVAL
    assert lib.trs_wgrad_wide_many(3, (ctypes.c_void_p * 3)(16, 24, 16), ldx, p3, ldg, 8192, M, N, S, p3, None) == ESHAPE
    assert "aligned" in _abi.last_error()
    z3, none3 = _ia([0, 0, 0]), (ctypes.c_void_p * 3)(0, 0, 0)
    assert lib.trs_wgrad_finish_t(0, none3, S, z3, z3, z3, z3, 1, none3, none3, none3, None, None, None) == EINVAL
    assert lib.trs_wgrad_finish_t(9, none3, S, z3, z3, z3, z3, 1, none3, none3, none3, None, None, None) == EINVAL
    assert lib.trs_wgrad_finish_t(3, none3, 0, z3, z3, z3, z3, 1, none3, none3, none3, None, None, None) == EINVAL
    assert lib.trs_wgrad_finish_t(3, none3, S, z3, z3, z3, _ia([4, 4, 4]), 1, none3, p3, none3, None, None, None) == EINVAL
    assert lib.trs_wgrad_finish_t(3, p3, S, z3, z3, z3, z3, 1, p3, none3, none3, None, None, None) == EINVAL      # sizes of 0
    sz = _ia([32, 32, 32])
    assert lib.trs_wgrad_finish_t(3, p3, S, sz, sz, _ia([33, 32, 32]), sz, 1, p3, none3, none3, None, None, None) == EINVAL
    assert lib.trs_wgrad_finish_t(3, p3, S, sz, sz, sz, sz, 1, p3, p3, none3, None, None, None) == EINVAL          # gb_f32 without gb
    assert lib.trs_wgrad_finish_t(3, p3, S, sz, sz, sz, sz, 7, p3, none3, none3, None, None, None) == -2           # dtype

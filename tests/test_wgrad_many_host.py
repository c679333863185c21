"""Host side of the batched weight-gradient launch (csrc/wgrad_rows.hip, trs_wgrad_rows_many): the workgroup ->
(job, row range, output block) map that the kernel reads, walked through trs_wgrad_rows_many_map on a box without a
GPU, and the ctypes signatures of the new entries against include/trs_abi.h."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trs_wgrad_rows_many_splits", "trs_wgrad_rows_many_map", "trs_wgrad_rows_many", "trs_wgrad_finish"]
# (M, N, ldg, ldx) the eight-wave LDS-DMA kernel takes: blocks of 12 | 13 tiles, 2 x 2 and 2 x 4 / 4 x 2 of them
SHAPES = [(400, 400, 416, 512), (400, 400, 416, 416), (416, 416, 416, 416), (384, 416, 384, 416), (400, 800, 416, 800),
          (832, 416, 832, 416)]


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def _ia(v):
    return (ctypes.c_int32 * len(v))(*v)


def _query(lib, jobs, rows):
    cols = [_ia([j[k] for j in jobs]) for k in range(4)]
    return int(lib.trs_wgrad_rows_many_splits(len(jobs), *cols, rows)), cols


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


def test_map_covers_every_job_range_and_block_once(lib):
    """over every job count and shape mix the query admits, at the smallest admitted row count, a ragged one and up to
    2**20 - 128 rows: every (job, range, block) triple has exactly one workgroup, a job's ranges tile [0, rows) in order
    without overlap, and the workgroups that share a (job, range) sit on one XCD (equal block % 8)"""
    out = (ctypes.c_int64 * 5)()
    seen_plans = 0
    for shape in SHAPES:
        for J in range(1, 10):
            jobs = [shape] * J if J % 2 else [shape, SHAPES[2] if shape[:2] == (400, 400) else shape] * (J // 2)
            r0 = next((r for r in range(128, (1 << 17) + 1, 128) if _query(lib, jobs, r)[0] > 0), None)
            if J > 8:
                assert r0 is None
                continue
            if r0 is None:
                continue
            for rows in (r0, r0 + 5 * 128, 65536, (1 << 20) - 128):
                S, cols = _query(lib, jobs, rows)
                if rows < r0:
                    continue
                assert S > 0 and S % 8 == 0, (jobs, rows, S)
                grid = int(lib.trs_wgrad_rows_many_map(J, *cols, rows, 0, out))
                assert 0 < grid <= 256 and grid % (S * J) == 0, (jobs, rows, grid)      # one resident round
                TB = grid // (S * J)
                where, ranges = {}, {}
                for b in range(grid):
                    assert int(lib.trs_wgrad_rows_many_map(J, *cols, rows, b, out)) == grid
                    job, slot, tile, lo, hi = (int(v) for v in out)
                    assert 0 <= job < J and 0 <= slot < S and 0 <= tile < TB
                    assert (job, slot, tile) not in where, f"two workgroups on {(job, slot, tile)}"
                    where[(job, slot, tile)] = b
                    assert ranges.setdefault((job, slot), (lo, hi)) == (lo, hi)
                assert len(where) == J * S * TB
                for job in range(J):
                    end = 0
                    for slot in range(S):
                        lo, hi = ranges[(job, slot)]
                        assert lo == end and hi >= lo + 256 and lo % 128 == 0 and hi % 128 == 0, (job, slot, lo, hi)
                        end = hi
                    assert end == rows
                    for slot in range(S):
                        assert len({where[(job, slot, t)] % 8 for t in range(TB)}) == 1
                assert int(lib.trs_wgrad_rows_many_map(J, *cols, rows, grid, out)) == 0
                seen_plans += 1
    assert seen_plans >= 20


def test_one_job_keeps_the_map_of_the_single_entry(lib):
    """a table of one: block b works on range (b % 8) * (S / 8) + (b / 8) / TB and block (b / 8) % TB, as the kernel did
    before it read its place from the map"""
    out = (ctypes.c_int64 * 5)()
    for rows in (16384, 65536):
        S, cols = _query(lib, [SHAPES[0]], rows)
        assert S == int(lib.trs_wgrad_rows_splits(400, 400, rows)) == 64
        grid = int(lib.trs_wgrad_rows_many_map(1, *cols, rows, 0, out))
        assert grid == 256
        for b in range(grid):
            lib.trs_wgrad_rows_many_map(1, *cols, rows, b, out)
            assert (int(out[0]), int(out[1]), int(out[2])) == (0, (b % 8) * (S // 8) + (b // 8) // 4, (b // 8) % 4)


def test_query_refusals(lib):
    two = [SHAPES[0], SHAPES[1]]
    assert _query(lib, two, 8192)[0] == 32 and _query(lib, two, 8192 - 128)[0] == 0
    assert _query(lib, two, 8192 + 64)[0] == 0
    assert _query(lib, [(400, 400, 392, 512), SHAPES[1]], 8192)[0] == 0
    assert _query(lib, [SHAPES[0], (8, 400, 8, 416)], 8192)[0] == 0
    assert _query(lib, [SHAPES[0], SHAPES[4]], 65536)[0] == 0           # different block counts
    assert _query(lib, [SHAPES[4]] * 5, 65536)[0] == 0                  # 5 x 8 blocks per range: more than one round
    assert _query(lib, two, 1 << 20)[0] == 0                             # the four-wave form's row counts
    assert int(lib.trs_wgrad_rows_many_splits(0, None, None, None, None, 8192)) == 0
    assert int(lib.trs_wgrad_rows_many_splits(2, None, None, None, None, 8192)) == 0

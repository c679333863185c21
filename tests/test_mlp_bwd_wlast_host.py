"""Host side of the output layer's weight gradient inside the fused MLP backward (csrc/mlp_fused.hip,
trs_mlp_fused_bwd_data_wlast) on a box without a GPU: the ctypes signatures of the new entries against
include/trs_abi.h, the query's LDS / reduce-entry arithmetic, and the argument checks that come back as error codes before
anything is launched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trs_mlp_fused_bwd_wlast_part_bytes", "trs_mlp_fused_bwd_data_wlast", "trs_wgrad_finish"]
TILE, ROW_OWNER, MIXED = 1, 2, 3
F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def _ia(v):
    return (ctypes.c_int32 * len(v))(*v)


def _pad32(v):
    return (v + 31) // 32 * 32


def _codes():
    src = open(os.path.join(ROOT, "include", "trs_abi.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(TRS_E\w+|TRS_OK)\s*=\s*(-?\d+)", src)}


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


def _query(lib, widths, rows, family, live, dtype=BF16):
    return int(lib.trs_mlp_fused_bwd_wlast_part_bytes(len(widths) - 1, _ia(widths), rows, dtype, family, live))


def _lds(widths, live):
    """the kernel's request: 128 activation rows, 8 slices of 512 partial sums, (L + 1) rows of column sums and ``live`` rows
    of the output layer's gradient, 512 floats each"""
    L = len(widths) - 1
    act_str = max(_pad32(w) for w in widths) * 2 + 16
    return 128 * act_str + 8 * 512 * 4 + (L + 1 + live) * 512 * 4


def test_query_arithmetic(lib):
    deep = [512, 400, 400, 8]
    assert _lds(deep, 0) == 157696 and _lds(deep, 3) == 163840 == 160 * 1024
    for widths in (deep, [416, 400, 8], [416, 400, 400, 8], [512, 512, 512, 8], [64, 72, 8]):
        for rows in (1, 2, 128, 129, 32901, 65536):
            grid = min((rows + 127) // 128, 256)
            for fam in (TILE, MIXED):
                for live in (1, 2, 3):
                    want = grid * live * _pad32(widths[-2]) * 4 if _lds(widths, live) <= 160 * 1024 else 0
                    assert _query(lib, widths, rows, fam, live) == want, (widths, rows, fam, live)
    assert _query(lib, deep, 65536, TILE, 1) == 256 * 416 * 4
    # declines: live columns, family, dtype, stacks without a hidden layer, entries of the one reduce launch, widths
    assert _query(lib, deep, 65536, TILE, 0) == 0 and _query(lib, deep, 65536, TILE, 4) == 0
    assert _query(lib, deep, 65536, ROW_OWNER, 1) == 0 and _query(lib, deep, 65536, 0, 1) == 0
    assert _query(lib, [64, 400, 400, 400, 64], 2560000, ROW_OWNER, 1) == 0
    assert _query(lib, deep, 65536, TILE, 1, F32) == 0
    assert _query(lib, deep, 0, TILE, 1) == 0
    assert _query(lib, [512, 8], 65536, TILE, 1) == 0
    assert _query(lib, [64] + [72] * 5 + [8], 4096, TILE, 1) > 0 and _query(lib, [64] + [72] * 5 + [8], 4096, TILE, 2) == 0
    assert _query(lib, [64] + [72] * 6 + [8], 4096, TILE, 1) == 0
    assert _query(lib, [544, 400, 8], 4096, TILE, 1) == 0 and _query(lib, [416, 544, 8], 4096, TILE, 1) == 0


def test_bad_arguments_come_back_before_any_launch(lib):
    """NULL and too-small buffers, strides and live counts the entry does not take: error codes, on a box where a launch
    could not even be attempted"""
    code = _codes()
    widths = [512, 400, 400, 8]
    L = 3
    buf = ctypes.create_string_buffer(1 << 16)          # 16-byte aligned host memory standing in for device pointers
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    arr = (ctypes.c_void_p * 4)(base, base, base, base)
    need = _query(lib, widths, 256, TILE, 1)
    ws = int(lib.trs_mlp_fused_workspace_bytes(L, _ia(widths)))

    def run(gy_stride=8, h_last=p, h_stride=416, live=1, part=p, part_bytes=need, gw=p, dtype=BF16, family=TILE):
        return int(lib.trs_mlp_fused_bwd_data_wlast(p, gy_stride, 256, L, _ia(widths), arr, arr, arr, arr, p, None, None,
                                                    h_last, h_stride, live, part, part_bytes, gw, dtype, family, p, ws,
                                                    None))

    assert run(h_last=None) == code["TRS_EINVAL"]
    assert run(part=None) == code["TRS_EINVAL"]
    assert run(gw=None) == code["TRS_EINVAL"]
    assert run(part_bytes=need - 1) == code["TRS_EWORKSPACE"]
    assert run(dtype=F32) == code["TRS_EDTYPE"]
    assert run(live=4) == code["TRS_ESHAPE"] and run(live=0) == code["TRS_ESHAPE"]
    assert run(family=ROW_OWNER) == code["TRS_ESHAPE"]
    assert run(gy_stride=2) == code["TRS_ESHAPE"] and run(gy_stride=16) == code["TRS_ESHAPE"]
    assert run(h_stride=400) == code["TRS_ESHAPE"] and run(h_stride=420) == code["TRS_ESHAPE"]
    assert run(h_last=ctypes.c_void_p(base + 8)) == code["TRS_EALIGN"]
    # a finish job without a product: gb_f32, gb and out_cols only
    fa = (ctypes.c_void_p * 1)(base)
    none = (ctypes.c_void_p * 1)(None)
    zero = _ia([0])
    fin = lambda n=1, S=1, ocols=_ia([400]), gw=none, gbf=fa, gb=fa, dtype=BF16: int(
        lib.trs_wgrad_finish(n, none, S, zero, zero, zero, ocols, dtype, gw, gbf, gb, None, None, None))
    assert fin(gw=fa) == code["TRS_EINVAL"] and fin(gbf=none) == code["TRS_EINVAL"] and fin(gb=none) == code["TRS_EINVAL"]
    assert fin(ocols=zero) == code["TRS_EINVAL"] and fin(S=0) == code["TRS_EINVAL"]
    assert fin(n=0) == code["TRS_EINVAL"] and fin(n=9) == code["TRS_EINVAL"]
    assert fin(dtype=7) == code["TRS_EDTYPE"]

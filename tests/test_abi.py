"""The C-ABI library loads on a CPU-only box and exports every symbol include/trs_abi.h declares; argument
validation (no kernel launch needed) reports errors through return codes and trs_last_error_string()."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "trs_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(trs_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


def test_exports_every_declared_symbol(lib):
    from torecsys_amd import _abi
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in trs_abi.h but not exported"
    assert sorted(_abi.SIGNATURES) == names, "ctypes SIGNATURES out of sync with the header"


def test_abi_version_3_and_sizes(lib):
    assert lib.trs_version() == 3
    assert lib.trs_csr_workspace_bytes(1000, 100) >= 400
    assert lib.trs_scatter_workspace_bytes(100000, 10, 16, 1) >= 8


def test_argument_errors_without_gpu(lib):
    from torecsys_amd import _abi
    null = ctypes.c_void_p(0)
    rc = lib.trs_gather_rows(null, 10, 4, 0, null, 0, null, 2, 2, null, null, null)
    assert rc == -1 and "NULL" in _abi.last_error()
    one = ctypes.c_void_p(16)
    rc = lib.trs_gather_rows(one, 10, 4, 7, one, 0, null, 2, 2, one, null, null)
    assert rc == -2 and "dtype" in _abi.last_error()
    rc = lib.trs_fm_fwd(one, 4, 0, 8, 0, one, null, null)
    assert rc == -1
    with pytest.raises(RuntimeError, match="trs_pair_dot_fwd failed"):
        _abi.call("trs_pair_dot_fwd", null, 1, 2, 4, 0, null, null)


def test_fused_update_tail_is_validated_without_gpu(lib):
    """The optimizer tail both fused-update entries share (optimizer, lr, lr_dev, eps, beta1, beta2, state, state2) is
    rejected with TRS_EINVAL and a message naming the entry before anything is launched; a mapped update of no rows is
    TRS_OK.  No call here carries a fully valid argument set with non-zero sizes."""
    from torecsys_amd import _abi
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    EINVAL = -1
    good = dict(optimizer=3, beta1=0.9, beta2=0.999, state=p, state2=p, table=p, row_map=p, U=5)

    def tail(a):
        return (a["optimizer"], 0.1, null, 1e-8, a["beta1"], a["beta2"], a["state"], a["state2"], p, 1 << 20, null)

    def plain(**kw):
        a = {**good, **kw}
        return lib.trs_scatter_rows_update(p, 0, null, 0, null, a["table"], p, p, 40, 10, 16, 4, 0, -1, *tail(a))

    def mapped(**kw):
        a = {**good, **kw}
        return lib.trs_scatter_rows_update_mapped(p, a["table"], a["row_map"], p, p, 40, a["U"], 10, 16, 0, *tail(a))

    bad_tails = [dict(optimizer=0), dict(optimizer=4), dict(optimizer=2, state=null), dict(optimizer=3, state2=null),
                 dict(beta1=1.0), dict(beta2=-0.1), dict(table=null)]
    for name, entry in (("scatter_rows_update", plain), ("scatter_rows_update_mapped", mapped)):
        for kw in bad_tails:
            assert entry(**kw) == EINVAL, (name, kw)
            assert _abi.last_error().startswith(name + ":"), (name, kw, _abi.last_error())
    assert mapped(row_map=null) == EINVAL and _abi.last_error().startswith("scatter_rows_update_mapped:")
    for opt_kw in (dict(optimizer=1, state=null, state2=null), dict(optimizer=2, state2=null), dict()):
        assert mapped(U=0, **opt_kw) == 0
    # a bad tail is refused even where there is nothing to update
    assert mapped(U=0, optimizer=4) == EINVAL
    retired = ["trs_scatter_rows_update_adam", "trs_scatter_rows_update_dev", "trs_scatter_rows_update_adam_dev",
               "trs_scatter_rows_update_mapped_dev"]
    for n in retired:
        assert not hasattr(lib, n), f"{n} is still exported"
        assert n not in _abi.SIGNATURES


def test_no_oracle_import_in_product():
    pkg = os.path.join(ROOT, "torecsys_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert "oracle" not in src.replace("no CPU", ""), f"{f} mentions the oracle"
    src = open(os.path.join(ROOT, "bench.py")).read() if os.path.exists(os.path.join(ROOT, "bench.py")) else ""
    assert "/root/reference" not in src

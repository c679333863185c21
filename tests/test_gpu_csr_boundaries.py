"""The row-bucket (CSR) build of csrc/scatter.hip at its seams.  Only F_.row_buckets is called -- no table is allocated --
and every check is exact: row_start equals the int64 exclusive prefix of the bincount, perm is a permutation of the valid
lookups grouped by row (scatter_ref._check_csr).

Scan seams: the prefix sum over the V + 1 counters runs in tiles of 4096; up to 2048 tiles one decoupled look-back pass,
above that three launches (tile sums -> one workgroup scanning the sums 256 at a time with a carry -> apply).  No other
test builds a CSR over more than 5 M rows, so the three-launch scan runs here only.
Partition gate: the LDS-counter build needs B >= 2048, N <= 120, at most 16 N + 256 (field, chunk) items and no skip_row;
inside it fields of <= 32 rows use privatised counters and a chunk's piece of perm is staged in LDS up to 24 576 positions.
tests/test_scatter_ref_host.py holds these numbers against the source."""
import pytest
import torch

import scatter_ref as R
from scatter_ref import _check_csr

pytestmark = pytest.mark.gpu

TILE, ONEPASS = 4096, 2048
SEAM_V = [4095, 4096, 64 * TILE - 1, 64 * TILE, 65 * TILE, ONEPASS * TILE - 1, ONEPASS * TILE, ONEPASS * TILE + 1,
          20_000_003]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _even_fields(V, N):
    sizes = [V // N] * N
    sizes[-1] += V - sum(sizes)
    return sizes


def _planted_rows(V):
    """row 0, row V - 1 and both sides of the tile edges a scan can trip over: the first ones, those around every 256th
    tile (the carried rounds of the one-workgroup scan of the tile sums: 256 sums per round), around the one-pass cap and
    the last ones.  Counter i of the scan is row i, so tile t starts at row t * 4096."""
    ntiles = R.scan_tiles(V, TILE)
    tiles = {1, 2, 3, 63, 64, 65, ONEPASS - 1, ONEPASS, ONEPASS + 1, ntiles - 2, ntiles - 1}
    for t in range(256, ntiles, 256):
        tiles |= {t - 1, t, t + 1}
    rows = {0, 1, V - 2, V - 1}
    for t in tiles:
        if 0 < t < ntiles:
            rows |= {t * TILE - 2, t * TILE - 1, t * TILE, t * TILE + 1}
    return sorted(r for r in rows if 0 <= r < V)


def _seam_indices(V, N, B, seed, dtype=torch.int64):
    """(idx (B,N), offsets (N,), rows_flat): every planted row is looked up (some twice), the rest of the batch is uniform
    over each field's own range"""
    g = torch.Generator().manual_seed(seed)
    sizes = _even_fields(V, N)
    off = R.field_offsets(sizes)
    planted = torch.tensor(_planted_rows(V))
    cols = []
    for n in range(N):
        lo, hi = int(off[n]), int(off[n]) + sizes[n]
        mine = planted[(planted >= lo) & (planted < hi)]
        mine = torch.cat([mine, mine[::3]])[:B]                       # every third planted row twice
        fill = torch.randint(lo, hi, (B - mine.numel(),), generator=g)
        col = torch.cat([mine, fill])[torch.randperm(B, generator=g)]
        cols.append(col - lo)
    idx = torch.stack(cols, 1).contiguous()
    rows_flat = (idx + off.view(1, -1)).reshape(-1)
    hit = torch.zeros(V, dtype=torch.bool)
    hit[rows_flat] = True
    assert bool(hit[planted].all())
    return idx.to(dtype), off, rows_flat


def _build_and_check(dev, idx, off, V, rows_flat, **kw):
    from torecsys_amd import functional as F_
    F_.clear_caches()
    rb = F_.row_buckets(idx.to(dev), off.to(dev) if off is not None else None, V, **kw)
    torch.cuda.synchronize()
    _check_csr(rb, rows_flat.to(dev), V)
    del rb
    F_.clear_caches()


@pytest.mark.parametrize("N,B", [(3, 1500), (39, 2048)], ids=["atomic-N3-B1500", "partitioned-N39-B2048"])
@pytest.mark.parametrize("V", SEAM_V)
def test_scan_seams(dev, V, N, B):
    """Both builds in front of both scans: N = 3, B = 1500 takes the global-atomic build; N = 39, B = 2048 the
    partitioned one wherever its item estimate N + ceil(V / chunk) stays within 16 N + 256 -- every V here but the
    largest (39 + 1303 > 880), which test_scan_seams_largest_table covers with N = 72."""
    assert (R.scan_tiles(V, TILE) <= ONEPASS) == (V < ONEPASS * TILE)          # one pass below the cap, three launches from it
    assert R.partitioned(V, N, B) == (N == 39 and V < 20_000_000)
    idx, off, rows_flat = _seam_indices(V, N, B, seed=V % 1000 + N)
    _build_and_check(dev, idx, off, V, rows_flat)


@pytest.mark.parametrize("case", ["partitioned-N72", "int32", "unchecked-out-of-range", "skip-row"])
def test_scan_seams_largest_table(dev, case):
    """V = 20 000 003: 4 883 tiles -- 20 rounds of the carried scan of the tile sums -- and an 80 MB row_start."""
    from torecsys_amd import functional as F_
    V = SEAM_V[-1]
    assert R.scan_tiles(V, TILE) == 4883
    if case == "partitioned-N72":
        assert R.partitioned(V, 72, 2048)
        idx, off, rows_flat = _seam_indices(V, 72, 2048, seed=1)
        _build_and_check(dev, idx, off, V, rows_flat)
    elif case == "int32":
        idx, off, rows_flat = _seam_indices(V, 3, 1500, seed=2, dtype=torch.int32)
        _build_and_check(dev, idx, off, V, rows_flat)
    elif case == "unchecked-out-of-range":
        # check=False: ids that land on -1 and on >= V are left out of the index without raising the flag
        idx, off, rows_flat = _seam_indices(V, 3, 1500, seed=3)
        F_.index_errors_seen()
        sizes = _even_fields(V, 3)
        idx[5, 0], idx[700, 0] = -1, -1
        idx[9, 2], idx[1499, 2] = sizes[2], sizes[2] + 12
        rows_flat = (idx + off.view(1, -1)).reshape(-1)
        assert int((rows_flat < 0).sum()) == 2 and int((rows_flat >= V).sum()) == 2
        _build_and_check(dev, idx, off, V, rows_flat, check=False)
        assert not F_.index_errors_seen()
    else:
        # skip_row: the lookups of one row (a list field's padding id) are left out; here the busiest planted row
        idx, off, rows_flat = _seam_indices(V, 3, 1500, seed=4)
        skip = ONEPASS * TILE
        idx[:400, 1] = skip - int(off[1])
        rows_flat = (idx + off.view(1, -1)).reshape(-1)
        assert int((rows_flat == skip).sum()) >= 400
        expect = torch.where(rows_flat == skip, torch.full_like(rows_flat, -1), rows_flat)
        _build_and_check(dev, idx, off, V, expect, skip_row=skip)


def _uniform(sizes, B, seed, dtype=torch.int64):
    g = torch.Generator().manual_seed(seed)
    off = R.field_offsets(sizes)
    idx = torch.stack([torch.randint(0, s, (B,), generator=g) for s in sizes], 1).contiguous()
    return idx.to(dtype), off, (idx + off.view(1, -1)).reshape(-1)


@pytest.mark.parametrize("B", [2047, 2048, 2049])
def test_partition_gate_batch_size(dev, B):
    sizes = [2564] * 5 + [17, 1, 333, 20000, 40]
    V, N = sum(sizes), len(sizes)
    assert R.partitioned(V, N, B) == (B >= 2048)
    idx, off, rows_flat = _uniform(sizes, B, 5)
    _build_and_check(dev, idx, off, V, rows_flat)


@pytest.mark.parametrize("N", [120, 121])
def test_partition_gate_field_count(dev, N):
    """120 fields is the most the transpose tile holds; 121 takes the global-atomic build"""
    sizes = [30 + (n % 7) for n in range(N)]
    V = sum(sizes)
    assert R.partitioned(V, N, 2048) == (N <= 120)
    idx, off, rows_flat = _uniform(sizes, 2048, 6)
    _build_and_check(dev, idx, off, V, rows_flat)


@pytest.mark.parametrize("extra", [0, 1])
def test_partition_gate_item_count(dev, extra):
    """N + ceil(V / chunk) exactly 16 N + 256 = 304 (partitioned), and one more chunk (global-atomic)"""
    V = 301 * 15360 + extra
    assert R.csr_chunk(V, 3)[0] == 15360 and R.csr_chunk(V, 3)[1] == 304 + extra
    assert R.partitioned(V, 3, 2048) == (extra == 0)
    idx, off, rows_flat = _seam_indices(V, 3, 2048, seed=7 + extra)
    _build_and_check(dev, idx, off, V, rows_flat)


def test_partition_tiny_fields_32_and_33(dev):
    """fields of <= 32 rows count into privatised LDS counters, 33 rows into the plain ones"""
    sizes = [32, 33, 31, 1, 5000, 32, 33, 1500]
    V = sum(sizes)
    assert R.partitioned(V, len(sizes), 4099)
    idx, off, rows_flat = _uniform(sizes, 4099, 8)
    _build_and_check(dev, idx, off, V, rows_flat)


@pytest.mark.parametrize("B", [24576, 24577])
def test_partition_staged_perm_piece(dev, B):
    """a one-chunk field of more than 32 rows owns a piece of perm of exactly B positions: 24 576 is the most the fill
    pass stages in LDS, 24 577 goes out as scattered stores"""
    sizes = [100, 33, 1000]
    V = sum(sizes)
    assert R.partitioned(V, len(sizes), B) and all(32 < s <= R.csr_chunk(V, len(sizes))[0] for s in sizes)
    idx, off, rows_flat = _uniform(sizes, B, 9)
    assert int(torch.bincount(rows_flat, minlength=V)[:100].sum()) == B
    _build_and_check(dev, idx, off, V, rows_flat)


def test_partition_spill_raises_the_device_side_fall_back(dev):
    """a lookup outside its field's own range (legal as long as it stays inside the table): the partitioned kernels
    stand down on the device and the gated global-atomic kernels build the same index"""
    sizes = [2564] * 5 + [17, 1, 333, 20000, 40]
    V = sum(sizes)
    idx, off, _ = _uniform(sizes, 4096, 10)
    assert R.partitioned(V, len(sizes), 4096)
    idx[5, 0] = sizes[0] + 3                    # into field 1
    idx[77, 8] = -40                            # back into field 7
    idx[4095, 9] = -sizes[8] - 1                # field 9 -> field 7's last row
    rows_flat = (idx + off.view(1, -1)).reshape(-1)
    assert bool(((rows_flat >= 0) & (rows_flat < V)).all())
    _build_and_check(dev, idx, off, V, rows_flat)

"""The deep branch's backward without its single-purpose launches (profiles/deep_bwd_launches.md), every part against the
launches it replaces, bit for bit:

A. trs_mlp_fused_bwd_data_parts leaves the reduce launch out; trs_wgrad_finish / trs_wgrad_finish_t with partial-row
   sources fold the per-workgroup partial rows themselves, in the reduce kernel's order -- every (dW, db), the output layer's row
   included, equals reduce + plain finish on the same operands.
(B, W1's fragment copy riding in the backward's pack launch, was measured and taken out again: no entry, no test.)
C. the FM walk zeroes its queue counters in the launch that stages the FM rows: two walks on one workspace, dense and
   fused-SGD sink, equal a walk on a fresh workspace, and the counter holds one walk's entries.
D. mixed family, the tile backward at the forward's width (416) against the 512-wide form on zero-padded weights.
"""
import pytest
import torch

from exact_ref import gen

pytestmark = pytest.mark.gpu

TILE, ROW_OWNER, MIXED = 1, 2, 3
# the three stacks of tests/test_gpu_mlp_bwd_wlast.py: name, family, forward widths, x_stride, backward widths
STACKS = [("tile 512-400-400-8", TILE, [512, 400, 400, 8], 0, [512, 400, 400, 8]),
          ("mixed 416-400-400-8 on 512-wide rows", MIXED, [416, 400, 400, 8], 512, [512, 400, 400, 8]),
          ("tile 416-400-8", TILE, [416, 400, 8], 0, [416, 400, 8])]
ROWS_A = [1, 129, 32901]      # one tile; two workgroups; 257 full tiles + 5 rows: workgroup 0 sums two tiles, nparts = 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _pad32(v):
    return (v + 31) // 32 * 32


_cache = {}


def _case(dev, name, rows):
    """a real forward of the stack (its masks) and random gy / h_last, once per (stack, rows)"""
    key = (name, rows)
    if key in _cache:
        return _cache[key]
    from torecsys_amd import functional as F_
    _, fam, wf, x_stride, wb = next(s for s in STACKS if s[0] == name)
    g = gen(9101, [s[0] for s in STACKS].index(name), rows)
    L = len(wf) - 1
    Ws = [(torch.randn(o, i, generator=g) / i ** 0.5).bfloat16().to(dev) for i, o in zip(wf[:-1], wf[1:])]
    if x_stride:                # the 416-wide copy of a 400-input layer's weight: zero columns behind the 400
        Ws[0][:, 400:] = 0
    bs = [(0.1 * torch.randn(o, generator=g)).bfloat16().to(dev) for o in wf[1:]]
    x = torch.randn(rows, x_stride or wf[0], generator=g).clamp_(min=0).bfloat16().to(dev)
    _, hidden, masks, mask_in, fam_ran = F_.fused_mlp_forward_raw(x, Ws, bs, input_mask=True, family=fam, x_stride=x_stride)
    assert fam_ran == fam
    Wb = list(Ws)
    if wb[0] != wf[0]:          # the backward at the full row width: zero weight columns behind the forward's
        Wb[0] = torch.zeros(wf[1], wb[0], dtype=torch.bfloat16, device=dev)
        Wb[0][:, :wf[0]] = Ws[0]
    h_last = hidden[L - 2]
    gy = torch.randn(rows, 1, generator=g).bfloat16().to(dev)
    _cache[key] = (fam, wf, Ws, wb, Wb, masks, mask_in, h_last, gy)
    return _cache[key]


# ---------------------------------------------------------------------------------------------- A
def _finish(transposed, parts, S, dims, gws, srcs, gbs):
    """one batched finish over product jobs ``dims`` = [(R, Cc, out_rows, out_cols)] (None: a job without a product) with
    fp32 sources ``srcs`` -- vectors or partial sets"""
    from torecsys_amd import _abi, functional as F_
    F_.wgrad_finish([(parts[k], gws[k], srcs[k], gbs[k], *(d if d is not None else (0, 0, 0, gbs[k].numel())))
                     for k, d in enumerate(dims)], S, _abi.TRS_BF16, transposed=transposed)


@pytest.mark.parametrize("rows", ROWS_A)
@pytest.mark.parametrize("name", [s[0] for s in STACKS])
def test_a_finish_folds_the_partials_bit_for_bit(dev, name, rows):
    from torecsys_amd import functional as F_
    fam, _, _, wb, Wb, masks, mask_in, h_last, gy = _case(dev, name, rows)
    L = len(wb) - 1
    old = F_.fused_mlp_backward_raw(gy, wb, Wb, masks, mask_in, family=fam, h_last=h_last, live=1)
    new = F_.fused_mlp_backward_raw(gy, wb, Wb, masks, mask_in, family=fam, h_last=h_last, live=1, parts=True)
    nparts = min((rows + 127) // 128, 256)
    assert torch.equal(new[0], old[0]) and all(torch.equal(a, b) for a, b in zip(new[1], old[1]))
    assert all(t.shape == (nparts, _pad32(w)) for t, w in zip(new[2], wb[1:]))
    assert new[3].shape == (nparts, _pad32(wb[0])) and new[4].shape == (nparts, 1, _pad32(wb[L - 1]))
    # the reduce launch on its own: the vectors today's entry writes
    sets = list(new[2]) + [new[3], new[4][:, 0]]
    plain = list(old[2]) + [old[3], old[4][0]]
    for got, want in zip(F_.colsum_parts_reduce(sets), plain):
        assert torch.equal(got, want)
    # both batched finishes: a product job per hidden layer and for the layer in front (its bias gradient is gb_in), the
    # output layer's dW row and bias as jobs without a product
    g = gen(9102, rows)
    S, in_f = 3, 264
    live_w = [min(400, wb[0])] + [wb[l + 1] for l in range(L - 1)]            # rows of the weights behind the sources
    src_new = [new[3]] + list(new[2][:L - 1]) + [new[4][:, 0], new[2][L - 1]]
    src_old = [old[3]] + list(old[2][:L - 1]) + [old[4][0], old[2][L - 1]]
    cast_cols = [wb[L - 1], 1]
    for entry, transposed in (("trs_wgrad_finish", False), ("trs_wgrad_finish_t", True)):
        prods = [torch.randn((S, in_f, _pad32(o)) if transposed else (S, _pad32(o), in_f), generator=g).to(dev) for o in live_w]
        dims = [(_pad32(o), in_f, o, in_f) for o in live_w] + [None, None]
        res = []
        for srcs in (src_old, src_new):
            gws = [torch.zeros(o, in_f, dtype=torch.bfloat16, device=dev) for o in live_w]
            gbs = [torch.zeros(o, dtype=torch.bfloat16, device=dev) for o in live_w + cast_cols]
            _finish(transposed, prods + [None, None], S, dims, gws + [None, None], srcs, gbs)
            res.append(gws + gbs)
        assert all(torch.equal(a, b) for a, b in zip(*res)), entry
        assert all(float(t.float().abs().max()) > 0 for t in res[0][:len(live_w)])
    # ... and the Python route: the output layer's (dW, db) through _tail_grads
    lay_old = [(gy, h_last, 1, wb[L - 1], torch.bfloat16, old[2][-1], True, True)]
    lay_new = [(gy, h_last, 1, wb[L - 1], torch.bfloat16, new[2][-1], True, True)]
    (gw0, gb0), = F_._tail_grads(lay_old, old[4])
    (gw1, gb1), = F_._tail_grads(lay_new, new[4])
    assert torch.equal(gw0, gw1) and torch.equal(gb0, gb1)


def test_a_without_the_carried_row(dev):
    """h_last = None: the bias partials alone"""
    from torecsys_amd import functional as F_
    fam, _, _, wb, Wb, masks, mask_in, _, gy = _case(dev, STACKS[0][0], 129)
    gy8 = F_.pad_cols(gy, 8)
    old = F_.fused_mlp_backward_raw(gy8, wb, Wb, masks, mask_in, family=fam)
    new = F_.fused_mlp_backward_raw(gy8, wb, Wb, masks, mask_in, family=fam, parts=True)
    assert len(new) == 4 and torch.equal(new[0], old[0]) and all(torch.equal(a, b) for a, b in zip(new[1], old[1]))
    for got, want in zip(F_.colsum_parts_reduce(list(new[2]) + [new[3]]), list(old[2]) + [old[3]]):
        assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- C
def _walk_case(dev, B):
    """bf16, E = 64, three fields of 40 / 1 / 50 rows: row 40 collects B lookups.  Small integers everywhere, so every sum
    is exact in fp32 whatever its order and the one rounding to bf16 is the reference's too."""
    from torecsys_amd import functional as F_
    sizes, E = [40, 1, 50], 64
    V, N = sum(sizes), 3
    g = gen(9104, B)
    offsets = torch.tensor([0, 40, 41], dtype=torch.int64)
    idx = torch.cat([torch.randint(0, s, (B, 1), generator=g) for s in sizes], 1)
    g_rows = torch.randint(-1, 2, (B, N, E), generator=g).bfloat16()
    gs = torch.randint(-1, 2, (B, 1), generator=g).bfloat16()
    fm_sum = torch.randint(-2, 3, (B, E), generator=g).float()
    table = torch.randint(-1, 2, (V, E), generator=g).bfloat16()
    rows = (idx + offsets).reshape(-1)
    term = g_rows.double() + (gs.double() * fm_sum.double())[:, None, :] - gs.double()[:, None, :] * table.double()[rows].view(B, N, E)
    exact = torch.zeros(V, E, dtype=torch.float64).index_add_(0, rows, term.reshape(-1, E))
    rb = F_.row_buckets(idx.to(dev), offsets.to(dev), V)
    return rb, V, E, N, g_rows.to(dev), gs.to(dev), fm_sum.to(dev), table.to(dev), exact


@pytest.mark.parametrize("B,queued", [(1, 0), (70, 1), (600, 3)])
def test_c_two_walks_on_one_workspace(dev, B, queued):
    from torecsys_amd import _abi, functional as F_
    rb, V, E, N, g_rows, gs, fm_sum, table, exact = _walk_case(dev, B)
    ws_bytes = F_.size_query("trs_scatter_workspace_bytes", rb.BN, N, E, _abi.TRS_BF16)

    def dense(ws):
        grad = torch.full((V, E), 7.0, dtype=torch.bfloat16, device=dev)
        F_.call("trs_scatter_rows", F_.ptr(g_rows), 0, F_.ptr(gs), 1, F_.ptr(fm_sum), F_.ptr(table), F_.ptr(rb.row_start),
                F_.ptr(rb.perm), rb.BN, V, E, N, _abi.TRS_BF16, -1, F_.ptr(grad), F_.ptr(ws), ws_bytes, F_.stream_ptr())
        return grad

    def sgd(ws):
        t = table.clone()
        F_.call("trs_scatter_rows_update", F_.ptr(g_rows), 0, F_.ptr(gs), 1, F_.ptr(fm_sum), F_.ptr(t), F_.ptr(rb.row_start),
                F_.ptr(rb.perm), rb.BN, V, E, N, _abi.TRS_BF16, -1, 1, 2.0 ** -10, F_.ptr(None), 0.0, 0.0, 0.0, F_.ptr(None),
                F_.ptr(None), F_.ptr(ws), ws_bytes, F_.stream_ptr())
        return t

    for walk in (dense, sgd):
        fresh = walk(torch.zeros(ws_bytes, dtype=torch.uint8, device=dev))
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
        first = walk(ws)
        assert int(ws.view(torch.int32)[0]) == queued
        second = walk(ws)                                   # meets the first walk's count and queue
        assert int(ws.view(torch.int32)[0]) == queued
        assert torch.equal(first, fresh) and torch.equal(second, fresh), walk.__name__
    grad = dense(torch.zeros(ws_bytes, dtype=torch.uint8, device=dev))
    assert float(exact.abs().max()) < 2 ** 24 and torch.equal(grad, exact.bfloat16().to(dev))
    assert torch.equal(F_.scatter_rows(rb, table, g_rows, gs, fm_sum), grad)
    step = (table.float() - sgd(torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)).float()).cpu().double() * 2 ** 10
    assert float((step - exact).abs().max()) <= float(exact.abs().max()) * 2 ** -7 + 2 ** -7 * 2 ** 10      # one bf16 rounding of the row


# ---------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("with_h_last", [False, True])
@pytest.mark.parametrize("rows", [1, 2, 32901])
def test_d_tile_backward_at_the_forwards_width(dev, rows, with_h_last):
    from torecsys_amd import functional as F_
    fam, wf, Ws, wb, Wb, masks, mask_in, h_last, gy = _case(dev, STACKS[1][0], rows)
    assert fam == MIXED and wf[0] == 416 and wb[0] == 512
    if with_h_last:
        kw = dict(h_last=h_last, live=1)
        gyf = gy
    else:
        kw = {}
        gyf = F_.pad_cols(gy, 8)
    wide = F_.fused_mlp_backward_raw(gyf, wb, Wb, masks, mask_in, family=fam, **kw)
    narrow = F_.fused_mlp_backward_raw(gyf, wf, Ws, masks, mask_in, family=fam, **kw)
    assert narrow[0].shape == (rows, 416) and wide[0].shape == (rows, 512)
    assert torch.equal(narrow[0][:, :400], wide[0][:, :400])
    assert not bool(wide[0][:, 400:].any()) and not bool(narrow[0][:, 400:].any())      # only zero-weight columns go
    assert all(torch.equal(a, b) for a, b in zip(narrow[1], wide[1]))
    assert all(torch.equal(a, b) for a, b in zip(narrow[2], wide[2]))
    assert narrow[3].shape == (416,) and torch.equal(narrow[3][:400], wide[3][:400])
    if with_h_last:
        assert torch.equal(narrow[4], wide[4])

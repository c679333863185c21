"""The output layer's weight gradient inside the fused MLP backward (trs_mlp_fused_bwd_data_wlast, csrc/mlp_fused.hip): the
tile kernel streams the last hidden activation beside its GEMMs, multiplies every row by the row's output gradient (which
it holds in LDS) and sums the rows per workgroup; the entry's reduce launch folds the workgroups in a fixed order.  The same
entry reads a contiguous (rows, live) output gradient where it lies instead of a copy padded to 8 columns.

Exact cases in the manner of profiles/mfma_exact_cases.md: ``h_last`` is only a pointer argument, so it is handed over with
values in {0, 1}; gy is in {-1, 0, 1} with at most 256 non-zero rows, so every sum is an integer of magnitude <= 256 --
exact in fp32 and in bf16 -- and the comparison is torch.equal against a float64 product.  Everything else the entry
writes is compared bit for bit with trs_mlp_fused_bwd_data on the same operands."""
import pytest
import torch

from exact_ref import gen

pytestmark = pytest.mark.gpu

TILE, ROW_OWNER, MIXED = 1, 2, 3
ROWS = [1, 2, 32901]            # the smallest count the entry admits, one more, 257 full tiles + 5 rows
# (name, family, forward widths, forward x_stride, backward widths)
STACKS = [("tile 512-400-400-8", TILE, [512, 400, 400, 8], 0, [512, 400, 400, 8]),
          ("mixed 416-400-400-8 on 512-wide rows", MIXED, [416, 400, 400, 8], 512, [512, 400, 400, 8]),
          ("tile 416-400-8", TILE, [416, 400, 8], 0, [416, 400, 8])]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _pad32(v):
    return (v + 31) // 32 * 32


def _nonzero_rows(rows):
    """first and last row of the first, second and last full tile, one row in every 16-row group of tile 1 (a different
    place in each), the ragged tail; at most 256 of them"""
    want = {0, 127, 128, 255}
    want |= {128 + 16 * k + (5 * k + 3) % 16 for k in range(8)}
    last_full = (rows // 128 - 1) * 128
    if last_full >= 0:
        want |= {last_full, last_full + 127}
    want |= set(range(rows // 128 * 128, rows))            # the ragged tail
    want |= {256 * 128, 256 * 128 + 127}                   # the second tile of workgroup 0
    return sorted(r for r in want if 0 <= r < rows)[:256]


_cache = {}


def _case(dev, name, rows):
    """a real forward of the stack (its masks), integer gy / h_last, and the results of today's entry -- computed once per
    (stack, rows) and left unchanged"""
    key = (name, rows)
    if key in _cache:
        return _cache[key]
    from torecsys_amd import functional as F_
    _, fam, wf, x_stride, wb = next(s for s in STACKS if s[0] == name)
    g = gen(7101, [s[0] for s in STACKS].index(name), rows)
    L = len(wf) - 1
    Ws = [(torch.randn(o, i, generator=g) / i ** 0.5).bfloat16().to(dev) for i, o in zip(wf[:-1], wf[1:])]
    bs = [(0.1 * torch.randn(o, generator=g)).bfloat16().to(dev) for o in wf[1:]]
    x = torch.randn(rows, x_stride or wf[0], generator=g).clamp_(min=0).bfloat16().to(dev)
    _, hidden, masks, mask_in, fam_ran = F_.fused_mlp_forward_raw(x, Ws, bs, input_mask=True, family=fam, x_stride=x_stride)
    assert fam_ran == fam
    Wb = list(Ws)
    if wb[0] != wf[0]:          # the backward sees the full row width: zero weight columns behind the forward's
        Wb[0] = torch.zeros(wf[1], wb[0], dtype=torch.bfloat16, device=dev)
        Wb[0][:, :wf[0]] = Ws[0]
    Kh = _pad32(wb[L - 1])
    h_last = torch.randint(0, 2, (rows, Kh), generator=g).bfloat16().to(dev)
    gy = torch.zeros(rows, 8, dtype=torch.bfloat16)
    nz = _nonzero_rows(rows)
    gy[nz, 0] = (torch.randint(0, 2, (len(nz),), generator=g) * 2 - 1).bfloat16()
    gy[nz, 1] = (torch.randint(-1, 2, (len(nz),), generator=g)).bfloat16()
    gy = gy.to(dev)
    old = {}
    for live in (1, 2):
        gyl = gy.clone()
        gyl[:, live:] = 0
        old[live] = (gyl, F_.fused_mlp_backward_raw(gyl, wb, Wb, masks, mask_in, family=fam))
    torch.cuda.synchronize()
    _cache[key] = (fam, wb, Wb, masks, mask_in, h_last, old)
    return _cache[key]


def _same(new, old):
    gx, gz, gb, gb_in = new[:4]
    assert torch.equal(gx, old[0])
    assert len(gz) == len(old[1]) and all(torch.equal(a, b) for a, b in zip(gz, old[1]))
    assert len(gb) == len(old[2]) and all(torch.equal(a, b) for a, b in zip(gb, old[2]))
    assert torch.equal(gb_in, old[3])


@pytest.mark.parametrize("live", [1, 2])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", [s[0] for s in STACKS])
def test_exact_row_and_unchanged_neighbours(dev, name, rows, live):
    from torecsys_amd import functional as F_
    fam, wb, Wb, masks, mask_in, h_last, old = _case(dev, name, rows)
    gyl, ref = old[live]
    assert F_.mlp_bwd_wlast_bytes(wb, rows, fam, live) == min((rows + 127) // 128, 256) * live * h_last.shape[1] * 4
    want = (gyl[:, :live].double().t() @ h_last.double())
    assert float(want.abs().max()) <= 256
    for form in (gyl, gyl[:, :live].contiguous()):          # padded to 8 columns, and where it lies
        new = F_.fused_mlp_backward_raw(form, wb, Wb, masks, mask_in, family=fam, h_last=h_last, live=live)
        _same(new, ref)
        assert new[4].dtype == torch.float32 and new[4].shape == (live, h_last.shape[1])
        assert torch.equal(new[4].double(), want)
    # the cast that rides in the finish launch: exact as well, sliced to the weight's shape
    in_f = wb[-2]
    layers = [(gyl, h_last, live, in_f, torch.bfloat16, ref[2][-1], True, True)]
    (gw, gbias), = F_._tail_grads(layers, new[4])
    assert gw.shape == (live, in_f) and torch.equal(gw.double(), want[:, :in_f])
    assert torch.equal(gbias, ref[2][-1][:live].bfloat16())


def test_random_operands_against_the_separate_product(dev):
    """8192 rows of random operands: the row the kernel sums against today's product + finish, both rounded once to bf16 from
    fp32 sums taken in different orders -- within 2^-7 of the largest entry; and two runs give identical bits"""
    from torecsys_amd import functional as F_
    name, rows = STACKS[0][0], 8192
    fam, wb, Wb, masks, mask_in, _, _ = _case(dev, name, rows)
    g = gen(7102, rows)
    h_last = torch.randn(rows, 416, generator=g).clamp_(min=0).bfloat16()
    h_last[:, 400:] = 0
    h_last = h_last.to(dev)
    gy1 = torch.randn(rows, 1, generator=g).bfloat16().to(dev)
    gy8 = F_.pad_cols(gy1, 8)
    ref = F_.fused_mlp_backward_raw(gy8, wb, Wb, masks, mask_in, family=fam)
    (gw_old, gb_old), = F_._tail_grads([(gy8, h_last, 1, 400, torch.bfloat16, ref[2][-1], True, True)])
    runs = []
    for _ in range(2):
        new = F_.fused_mlp_backward_raw(gy1, wb, Wb, masks, mask_in, family=fam, h_last=h_last, live=1)
        _same(new, ref)          # B: the (rows, 1) gradient read where it lies, every other output bit for bit
        runs.append(F_._tail_grads([(gy1, h_last, 1, 400, torch.bfloat16, new[2][-1], True, True)], new[4])[0])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    gw_new, gb_new = runs[0]
    ratio = float((gw_new.float() - gw_old.float()).abs().max() / gw_old.float().abs().max())
    print(f"max|new - old| / max|old| = {ratio:.3e}")
    assert ratio <= 2 ** -7
    assert torch.equal(gb_new, gb_old)
    f64 = gy1.double().t() @ h_last.double()
    assert float((new[4].double() - f64).abs().max() / f64.abs().max()) <= 1e-5          # the fp32 sum itself


def _record_calls(monkeypatch, n_jobs=None):
    """the names of the entries called; ``n_jobs``: a list that takes (name, job count) of every finish, of both orientations"""
    from torecsys_amd import functional as F_
    names, orig = [], F_.call

    def record(name, *a):
        names.append(name)
        if n_jobs is not None and name in ("trs_wgrad_finish", "trs_wgrad_finish_t"):
            n_jobs.append((name, a[0]))
        return orig(name, *a)

    monkeypatch.setattr(F_, "call", record)
    return names


def test_deep_branch_graphed_replays_equal_eager(dev, monkeypatch):
    """the 2496-400-400-400-1 module at 8192 rows: the step takes the new entry (no padded copy of the logit gradient, no
    product or finish launch for the output layer), and three replays of the captured step equal the eager step"""
    from torecsys_amd import layers as L
    from torecsys_amd.graph import GraphedStep
    torch.manual_seed(11)
    lay = L.DNNLayer(inputs_size=2496, output_size=1, layer_sizes=[400, 400, 400]).to(dev).bfloat16()
    params = list(lay.parameters())
    g = gen(7103)
    batches = [((0.5 * torch.randn(8192, 2496, generator=g)).bfloat16().to(dev), torch.randn(8192, 1, generator=g).to(dev))
               for _ in range(3)]

    def fn(x, lab):
        loss = ((lay(x).rename(None).float() - lab) ** 2).mean()
        loss.backward()
        return loss

    n_jobs = []
    names = _record_calls(monkeypatch, n_jobs)
    eager = []
    for x, lab in batches:
        for p in params:
            p.grad = None
        loss = fn(x, lab)
        eager.append((loss.detach().clone(), [p.grad.clone() for p in params]))
    del loss
    assert "trs_mlp_fused_bwd_data_wlast" in names
    # Per step one batched finish (two or more jobs: the tail layers with the output layer's casts) and no one-job finish of
    # that orientation; the only other finish is the first layer's own, one transposed job behind trs_wgrad_wide.
    print("finish calls (entry, jobs):", n_jobs)
    plain = [n for name, n in n_jobs if name == "trs_wgrad_finish"]
    assert len(plain) == len(batches) and all(n >= 2 for n in plain)
    assert [n for name, n in n_jobs if name == "trs_wgrad_finish_t"] == [1] * len(batches)
    assert not {"trs_pad_cols", "trs_mlp_fused_bwd_data", "trs_wgrad_rows"} & set(names)
    step = GraphedStep(fn, batches[0], params=params, warmup=2)
    for (x, lab), (l0, g0) in zip(batches, eager):
        loss = step(x, lab)
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), l0)
        for p, gref in zip(params, g0):
            assert torch.equal(p.grad, gref)


def test_declines(dev, monkeypatch):
    """too many live columns, fp32, the row-owner family: the query answers 0, the entry returns an error code before any
    launch, and a layer whose output is too wide keeps today's path and today's result"""
    from torecsys_amd import _abi, functional as F_, layers as L
    fam, wb, Wb, masks, mask_in, h_last, old = _case(dev, STACKS[0][0], 2)
    assert F_.mlp_bwd_wlast_bytes(wb, 2, fam, 4) == 0 and F_.mlp_bwd_wlast_bytes(wb, 2, fam, 0) == 0
    assert F_.mlp_bwd_wlast_bytes(wb, 2, ROW_OWNER, 1) == 0
    assert F_.mlp_bwd_wlast_bytes([64, 400, 400, 400, 64], 1 << 20, ROW_OWNER, 1) == 0
    assert F_.size_query("trs_mlp_fused_bwd_wlast_part_bytes", 3, F_._i32_array(wb), 2, _abi.TRS_F32, fam, 1) == 0
    assert F_.mlp_bwd_wlast_bytes([512, 8], 2, TILE, 1) == 0                     # no hidden layer in the stack
    assert F_.mlp_bwd_wlast_bytes([64] + [72] * 5 + [8], 2, TILE, 1) > 0         # 6 + 1 + 1 entries of the reduce launch
    assert F_.mlp_bwd_wlast_bytes([64] + [72] * 6 + [8], 2, TILE, 1) == 0        # 7 + 1 + 1 do not fit
    with pytest.raises(RuntimeError):
        F_.fused_mlp_backward_raw(old[1][0], wb, Wb, masks, mask_in, family=fam, h_last=h_last, live=4)
    torch.manual_seed(5)
    lay = L.DNNLayer(inputs_size=2496, output_size=4, layer_sizes=[400, 400]).to(dev).bfloat16()
    x = (0.5 * torch.randn(8192, 2496, device=dev)).bfloat16()
    go = torch.randn(8192, 4, device=dev).bfloat16()
    names = _record_calls(monkeypatch)
    lay(x).rename(None).backward(go)
    assert "trs_mlp_fused_bwd_data" in names and "trs_mlp_fused_bwd_data_wlast" not in names
    lin = [m for m in lay.model if isinstance(m, torch.nn.Linear)]
    h = x.float()
    for m in lin[:-1]:
        h = torch.relu(h @ m.weight.float().t() + m.bias.float()).bfloat16().float()
    want = (go.float().t() @ h).detach()
    got = lin[-1].weight.grad.detach().float()
    assert float((got - want).abs().max() / want.abs().max()) <= 2e-2

"""GPU tests of attention pooling over ragged bags (RaggedListIndicesEmbedding(use_attn=True),
functional.attn_pool_ragged[_layer], the ragged kernels of csrc/attn_pool.hip) against the fp64 restatement
tests/attn_ragged_ref.py (pinned to nn.MultiheadAttention by tests/test_attn_ragged_host.py).  Tolerances are those of
tests/test_gpu_list_attn.py: fp32 1e-5 relative; bf16 max(1e-2, 2 x e_aten), e_aten the error of the bf16 ATen composition
(pad + nn.MultiheadAttention(key_padding_mask) + masked pooling) on the same inputs."""
import pytest
import torch

from attn_ragged_ref import live_positions, parity_lengths, ragged_attn, ragged_attn_with
from bag_ragged_ref import bags_from_lengths
from conftest import rel_err
from list_attn_ref import ATTN_KEYS, make_attention

pytestmark = pytest.mark.gpu

TOL32 = 1e-5
TOLBF = 1e-2
V, PAD = 300, 0
KEYS = ["embedding.weight"] + ATTN_KEYS
# (ids dtype, offsets dtype, include_last_offset)
FORMS = [(torch.int64, torch.int64, True), (torch.int32, torch.int32, False), (torch.int64, torch.int32, False),
         (torch.int32, torch.int64, True)]
SHAPES = [(64, 1), (64, 4), (128, 8), (16, 2), (10, 5)]
MODES = [("sum", False), ("mean", True), ("sum", True), ("mean", False)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _rounded_attention(E, H, g, dtype, bias=True):
    attn = make_attention(E, H, bias, generator=g)
    with torch.no_grad():
        for p in attn.parameters():
            p.copy_(p.to(dtype).float())                                      # the rounded parameters are THE parameters
    return attn


def _module(dev, E, H, method, attn, w, dtype=torch.float32, **kw):
    from torecsys_amd.inputs import RaggedListIndicesEmbedding
    m = RaggedListIndicesEmbedding(embed_size=E, field_size=w.shape[0], output_method=method, use_attn=True, num_heads=H,
                                   bias=attn.in_proj_bias is not None, **kw)
    sd = {"embedding.weight": w}
    sd.update({"attention." + k: p.detach() for k, p in attn.named_parameters()})
    m.load_state_dict(sd)
    return m.to(dev).to(dtype)


def _form(ids, offsets, form, dev):
    idt, odt, last = form
    if not last:                                                              # the last bag runs to n: no trailing ids
        ids, offsets = ids[:int(offsets[-1])], offsets[:-1]
    return ids, offsets, ids.to(dev).to(idt), offsets.to(dev).to(odt), last


def _run(m, ids_d, off_d, gout_d):
    for p in m.parameters():
        p.grad = None
    y = m(ids_d, off_d)
    assert y.names == ("B", "N", "E")
    y = y.rename(None)
    (y * gout_d).sum().backward()
    return y.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _errors(y, grads, want):
    errs = {"out": rel_err(y.float().cpu(), want["y"])}
    for k in KEYS:
        errs[k] = rel_err(grads[k].float().cpu(), want[k])
    return errs


def _aten_padded(dev, w, attn, ids, taken, mode, gout, dtype, L):
    """the ATen composition on the device in ``dtype``: the taken ids of every bag padded to L, nn.MultiheadAttention with a
    key_padding_mask, masked sum / mean (a bag that takes nothing is a zero row: ATen's softmax would give NaN there)"""
    B, E = len(taken), w.shape[1]
    idx = torch.full((B, L), PAD, dtype=torch.int64)
    mask = torch.ones(B, L, dtype=torch.bool)
    for b, pos in enumerate(taken):
        idx[b, :len(pos)] = ids[torch.tensor(pos, dtype=torch.int64)]
        mask[b, :len(pos)] = False
    live = (~mask.all(dim=1)).nonzero().flatten().to(dev)
    idx, mask = idx.to(dev)[live], mask.to(dev)[live]
    a = make_attention(E, attn.num_heads, True, params={k: p for k, p in attn.named_parameters()}).to(dev).to(dtype)
    wl = w.to(dtype).to(dev).requires_grad_()
    seq = torch.nn.functional.embedding(idx, wl).transpose(0, 1)
    o, _ = a(seq, seq, seq, key_padding_mask=mask, need_weights=False)
    o = (o.transpose(0, 1) * (~mask).unsqueeze(-1)).sum(dim=1)
    if mode == "mean":
        o = o / (~mask).sum(dim=1, keepdim=True)
    y = torch.zeros(B, 1, E, dtype=dtype, device=dev).index_add(0, live, o.unsqueeze(1).to(dtype))
    (y * gout.to(dev).to(dtype)).sum().backward()
    grads = {"embedding.weight": wl.grad.clone()}
    grads["embedding.weight"][PAD] = 0
    grads.update({"attention." + k: p.grad for k, p in a.named_parameters()})
    return y.detach(), grads


def _parity_batch(g):
    """B = 97 bags: the fixed boundary lengths, then long / short alternating; padding ids sprinkled in (interleaved), bag 7
    with leading and bag 9 with trailing padding, bags 21 and 41 (long ones) of nothing but padding; 5 ids behind the last bag"""
    lengths = parity_lengths(g)
    ids, offsets = bags_from_lengths(g, lengths, V, PAD, trailing=5, sprinkle=0.15, all_pad=(21, 41))
    ids[int(offsets[7]):int(offsets[7]) + 6] = PAD                            # bag 7 (32 ids): leading padding
    ids[int(offsets[10]) - 9:int(offsets[10])] = PAD                          # bag 9 (63 ids): trailing padding
    return ids, offsets


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("me", range(4), ids=["sum", "mean_excl", "sum_excl", "mean"])
@pytest.mark.parametrize("sh", range(5), ids=["E%d_H%d" % s for s in SHAPES])
def test_parity_with_the_restatement(dev, sh, me, dtype):
    """the output, the table gradient (padding row exactly zero) and all four attention parameters; every (E, H) meets
    every index / offset form, both modes and exclude_padding on and off, in both dtypes"""
    from torecsys_amd import functional as F_
    (E, H), (mode, exclude), form = SHAPES[sh], MODES[me], FORMS[(sh + me) % 4]
    g = torch.Generator().manual_seed(1000 + 10 * sh + me)
    ids, offsets = _parity_batch(g)
    w = (torch.randn(V, E, generator=g) * 0.5).to(dtype).float()
    attn = _rounded_attention(E, H, g, dtype)
    ids, offsets, ids_d, off_d, last = _form(ids, offsets, form, dev)
    B = offsets.numel() - 1 if last else offsets.numel()
    assert B == 97
    gout = torch.randn(B, 1, E, generator=g).to(dtype).float()
    want = ragged_attn_with(w.double(), ids, offsets, attn, mode, 64, pad=PAD, exclude=exclude, include_last_offset=last,
                            gout=gout.double())
    assert not any(want["over"]) and want["cnt"][0] == 0 and (want["cnt"][21] == 0) == exclude
    assert F_.attn_pool_path(64, E, H, dtype) == (2 if dtype == torch.bfloat16 and E % 16 == 0 and (E // H) % 16 == 0
                                                  else 1)
    torch.cuda.synchronize()
    F_.index_errors_seen()
    m = _module(dev, E, H, mode, attn, w, dtype, max_length=64, exclude_padding=exclude, include_last_offset=last)
    y, grads = _run(m, ids_d, off_d, gout.to(dev).to(dtype))
    assert tuple(y.shape) == (B, 1, E) and y.dtype == dtype
    assert not F_.index_errors_seen()
    assert float(grads["embedding.weight"][PAD].abs().max()) == 0.0
    assert float(y[0].abs().max()) == 0.0                                     # the empty bag: an exact zero row
    if exclude:
        assert float(y[21].abs().max()) == 0.0 and float(y[41].abs().max()) == 0.0
    got = _errors(y, grads, want)
    if dtype == torch.float32:
        for k, e in got.items():
            print(f"fp32 E={E} H={H} {mode} excl={exclude} {k}: {e:.3e}")
        for k, e in got.items():
            assert e <= TOL32, (k, e)
        return
    taken, _ = live_positions(ids, offsets, 64, PAD, exclude, last)
    aten = _errors(*_aten_padded(dev, w, attn, ids, taken, mode, gout, dtype, 64), want)
    for k in got:
        print(f"bf16 E={E} H={H} {mode} excl={exclude} {k}: fused {got[k]:.3e} aten {aten[k]:.3e}")
    for k in got:
        assert got[k] <= max(TOLBF, 2 * aten[k]), (k, got[k], aten[k])


# ------------------------------------------------------------------------------------------------ 2. the cap and the flag
def _cap_batch(g, long_bags):
    """bags of 19 and 20 live ids and, with ``long_bags``, of 21 and 100; padding ids interleaved (so a live id's rank is
    not its position); the live ids beyond the 20th of the long bags are 200 .. 280, which occur nowhere else"""
    live = [19, 20, 3] + ([21, 100] if long_bags else []) + [7]
    parts, lens, fresh = [], [], 200
    for Lb in live:
        bag = []
        for j in range(Lb):
            if j >= 20:
                bag.append(fresh)
                fresh += 1
            else:
                bag.append(int(torch.randint(1, 200, (1,), generator=g)))
            if j % 3 == 1:
                bag.append(PAD)
        parts += bag
        lens.append(len(bag))
    assert fresh <= V
    return torch.tensor(parts), torch.tensor([0] + lens).cumsum(0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_max_length_caps_a_bag_and_raises_the_flag(dev, dtype):
    from torecsys_amd import functional as F_
    E, H = 16, 1
    tol = TOL32 if dtype == torch.float32 else TOLBF
    for long_bags in (True, False):
        g = torch.Generator().manual_seed(77)
        ids, offsets = _cap_batch(g, long_bags)
        w = (torch.randn(V, E, generator=g) * 0.5).to(dtype).float()
        attn = _rounded_attention(E, H, g, dtype)
        B = offsets.numel() - 1
        gout = torch.randn(B, 1, E, generator=g).to(dtype).float()
        want = ragged_attn_with(w.double(), ids, offsets, attn, "mean", 20, pad=PAD, exclude=True,
                                include_last_offset=True, gout=gout.double())
        assert want["over"] == ([False, False, False, True, True, False] if long_bags else [False] * 4)
        assert want["cnt"].tolist() == ([19, 20, 3, 20, 20, 7] if long_bags else [19, 20, 3, 7])
        torch.cuda.synchronize()
        F_.index_errors_seen()
        m = _module(dev, E, H, "mean", attn, w, dtype, max_length=20, exclude_padding=True, include_last_offset=True)
        y, grads = _run(m, ids.to(dev), offsets.to(dev), gout.to(dev).to(dtype))
        assert F_.index_errors_seen() is long_bags
        for k, e in _errors(y, grads, want).items():
            assert e <= tol, (k, e, long_bags)
        if long_bags:      # the ids that were not taken: exactly zero gradient
            assert float(want["embedding.weight"][200:].abs().max()) == 0.0
            assert float(grads["embedding.weight"][200:].abs().max()) == 0.0
            xt, cnt = F_.attn_pool_ragged(m.embedding.weight.detach(), ids.to(dev), offsets.to(dev),
                                          m.attention.in_proj_weight[:2 * E].detach(), None, H, "mean", PAD, max_length=20,
                                          exclude_padding=True, include_last_offset=True)
            assert cnt.tolist() == want["cnt"].tolist() and cnt.dtype == torch.float32 and not cnt.requires_grad
            F_.index_errors_seen()


def test_out_of_range_id_and_decreasing_offsets(dev):
    """each raises the flag; the out-of-range id reads as a zero row that takes part, the bag of the decreasing pair is
    empty, and neither leaks into another row of the output or of the table gradient"""
    from torecsys_amd import functional as F_
    E, H = 16, 2
    g = torch.Generator().manual_seed(5)
    w = torch.randn(V, E, generator=g) * 0.5
    attn = make_attention(E, H, True, generator=g)
    n = 30
    good_ids = torch.randint(1, V, (n,), generator=g)
    good_off = torch.tensor([0, 4, 9, 9])                                     # ids 9 .. 29 belong to no bag
    bad_ids = good_ids.clone()
    bad_ids[5], bad_ids[2] = V + 7, -3
    bad_off = torch.tensor([0, 4, 9, 6])                                      # 9 > 6: bag 2 is empty (no bags overlap)
    gout = torch.randn(3, 1, E, generator=g)
    torch.cuda.synchronize()
    F_.index_errors_seen()
    for ids, off, flagged in ((good_ids, good_off, False), (bad_ids, good_off, True), (good_ids, bad_off, True)):
        want = ragged_attn_with(w.double(), ids, off, attn, "sum", 64, pad=PAD, include_last_offset=True, gout=gout.double())
        m = _module(dev, E, H, "sum", attn, w, max_length=64, include_last_offset=True)
        y, grads = _run(m, ids.to(dev), off.to(dev), gout.to(dev))
        assert F_.index_errors_seen() is flagged
        for k, e in _errors(y, grads, want).items():
            assert e <= TOL32, (k, e, flagged)
        assert float(y[2].abs().max()) == 0.0


def test_no_ids_and_no_bags(dev):
    from torecsys_amd import functional as F_
    E, H = 16, 2
    g = torch.Generator().manual_seed(6)
    attn = make_attention(E, H, True, generator=g)
    m = _module(dev, E, H, "sum", attn, torch.randn(V, E, generator=g), max_length=8)
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    y, grads = _run(m, none, torch.zeros(3, dtype=torch.int64, device=dev), torch.ones(3, 1, E, device=dev))
    assert tuple(y.shape) == (3, 1, E) and float(y.abs().max()) == 0.0
    assert all(float(v.abs().max()) == 0.0 for k, v in grads.items() if "out_proj" not in k)
    y = m(torch.ones(4, dtype=torch.int64, device=dev), none)
    assert tuple(y.shape) == (0, 1, E)
    assert not F_.index_errors_seen()


# ------------------------------------------------------------------------------------------------ 3. the padded kernel
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("L", [5, 33, 64])
def test_bags_of_one_length_equal_the_padded_layer(dev, L, mode):
    """every bag of length L = max_length, no exclusion: functional.attn_pool_layer on ids.view(B, L), output and every
    gradient"""
    from torecsys_amd import functional as F_
    B, E, H = 97, 64, 4
    g = torch.Generator().manual_seed(50 + L)
    ids = torch.randint(0, V, (B * L,), generator=g).to(dev)
    offsets = (torch.arange(B) * L).to(dev)
    w = (torch.randn(V, E, generator=g) * 0.5).to(dev)
    attn = make_attention(E, H, True, generator=g).to(dev)
    gout = torch.randn(B, 1, E, generator=g).to(dev)
    a = attn
    res = []
    for ragged in (False, True):
        leaves = [t.detach().clone().requires_grad_() for t in (w, a.in_proj_weight, a.in_proj_bias, a.out_proj.weight,
                                                                 a.out_proj.bias)]
        if ragged:
            y = F_.attn_pool_ragged_layer(leaves[0], ids, offsets, *leaves[1:], H, mode, PAD, max_length=L)
        else:
            y = F_.attn_pool_layer(leaves[0], ids.view(B, L), *leaves[1:], H, mode, PAD)
        (y * gout).sum().backward()
        res.append([y.detach()] + [t.grad for t in leaves])
    for i, (p, r) in enumerate(zip(*res)):
        assert rel_err(r.cpu(), p.cpu()) <= TOL32, i


# ------------------------------------------------------------------------------------------------ 4. exact operands
def _exact_batch(g, exclude):
    """33 bags whose LIVE counts are powers of two (1 .. 64), shuffled; with ``exclude`` padding ids are interleaved"""
    counts = [1, 2, 4, 8, 16, 32, 64] * 5
    counts = [counts[i] for i in torch.randperm(len(counts), generator=g).tolist()][:33]
    parts, lens = [], []
    for Lb in counts:
        bag = []
        for _ in range(Lb):
            bag.append(int(torch.randint(1, V, (1,), generator=g)))
            if exclude and int(torch.randint(0, 4, (1,), generator=g)) == 0:
                bag.append(PAD)
        parts += bag
        lens.append(len(bag))
    return torch.tensor(parts), torch.tensor([0] + lens).cumsum(0), counts


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("E,H", [(64, 4), (32, 2), (16, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16_mfma"])
def test_exact_integer_operands(dev, dtype, E, H, mode, exclude):
    """Wq = 0 and bq = 0: every score is 0, P = 1 / L_b, pbar = c exactly for L_b in {1, 2, 4, 8, 16, 32, 64}; table entries
    are integers in [-4, 4] and the gradient of xt is in {-1, 0, 1}, so xt = c sum X, dX = c sum_h g_h and every fp32 sum
    is exact in any order: xt, cnt and the table gradient equal the fp64 result rounded once (d = 16: 1 / sqrt(d) exact)."""
    from torecsys_amd import functional as F_
    g = torch.Generator().manual_seed(E + H)
    ids, offsets, counts = _exact_batch(g, exclude)
    B = len(counts)
    w = torch.randint(-4, 5, (V, E), generator=g).double()
    w_qk = torch.cat([torch.zeros(E, E), torch.randint(-1, 2, (E, E), generator=g).float()]).double()
    b_qk = torch.cat([torch.zeros(E), torch.randint(-1, 2, (E,), generator=g).float()]).double()
    gxt = torch.randint(-1, 2, (B, H, E), generator=g).double()
    in_w = torch.cat([w_qk, torch.zeros(E, E, dtype=torch.float64)])          # the value rows play no part in xt
    in_b = torch.cat([b_qk, torch.zeros(E, dtype=torch.float64)])
    want = ragged_attn(w, ids, offsets, in_w, in_b, torch.eye(E, dtype=torch.float64), None, H, mode, 64, pad=PAD,
                       exclude=exclude, include_last_offset=True, gxt=gxt)
    assert want["cnt"].tolist() == [float(c) for c in counts]
    assert F_.attn_pool_path(64, E, H, dtype) == (2 if dtype == torch.bfloat16 else 1)
    wd = w.to(dtype).to(dev).requires_grad_()
    xt, cnt = F_.attn_pool_ragged(wd, ids.to(dev), offsets.to(dev), w_qk.to(dtype).to(dev), b_qk.to(dtype).to(dev), H, mode,
                                  PAD, max_length=64, exclude_padding=exclude, include_last_offset=True)
    (xt * gxt.to(dtype).to(dev)).sum().backward()
    assert torch.equal(cnt.cpu(), want["cnt"])
    bad = [c for b, c in enumerate(counts) if not torch.equal(xt[b].detach().cpu(), want["xt"][b].to(dtype))]
    assert not bad, f"xt inexact for live counts {sorted(set(bad))}"
    assert torch.equal(wd.grad.cpu(), want["embedding.weight"].to(dtype))


# ------------------------------------------------------------------------------------------------ 5. reproducible bits
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_several_samples_per_workgroup_and_reproducible_bits(dev, dtype):
    """B = 2000 bags on at most B / 3 workgroups: the per-workgroup partials accumulate across samples; the same call twice
    gives the same bits for the output and every gradient.  The same call: the same ids tensor -- the table gradient is
    summed in the order of the row buckets of ``ids``, which the bucket build fixes once per ids tensor (its order inside a
    bucket is not specified, and is not these kernels': tests/test_gpu_bag_ragged.py says the same of its own)."""
    from torecsys_amd import _abi
    B, E, H = 2000, 64, 4
    code = _abi.TRS_F32 if dtype == torch.float32 else _abi.TRS_BF16
    blocks = _abi.size_query("trs_attn_pool_ragged_blocks", B, 64, E, H, code, 1)
    assert 1 <= blocks and B >= 3 * blocks, blocks
    g = torch.Generator().manual_seed(19)
    lengths = torch.randint(0, 41, (B,), generator=g).tolist()
    ids, offsets = bags_from_lengths(g, lengths, V, PAD, trailing=3, sprinkle=0.1)
    attn = make_attention(E, H, True, generator=g)
    w = torch.randn(V, E, generator=g) * 0.5
    gout = torch.randn(B, 1, E, generator=g).to(dev).to(dtype)
    ids_d, off_d = ids.to(dev), offsets.to(dev)
    res = []
    for _ in range(2):
        m = _module(dev, E, H, "mean", attn, w, dtype, max_length=64, exclude_padding=True, include_last_offset=True)
        res.append(_run(m, ids_d, off_d, gout))
    assert torch.equal(res[0][0], res[1][0]) and float(res[0][0].abs().max()) > 0
    for k in KEYS:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
        assert float(res[0][1][k].abs().max()) > 0, k


# ------------------------------------------------------------------------------------------------ 6. hipGraph capture
def test_graphed_forward_backward_matches_eager(dev):
    """no host value depends on the lengths: a graph captured on one batch replays on another of the same n and B"""
    from torecsys_amd.graph import GraphedStep
    B, E, H = 256, 32, 2
    g = torch.Generator().manual_seed(3)
    attn = make_attention(E, H, True, generator=g)
    m = _module(dev, E, H, "mean", attn, torch.randn(V, E, generator=g), max_length=48, exclude_padding=True)
    params = list(m.parameters())
    proj = torch.randn(1, 1, E, generator=g).to(dev)
    lengths = torch.randint(0, 49, (B,), generator=g)
    batches = []
    for _ in range(3):
        lens = lengths[torch.randperm(B, generator=g)].tolist()              # the same n, other bags
        ids, offsets = bags_from_lengths(g, lens, V, PAD, sprinkle=0.1)
        batches.append((ids.to(dev), offsets[:-1].to(dev), torch.randn(B, 1, generator=g).to(dev)))
    assert len({b[0].numel() for b in batches}) == 1

    def fn(ids, off, lab):
        loss = (((m(ids, off).rename(None) * proj).sum(-1) - lab) ** 2).mean()
        loss.backward()
        return loss

    eager = []
    for batch in batches:
        for p in params:
            p.grad = None
        loss = fn(*batch)
        eager.append((loss.detach().clone(), [p.grad.clone() for p in params]))
    del loss
    step = GraphedStep(fn, batches[0], params=params, warmup=2)
    for batch, (l0, g0) in zip(batches, eager):
        loss = step(*batch)
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), l0)
        for p, gp in zip(params, g0):
            assert rel_err(p.grad.cpu(), gp.cpu()) <= TOL32


# ------------------------------------------------------------------------------------------------ 7. module and router
def test_module_checkpoint_names_and_inputs_route(dev):
    from torecsys_amd import functional as F_
    from torecsys_amd.inputs import Inputs, ListIndicesEmbedding, RaggedListIndicesEmbedding
    E, H = 16, 2
    g = torch.Generator().manual_seed(8)
    ids, offsets = bags_from_lengths(g, [3, 0, 12, 1, 7], V, PAD, trailing=2, sprinkle=0.2)
    old = ListIndicesEmbedding(embed_size=E, field_size=V, use_attn=True, num_heads=H).to(dev)
    m = RaggedListIndicesEmbedding(embed_size=E, field_size=V, use_attn=True, num_heads=H, max_length=16,
                                   exclude_padding=True, include_last_offset=True).to(dev)
    assert list(m.state_dict().keys()) == list(old.state_dict().keys())
    m.load_state_dict(old.state_dict())                      # a ListIndicesEmbedding(use_attn=True) checkpoint loads
    out = m(ids.to(dev), offsets.to(dev))
    assert out.names == ("B", "N", "E") and tuple(out.shape) == (5, 1, E)
    cpu = torch.nn.MultiheadAttention(E, H)
    cpu.load_state_dict({k: v.cpu() for k, v in m.attention.state_dict().items()})
    want = ragged_attn_with(m.embedding.weight.detach().cpu().double(), ids, offsets, cpu, "mean", 16, pad=PAD,
                            exclude=True, include_last_offset=True)
    assert rel_err(out.rename(None).cpu(), want["y"]) <= TOL32
    a = m.attention
    direct = F_.attn_pool_ragged_layer(m.embedding.weight, ids.to(dev), offsets.to(dev), a.in_proj_weight, a.in_proj_bias,
                                       a.out_proj.weight, a.out_proj.bias, H, "mean", PAD, max_length=16,
                                       exclude_padding=True, include_last_offset=True)
    assert torch.equal(out.rename(None), direct)
    m.set_schema("tags", offsets="tag_offsets")
    routed = Inputs(schema={"tags": m})({"tags": ids.to(dev), "tag_offsets": offsets.to(dev)})["tags"]
    assert routed.names == ("B", "N", "E") and torch.equal(routed.rename(None), out.rename(None))

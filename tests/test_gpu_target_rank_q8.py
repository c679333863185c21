"""functional.target_ranks_q8 / QuantizedEmbeddingPairScorer.rank (csrc/target_rank.hip, Q8 targets) against the int64 /
fp64 count of tests/target_rank_ref.py over the rows c * scale + bias, and against topk_scores_q8; the exact cases and the
bound of the real-valued ones are those of tests/test_gpu_topk_q8.py."""
import numpy as np
import pytest
import torch

import q8_ref
from target_rank_ref import target_rank_ref
from test_gpu_target_rank import assert_exact, dtype_sim
from test_gpu_topk_q8 import B, DTYPES, _F, dev, int_case  # noqa: F401 (dev: the fixture)
from topk_ref import gamma

gpu = pytest.mark.gpu


def real_case(dtype, E, Vt=1000):      # anchors, Q8 rows of a quantized randn table, its codes / scale / bias in fp64
    g = torch.Generator().manual_seed(11)
    a = torch.randn(B, E, generator=g).to(dtype).float()
    qn = q8_ref.quantize(torch.randn(Vt, E, generator=g).numpy())
    scale, bias = (torch.from_numpy(t.astype(np.float64)) for t in q8_ref.tails(qn, E))
    return a, torch.from_numpy(qn), torch.from_numpy(qn[:, :E].astype(np.float64)), scale, bias


def labels(Vt, P, seed=0):             # (B, P), a padding label in every fifth sample
    y = torch.randint(0, Vt, (B, P), generator=torch.Generator().manual_seed(seed + Vt + P))
    y[::5, P - 1] = -1
    return y


def run(dev, a, q, E, y, dtype, exclude=None, **kw):
    r, s = _F().target_ranks_q8(a.to(dev, dtype), None, q.to(dev), E, y.to(dev), exclude=exclude, **kw)
    assert r.dtype == torch.int64 and s.dtype == torch.float32 and tuple(r.shape) == tuple(s.shape) == (B, y.shape[1])
    return r.cpu(), s.cpu()


@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("Vt", [127, 129, 1000, 5003])
@pytest.mark.parametrize("E", ["vec", 56, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_exact_with_ties(dev, dtype, E, Vt, P):
    E = (8 if dtype == torch.bfloat16 else 4) if E == "vec" else E      # E = 56: codes and the tail share a Q8 vector
    (a, q, x), y = int_case(Vt, E), labels(Vt, P)
    got = run(dev, a, q, E, y, dtype)
    assert_exact(got, target_rank_ref(a, x, y))
    assert got[0][0, P - 1] == -1 and got[1][0, P - 1] == float("-inf")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_widest_rows_and_most_labels(dev, dtype):
    """E = 256: the small arrangements and 17 Q8 vectors per row; P = 16: the thresholds kept in LDS"""
    (a, q, x), y = int_case(300, 256), labels(300, 16)
    assert_exact(run(dev, a, q, 256, y, dtype), target_rank_ref(a, x, y))


@gpu
@dtype_sim[0]
@dtype_sim[1]
@pytest.mark.parametrize("excl", [False, True])
def test_agrees_with_topk_scores_q8(dev, dtype, sim, excl):
    F_ = _F()
    a, q = (t.to(dev) for t in real_case(dtype, 64)[:2])
    a = a.to(dtype)
    ex = F_.topk_scores_q8(a, None, q, 64, 4, sim=sim)[1] if excl else None      # the four best are taken out
    v, i = F_.topk_scores_q8(a, None, q, 64, 128, sim=sim, exclude=ex)
    far = torch.tensor([min(set(range(200)) - set(row)) for row in (i if ex is None else torch.cat([i, ex], 1)).tolist()])
    y = torch.stack([i[:, 5], i[:, 100], far.to(dev), i[:, 0]], dim=1)
    r, s = F_.target_ranks_q8(a, None, q, 64, y, sim=sim, exclude=ex)
    assert r[:, [0, 1, 3]].tolist() == [[5, 100, 0]] * B and bool((r[:, 2] >= 128).all())
    assert torch.equal(s[:, [0, 1, 3]], v[:, [5, 100, 0]])


@gpu
@dtype_sim[0]
@dtype_sim[1]
def test_same_bits_in_both_kernels(dev, dtype, sim):
    """Sample b's best row by far (the quantized 2 a_b) stands at five ids, the same Q8 bytes, the label the (b % 5)-th of
    them: the rank is exactly b % 5 only if the list kernel and the streaming kernel give the pair the same bits."""
    a, q, _, _, _ = real_case(dtype, 64)
    q = q.clone()
    spots = torch.randperm(1000, generator=torch.Generator().manual_seed(4))[:5 * B].reshape(B, 5).sort(dim=1)[0]
    q[spots.reshape(-1)] = torch.from_numpy(q8_ref.quantize((2 * a).numpy())).repeat_interleave(5, dim=0)
    want = torch.arange(B) % 5
    y = spots.gather(1, want[:, None])
    x = torch.from_numpy(q8_ref.dequant(q.numpy(), 64))
    assert bool((target_rank_ref(a, x, y, sim)[1] <= 4).all())      # in fp64: nothing but the copies is near the label
    assert torch.equal(run(dev, a, q, 64, y, dtype, sim=sim)[0], want[:, None])


@gpu
@dtype_sim[0]
@dtype_sim[1]
@pytest.mark.parametrize("E", [64, 40])
def test_real_valued(dev, dtype, sim, E):
    a, q, c, scale, bias = real_case(dtype, E)
    x = c * scale + bias      # fp64: the reference rows
    y = torch.randint(0, 1000, (B, 3), generator=torch.Generator().manual_seed(E))
    scores = target_rank_ref(a, x, y, sim)[0]
    bound = gamma(E + 4 if sim == "dot" else E + 20) * (a.double().abs() @ (c * scale + bias.abs()).T)
    if sim == "cosine":
        bound = bound / (a.double().norm(dim=1)[:, None] * x.norm(dim=1)[None, :])
    sl, bl = scores.gather(1, y)[:, :, None], bound.gather(1, y)[:, :, None]
    other = torch.arange(1000)[None, None, :] != y[:, :, None]
    lo = ((scores[:, None, :] > sl + bound[:, None, :] + bl) & other).sum(dim=2)
    hi = ((scores[:, None, :] >= sl - bound[:, None, :] - bl) & other).sum(dim=2)
    r, s = run(dev, a, q, E, y, dtype, sim=sim)
    print(f"max err / bound = {float(((s.double() - sl[:, :, 0]).abs() / bl[:, :, 0]).max()):.3f}, widest interval "
          f"{int((hi - lo).max())}")
    assert bool(((lo <= r) & (r <= hi)).all())
    assert bool(((s.double() - sl[:, :, 0]).abs() <= bl[:, :, 0]).all())


@gpu
def test_addressing_exclusion_and_index_flag(dev):
    """anchors through int32 ids + offset, targets inside the Q8 table; listed: labels, repeats, padding, ids past the range"""
    F_ = _F()
    E, lo, hi, off, Vt = 32, 150, 450, 3, 300
    _, q, x = int_case(900, E, seed=1)
    g = torch.Generator().manual_seed(3)
    table = torch.randint(-2, 3, (200, E), generator=g).float()
    idx, y = torch.randint(0, 190, (B,), generator=g), torch.randint(0, Vt, (B, 2), generator=g)
    rnd = torch.randint(0, Vt, (B, 20), generator=g)
    ex = torch.cat([y[:, 1:], y[:, :1], rnd, rnd[:, :10], torch.full((B, 4), -1), torch.full((B, 4), Vt + 7)], dim=1)
    ref = target_rank_ref(table[idx + off], x[lo:hi], y, exclude=ex)
    assert not torch.equal(ref[1], target_rank_ref(table[idx + off], x[lo:hi], y)[1])
    w, qd, exd = table.to(dev, torch.bfloat16), q.to(dev), ex.to(dev)
    F_.index_errors_seen()
    got = F_.target_ranks_q8(w, idx.to(dev, torch.int32), qd, E, y.to(dev, torch.int32), anchor_offset=off, target_lo=lo,
                             target_hi=hi, exclude=exd)
    assert_exact((got[0].cpu(), got[1].cpu()), ref)
    assert not F_.index_errors_seen()
    y[7, 1] = Vt      # one label past the range
    r, s = F_.target_ranks_q8(w, idx.to(dev), qd, E, y.to(dev), anchor_offset=off, target_lo=lo, target_hi=hi, exclude=exd)
    assert F_.index_errors_seen() and int(r[7, 1]) == -1 and float(s[7, 1]) == float("-inf")
    assert torch.equal(r[8:], got[0][8:]) and torch.equal(r[:, 0], got[0][:, 0])


@gpu
@pytest.mark.parametrize("shared", [False, True])
def test_module_equals_functional(dev, shared):
    from torecsys_amd.fused import EmbeddingPairScorer
    from torecsys_amd.quant import QuantizedEmbeddingPairScorer
    F_ = _F()
    torch.manual_seed(2)
    m = EmbeddingPairScorer(32, *((400, None) if shared else (100, 300)), similarity="cosine", target_offset=100 if shared else 0)
    qm = QuantizedEmbeddingPairScorer.from_float(m.to(dev))
    idx, y = torch.randint(0, 100, (B,), device=dev), torch.randint(-1, 300, (B, 5), device=dev)
    ex = torch.randint(-1, 300, (B, 4), device=dev)
    r, s = qm.rank(idx, y, exclude=ex)
    anchors = F_.gather_rows_q8(qm.qweight if shared else qm.anchor_qweight, 32, idx.view(-1, 1)).view(B, 32)
    rr, rs = F_.target_ranks_q8(anchors, None, qm.qweight, 32, y, target_lo=100 if shared else 0, sim="cosine", exclude=ex)
    assert torch.equal(r, rr) and torch.equal(s, rs) and tuple(r.shape) == (B, 5) and int(r.max()) < 300

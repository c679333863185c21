"""Mapped update with the identity map is the plain update.

F_.scatter_rows_update and F_.scatter_rows_update_mapped run the same bucket walk into the same row sink; the mapped one
only sends every finished row through ``row_map``.  With row_map = arange(V) the two must therefore agree bit for bit --
tables and every optimizer state tensor, rows nobody looked up included -- for every optimizer, for the step size by
value and on the device, and on the vector and the element walk.  One bucket index over (K, 1) ids whose rows receive 0,
1, 32, 33, 64, 65, 257 and 2049 lookups: both sides of LONG_ROW_ELEM (32) and LONG_ROW (64), a chunked hot row (>
LONG_CHUNK = 256) and a row the element walk splits over several waves (> ELEM_SPLIT = 2048), plus 24 single lookups:
V = 40 rows, K = 2525 lookups.  Two steps with different integer-valued gradients (scatter_ref.integer_case), so the
second step starts from non-zero state."""
import functools

import pytest
import torch

import scatter_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
LENGTHS = (0, 1, 32, 33, 64, 65, 257, 2049)
LR = 2.0 ** -6
BETAS = (0.875, 0.984375)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _buckets():
    fs, idx = R.bucket_ladder(LENGTHS, 1, seed=11, singles=24, spare=8)
    counts = torch.bincount(idx[:, 0], minlength=fs[0])
    assert fs[0] == 40 and idx.shape == (2525, 1)
    assert sorted(set(counts.tolist())) == sorted(set(LENGTHS))
    return fs, idx, counts


def _optimizer(kind, capturable):
    from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseAdam, FusedSparseSGD
    if kind == "sgd":
        return FusedSparseSGD(LR, capturable=capturable)
    if kind == "adagrad":
        return FusedSparseAdagrad(LR, eps=1e-10, capturable=capturable)
    return FusedSparseAdam(LR, betas=BETAS, eps=1e-8, capturable=capturable)


def _state(opt, table, kind, capturable):
    """every state tensor the optimizer keeps for ``table``, by name"""
    if kind == "sgd":
        return {}
    if kind == "adagrad":
        return {"sum": opt.state_for(table, table)}
    out = dict(zip(("exp_avg", "exp_avg_sq"), opt.state_for(table, table)))
    if capturable:
        out.update(zip(("step_dev", "step_size_dev"), opt.step_tensors(table, table)))
    return out


@pytest.mark.parametrize("capturable", [False, True], ids=["byvalue", "capturable"])
@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam"])
@pytest.mark.parametrize("dtype,E", [(F32, 16), (F32, 10), (BF16, 32)], ids=["f32-E16-vec", "f32-E10-elem", "bf16-E32-vec"])
def test_mapped_update_with_the_identity_map_is_the_plain_update(dev, dtype, E, kind, capturable):
    from torecsys_amd import functional as F_
    fs, idx, counts = _buckets()
    V, K = fs[0], idx.shape[0]
    F_.clear_caches()
    rb = F_.row_buckets(idx.int().to(dev), None, V)
    assert (rb.V, rb.BN, rb.N) == (V, K, 1)
    w0 = R.integer_case(fs, idx, E, 3)["w"].to(dev).to(dtype)
    A, B = w0.clone(), w0.clone()
    optA, optB = _optimizer(kind, capturable), _optimizer(kind, capturable)
    identity = torch.arange(V, dtype=torch.int32, device=dev)
    untouched = (counts == 0).to(dev)
    assert int(untouched.sum()) == 9           # the 0-lookup row of the ladder and the eight spare rows
    for step in (1, 2):
        G = R.integer_case(fs, idx, E, 20 + step)["ge"].reshape(K, E).to(dev).to(dtype)
        before = A.clone()
        F_.scatter_rows_update(rb, A, optA, g_rows=G, key=A)
        F_.scatter_rows_update_mapped(rb, B, optB, G, identity, key=B)
        assert torch.equal(A, B), f"step {step}: the tables differ"
        sa, sb = _state(optA, A, kind, capturable), _state(optB, B, kind, capturable)
        assert sa.keys() == sb.keys()
        for name in sa:
            assert torch.equal(sa[name], sb[name]), f"step {step}: {name} differs"
        # not vacuous: the step changed looked-up rows and nothing else
        assert torch.equal(A[untouched], w0[untouched])
        assert not torch.equal(A[~untouched], before[~untouched])
    if kind == "adam" and not capturable:
        assert optA._entry(A, A)["step"] == optB._entry(B, B)["step"] == 2
    if kind == "adam" and capturable:
        assert int(sa["step_dev"]) == 2
    torch.cuda.synchronize()
    assert not F_.index_errors_seen()

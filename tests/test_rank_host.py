"""Host-side checks of the pair-score / ranking-loss feature (no GPU): tests/rank_ref.py against the reference's own
outputs and gradients (tests/golden/rank.npz), argument validation of the new library entries (all refusals happen before
any launch), the pure path function, reduction parsing, and the negative sampler's pairing."""
import ctypes
from functools import partial

import pytest
import torch
import torch.nn.functional as F

from rank_ref import (LOSS_CASES, RANK_SHAPES, fixture_reduction, loss_cases, pair_scores_ref, rank_loss_ref, shape_tag)

TOL = 1e-6
OK, EINVAL, EDTYPE = 0, -1, -2


def _err(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def lib():
    from torecsys_amd import build, _abi
    build.build()
    return _abi.load()


# ------------------------------------------------------------------------------------------------ rank_ref vs the fixture
@pytest.mark.parametrize("shape", RANK_SHAPES, ids=shape_tag)
def test_ref_scores_match_the_fixture(golden, shape):
    G = golden("rank")
    B, K, E = shape
    tag = shape_tag(shape)
    # MatrixFactorizationModel: the block's rows as a (2B, E) table
    x = G(f"mf/{tag}/x").requires_grad_()
    ids = torch.arange(B) * 2
    y = pair_scores_ref(x.view(2 * B, E), ids, x.view(2 * B, E), (ids + 1).view(B, 1))
    assert _err(y, G(f"mf/{tag}/out")) <= TOL
    (y * G(f"mf/{tag}/gout")).sum().backward()
    assert _err(x.grad, G(f"mf/{tag}/gx")) <= TOL
    # StarSpaceModel: row n of context against row n of target
    n = B * (1 + K)
    for name, sim in (("ss_dot", "dot"), ("ss_cos", "cosine")):
        c, t = G(f"{name}/{tag}/context").requires_grad_(), G(f"{name}/{tag}/target").requires_grad_()
        y = pair_scores_ref(c.view(n, E), torch.arange(n), t.view(n, E), torch.arange(n).view(n, 1), sim=sim)
        assert _err(y, G(f"{name}/{tag}/out")) <= TOL
        (y * G(f"{name}/{tag}/gout")).sum().backward()
        assert _err(c.grad, G(f"{name}/{tag}/gcontext")) <= TOL and _err(t.grad, G(f"{name}/{tag}/gtarget")) <= TOL


@pytest.mark.parametrize("shape", RANK_SHAPES, ids=shape_tag)
def test_ref_losses_match_the_fixture(golden, shape):
    G = golden("rank")
    tag = shape_tag(shape)
    margins = G("loss/margins")
    for name, red in loss_cases():
        kind, mi, _ = LOSS_CASES[name]
        margin = float(margins[mi]) if mi is not None else 0.0
        for mname in ("nomask", "mask"):
            mask = G(f"loss/{tag}/mask") if mname == "mask" else None
            p, n = G(f"loss/{tag}/pos").requires_grad_(), G(f"loss/{tag}/neg").requires_grad_()
            val = rank_loss_ref(p, n, kind, margin, mask, fixture_reduction(name, red, mask is not None))
            val.backward()
            key = f"loss/{name}/{tag}/{mname}/{red}"
            assert _err(val, G(key + "/loss")) <= TOL, key
            assert _err(p.grad, G(key + "/gpos")) <= TOL and _err(n.grad, G(key + "/gneg")) <= TOL, key


def test_fixture_pins_the_tie_rule(golden):
    """where K >= 2 sample 1 has two equal maximal negatives (columns 0 and K - 1) and an active hinge: the reference gives
    the whole gradient to ONE of them -- the first"""
    G = golden("rank")
    for shape in RANK_SHAPES:
        B, K, E = shape
        if K < 2:
            continue
        tag = shape_tag(shape)
        neg = G(f"loss/{tag}/neg")
        assert neg[1, 0] == neg[1, K - 1] == neg[1].max()
        g = G(f"loss/adaptive/{tag}/nomask/sum/gneg")
        assert g[1, 0] == 1.0 and float(g[1, 1:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ argument validation
def _score_fwd(lib, **kw):
    p, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    a = dict(a_table=p, a_idx=p, t_table=p, t_idx=p, E=8, dtype=0, idx_dtype=0, B=4, K=3, sim=0, scores=p, out_dtype=0)
    a.update(kw)
    return lib.trs_embed_pair_score_fwd(a["a_table"], 10, a["a_idx"], 0, a["t_table"], 10, a["t_idx"], 0, a["E"],
                                        a["dtype"], a["idx_dtype"], a["B"], a["K"], a["sim"], a["scores"], a["out_dtype"],
                                        null, null)


def _score_bwd(lib, **kw):
    p, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    a = dict(a_table=p, t_idx=p, dtype=0, idx_dtype=0, B=4, K=3, sim=0, g=p, g_dtype=0, block=p)
    a.update(kw)
    return lib.trs_embed_pair_score_bwd(a["a_table"], 10, p, 0, p, 10, a["t_idx"], 0, 8, a["dtype"], a["idx_dtype"],
                                        a["B"], a["K"], a["sim"], a["g"], a["g_dtype"], a["block"], null, 0, null)


def test_pair_score_entries_validate_without_gpu(lib):
    from torecsys_amd import _abi
    null = ctypes.c_void_p(0)
    for entry, name in ((_score_fwd, "embed_pair_score_fwd"), (_score_bwd, "embed_pair_score_bwd")):
        assert entry(lib, a_table=null) == EINVAL and "NULL" in _abi.last_error()
        assert _abi.last_error().startswith(name + ":")
        assert entry(lib, t_idx=null) == EINVAL
        assert entry(lib, dtype=7) == EDTYPE and "dtype" in _abi.last_error()
        assert entry(lib, sim=2) == EINVAL and "sim" in _abi.last_error()
        assert entry(lib, sim=-1) == EINVAL
        assert entry(lib, idx_dtype=5) == EINVAL and "idx dtype" in _abi.last_error()
        assert entry(lib, K=-1) == EINVAL
        assert entry(lib, B=0) == OK
        assert entry(lib, B=0, a_table=null, t_idx=null) == OK       # an empty batch touches nothing
    assert _score_fwd(lib, scores=null) == EINVAL
    assert _score_fwd(lib, dtype=0, out_dtype=1) == EDTYPE           # fp32 tables do not narrow their scores
    assert _score_bwd(lib, g=null) == EINVAL and _score_bwd(lib, block=null) == EINVAL
    assert _score_bwd(lib, g_dtype=3) == EDTYPE


def _loss_fwd(lib, **kw):
    p, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    a = dict(pos=p, neg=p, dtype=0, B=4, K=3, kind=1, reduction=0, loss=p, ws=p, ws_bytes=1 << 20, ps=4, ns=4)
    a.update(kw)
    return lib.trs_rank_loss_fwd(a["pos"], a["ps"], a["neg"], a["ns"], a["dtype"], null, a["B"], a["K"], a["kind"], 1.0,
                                 a["reduction"], a["loss"], null, a["ws"], a["ws_bytes"], null)


def _loss_bwd(lib, **kw):
    p, null = ctypes.c_void_p(16), ctypes.c_void_p(0)
    a = dict(pos=p, neg=p, dtype=0, B=4, K=3, kind=1, reduction=0, gp=p, gn=p, mask=null, denom=null, ps=4, ns=4)
    a.update(kw)
    return lib.trs_rank_loss_bwd(a["pos"], a["ps"], a["neg"], a["ns"], a["dtype"], a["mask"], a["B"], a["K"], a["kind"],
                                 1.0, a["reduction"], null, a["denom"], a["gp"], 4, a["gn"], 4, null)


def test_rank_loss_entries_validate_without_gpu(lib):
    from torecsys_amd import _abi
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(16)
    assert lib.trs_rank_loss_workspace_bytes(1 << 20) >= 8
    for entry, name in ((_loss_fwd, "rank_loss_fwd"), (_loss_bwd, "rank_loss_bwd")):
        assert entry(lib, pos=null) == EINVAL and "NULL" in _abi.last_error()
        assert _abi.last_error().startswith(name + ":")
        assert entry(lib, neg=null) == EINVAL
        assert entry(lib, dtype=9) == EDTYPE
        assert entry(lib, kind=4) == EINVAL and "kind" in _abi.last_error()
        assert entry(lib, kind=-1) == EINVAL
        assert entry(lib, reduction=3) == EINVAL and "reduction" in _abi.last_error()
        assert entry(lib, K=0) == EINVAL
        assert entry(lib, ns=2) == EINVAL          # a row stride shorter than the row
        assert entry(lib, B=0) == OK
    assert _loss_fwd(lib, loss=null) == EINVAL
    assert _loss_fwd(lib, ws_bytes=4) == -6
    assert _loss_bwd(lib, gp=null) == EINVAL
    assert _loss_bwd(lib, mask=p, reduction=2) == EINVAL and "denominator" in _abi.last_error()


def test_pair_score_path_is_a_pure_function(lib):
    from torecsys_amd import functional as F_

    def expected(E, size):      # written out here: rows of 1, 2, 4 .. 64 whole 16-byte vectors
        b = E * size
        return 1 if b % 16 == 0 and (b // 16) in (1, 2, 4, 8, 16, 32, 64) else 0

    for E in (1, 2, 4, 8, 10, 12, 16, 24, 32, 48, 64, 100, 128, 256, 512, 1024):
        assert F_.pair_score_path(E, torch.float32) == expected(E, 4), E
        assert F_.pair_score_path(E, torch.bfloat16) == expected(E, 2), E
    assert F_.pair_score_path(8, torch.float16) == -1
    assert lib.trs_pair_score_path(0, 0) == -1 and lib.trs_pair_score_path(8, 5) == -1
    assert lib.trs_pair_score_bwd_workspace_bytes(100, 3, 64, 1) == 0
    assert lib.trs_pair_score_bwd_workspace_bytes(100, 3, 10, 0) == 100 * 4 * 8


# ------------------------------------------------------------------------------------------------ host mirror without a device
def test_reduction_parsing():
    from torecsys_amd import functional as F_, losses as Ls
    assert F_.rank_reduction_code("sum") == F_.rank_reduction_code(torch.sum) == 0
    assert F_.rank_reduction_code("mean") == F_.rank_reduction_code(torch.mean) == 1
    assert F_.rank_reduction_code("sample") == 2
    for bad in ("max", torch.max, None, 3, True):
        with pytest.raises(ValueError):
            F_.rank_reduction_code(bad)
    assert Ls.BayesianPersonalizedRankingLoss().reduction == "sum"
    assert Ls.HingeLoss().reduction == "sum" and Ls.HingeLoss(0.5, torch.mean).reduction == "mean"
    assert Ls.AdaptiveHingeLoss(reduction="mean").reduction == "mean"
    with pytest.raises(AssertionError):
        Ls.HingeLoss(reduction="nope")
    with pytest.raises(NotImplementedError):
        Ls.BayesianPersonalizedRankingLoss(reduction=torch.max)
    with pytest.raises(TypeError):
        Ls.AdaptiveHingeLoss(reduction=3)
    with pytest.raises(ValueError):
        Ls.TripletLoss(reduction="none")
    with pytest.raises(ValueError):
        F_.rank_loss(torch.zeros(2, 3), None, "nope")
    with pytest.raises(RuntimeError, match="no CPU path"):
        Ls.HingeLoss()(torch.zeros(2, 1), torch.zeros(2, 3))


def test_layers_keep_the_reference_interface():
    from torecsys_amd import layers as L
    gmf = L.GeneralizedMatrixFactorizationLayer()
    assert gmf.inputs_size == {'inputs': ('B', '2', 'E',)} and gmf.outputs_size == {'outputs': ('B', '1',)}
    ss = L.StarSpaceLayer(partial(L.inner_product_similarity, dim=2))
    assert ss.inputs_size == {'inputs': ('B', '2', 'E',)} and ss.outputs_size == {'outputs': ('B', 'E',)}
    assert ss._fused == "dot"
    assert L.StarSpaceLayer(partial(F.cosine_similarity, dim=2))._fused == "cosine"
    assert L.StarSpaceLayer(partial(F.cosine_similarity, dim=2, eps=1e-6))._fused is None
    assert L.StarSpaceLayer(partial(F.cosine_similarity, dim=1))._fused is None
    assert L.StarSpaceLayer(F.pairwise_distance)._fused is None
    # any other callable is simply called on the two (B, 1, E) views, off the device too
    x = torch.randn(3, 2, 4)
    y = L.StarSpaceLayer(F.pairwise_distance)(x)
    assert y.names == ('B', 'O') and torch.equal(y.rename(None), F.pairwise_distance(x[:, 0:1], x[:, 1:2]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        gmf(x)


@pytest.mark.parametrize("shape", RANK_SHAPES, ids=shape_tag)
def test_in_batch_negatives_pairs_like_the_reference_miner(golden, shape):
    from harness.emb_models import in_batch_negatives
    G = golden("rank")
    B, K, E = shape
    tag = shape_tag(shape)
    anchor, target = G(f"miner/{tag}/anchor"), G(f"miner/{tag}/target")
    pos, neg = G(f"miner/{tag}/pos"), G(f"miner/{tag}/neg")          # (B, 2) and (B K, 2): [anchor id, target id]
    ids = in_batch_negatives(target, K, torch.Generator().manual_seed(int(G(f"miner/{tag}/seed"))))
    assert tuple(ids.shape) == (B, 1 + K) and ids.dtype == target.dtype
    assert torch.equal(ids[:, 0], pos[:, 1]) and torch.equal(anchor, pos[:, 0])
    # negative b K + k belongs to anchor b
    assert torch.equal(neg[:, 0], anchor.repeat_interleave(K))
    assert torch.equal(ids[:, 1:].reshape(-1), neg[:, 1])

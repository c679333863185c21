"""fp64 reference of topk_scores / target_ranks with ``interests=G``: the scores of tests/topk_ref.py per (interest,
target), their max over a user's G interests, then the same stable sort and the same plain count; and what the two test
files share.  U = 37: the last anchor tile is ragged at every group width."""
from functools import lru_cache

import pytest
import torch

from topk_ref import gamma, topk_ref

U = 37
dtypes = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def same(got, ref):
    return torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@lru_cache(maxsize=None)
def int_tables(G, Vt, E, seed=0):
    """(U G, E) anchors and (Vt, E) targets drawn from {-2 .. 2}: exact in bf16 and fp32, ties everywhere"""
    g = torch.Generator().manual_seed(seed * 7919 + Vt * 31 + E + 101 * G)
    return torch.randint(-2, 3, (U * G, E), generator=g).float(), torch.randint(-2, 3, (Vt, E), generator=g).float()


def multi_scores(anchors, targets, G, sim="dot"):
    """``anchors`` (U G, E) user-major -> (scores (U, Vt) fp64, bound (U, Vt) fp64): the error of a max is at most the
    largest of its operands' bounds, gamma(E) or gamma(E + 16) times sum |a_e t_e| (over the norms for cosine)"""
    a, t = anchors.double(), targets.double()
    bound = gamma(a.shape[1] + (16 if sim == "cosine" else 0)) * (a.abs() @ t.abs().T)
    if sim == "cosine":
        bound = bound / (a.norm(dim=1)[:, None] * t.norm(dim=1)[None, :])
    return topk_ref(anchors, targets, 1, sim)[0].view(-1, G, t.shape[0]).amax(1), bound.view(-1, G, t.shape[0]).amax(1)


def multi_topk_ref(anchors, targets, G, k, sim="dot", exclude=None):
    """(values (U, k) fp64, ids (U, k)), as topk_ref: excluded targets sort last and read -inf / -1"""
    key = -multi_scores(anchors, targets, G, sim)[0]
    for u, row in enumerate(exclude.tolist() if exclude is not None else []):
        key[u, [j for j in row if j >= 0]] = float("inf")
    key, ids = torch.sort(key, dim=1, stable=True)
    key, ids = key[:, :k], ids[:, :k].clone()
    ids[key == float("inf")] = -1
    return -key, ids


def multi_rank_ref(anchors, targets, G, labels, sim="dot", exclude=None):
    """(ranks (U, P) int64, label_scores (U, P) fp64), as target_rank_ref: a plain count per label"""
    scores, Vt = multi_scores(anchors, targets, G, sim)[0], targets.shape[0]
    ranks, ls = torch.full(labels.shape, -1), torch.full(labels.shape, float("-inf"), dtype=torch.float64)
    for u, row in enumerate(labels.tolist()):
        drop = {j for j in exclude[u].tolist() if 0 <= j < Vt} if exclude is not None else set()
        for p, l in enumerate(row):
            if 0 <= l < Vt:
                s = scores[u]
                front = (s > s[l]) | ((s == s[l]) & (torch.arange(Vt) < l))
                front[sorted(drop - {l})] = False
                ranks[u, p], ls[u, p] = int(front.sum()), s[l]
    return ranks, ls

#!/usr/bin/env python3
"""Golden vectors for the embedding models and the ranking losses, from the REAL reference (read-only, build container
only; the import recipe is make_golden.py's):

    python tests/golden/make_golden_rank.py            # rewrites tests/golden/rank.npz

  mf/<tag>/...            MatrixFactorizationModel on (B, 2, E): out, input gradient
  ss_dot|ss_cos/<tag>/... StarSpaceModel(E, K, partial(inner_product_similarity | F.cosine_similarity, dim=2)) on context /
                          target rows (B (1+K), 1, E): out, both input gradients
  loss/<name>/<tag>/<nomask|mask>/<sum|mean>/...   the five loss classes: loss, d/dpos, d/dneg
  miner/<tag>/...         UniformBatchMiner(K) on (B,) anchor / target ids after torch.manual_seed(seed)

<tag> = B_K_E.  The adaptive hinge is the reference's own ``hinge_loss(p, n.max(1, keepdim=True)[0], margin)`` reduced
by its ``apply_mask`` / reduction: the class itself broadcasts into a (B, B, 1) cross-sample matrix.
Asserted here, so the reference is well defined on every vector: no hinge argument is exactly 0 (clamp and
MarginRankingLoss differ there), every |p - n| < 20 (BPR finite), every mask keeps a sample, and where K >= 2 sample 1
has two equal maximal negatives (which pins the tie rule of the adaptive hinge).  Data only; no reference source is copied.
"""
import importlib
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, npy  # noqa: E402

SHAPES = [(5, 3, 8), (4, 1, 10), (6, 5, 64), (3, 4, 16)]
HINGE_MARGIN, ADAPTIVE_MARGIN, TRIPLET_MARGIN = 1.0, 0.7, 1.0


def leaf(t):
    return t.clone().requires_grad_()


def gen_models(models_emb, ops, out):
    for (B, K, E) in SHAPES:
        tag = f"{B}_{K}_{E}"
        g = torch.Generator().manual_seed(7000 + 31 * B + 7 * K + E)
        x = torch.randn(B, 2, E, generator=g)
        gout = torch.randn(B, 1, generator=g)
        xl = leaf(x)
        y = models_emb.MatrixFactorizationModel()(xl)
        (y * gout).sum().backward()
        out[f"mf/{tag}/x"], out[f"mf/{tag}/out"] = npy(x), npy(y)
        out[f"mf/{tag}/gout"], out[f"mf/{tag}/gx"] = npy(gout), npy(xl.grad)
        n = B * (1 + K)
        ctx_rows = torch.randn(n, 1, E, generator=g)
        tgt_rows = torch.randn(n, 1, E, generator=g)
        gout = torch.randn(n, 1, generator=g)
        for name, sim in (("ss_dot", partial(ops.inner_product_similarity, dim=2)),
                          ("ss_cos", partial(F.cosine_similarity, dim=2))):
            c, t = leaf(ctx_rows), leaf(tgt_rows)
            y = models_emb.StarSpaceModel(embed_size=E, num_neg=K, similarity=sim)(c, t)
            (y * gout).sum().backward()
            out[f"{name}/{tag}/context"], out[f"{name}/{tag}/target"] = npy(ctx_rows), npy(tgt_rows)
            out[f"{name}/{tag}/out"], out[f"{name}/{tag}/gout"] = npy(y), npy(gout)
            out[f"{name}/{tag}/gcontext"], out[f"{name}/{tag}/gtarget"] = npy(c.grad), npy(t.grad)


def gen_losses(ltr, fn, utils, out):
    def adaptive(margin, reduction):
        red = utils.get_reduction(reduction)

        def f(p, n, mask=None):
            loss = fn.hinge_loss(p, n.max(1, keepdim=True)[0], margin)
            return red(fn.apply_mask(loss, mask)) if mask is not None else red(loss)
        return f

    for (B, K, E) in SHAPES:
        tag = f"{B}_{K}_{E}"
        g = torch.Generator().manual_seed(9000 + 31 * B + 7 * K + E)
        pos = torch.randn(B, 1, generator=g) * 1.5
        neg = torch.randn(B, K, generator=g) * 1.5
        if K >= 2:      # two equal maximal negatives in sample 1, the hinge active there
            top = float(neg[1].max()) + 0.25
            neg[1, K - 1] = top
            neg[1, 0] = top
            pos[1, 0] = top - 0.1
        mask = torch.rand(B, generator=g) < 0.6
        mask[0] = True
        mask[B - 1] = False
        assert bool(mask.any()) and not bool(mask.all())
        assert float((pos - neg).abs().max()) < 20.0
        for m in (HINGE_MARGIN, ADAPTIVE_MARGIN, TRIPLET_MARGIN):
            assert float((m - pos + neg).abs().min()) > 1e-4, "a hinge argument is (nearly) 0"
        if K >= 2:
            assert int((neg[1] == neg[1].max()).sum()) == 2
            assert float(ADAPTIVE_MARGIN - pos[1, 0] + neg[1].max()) > 0
        out[f"loss/{tag}/pos"], out[f"loss/{tag}/neg"], out[f"loss/{tag}/mask"] = npy(pos), npy(neg), npy(mask)
        cases = []
        for red in ("sum", "mean"):
            cases += [("bpr", red, ltr.BayesianPersonalizedRankingLoss(reduction=red)),
                      ("hinge", red, ltr.HingeLoss(margin=HINGE_MARGIN, reduction=getattr(torch, red))),
                      ("adaptive", red, adaptive(ADAPTIVE_MARGIN, getattr(torch, red))),
                      ("triplet", red, ltr.TripletLoss(margin=TRIPLET_MARGIN, reduction=red)),
                      ("triplet0", red, ltr.TripletLoss(margin=0.0, reduction=red))]
        cases.append(("pointwise", "mean", ltr.PointwiseLogisticLoss()))
        for name, red, loss_fn in cases:
            for mname, mk in (("nomask", None), ("mask", mask)):
                p, n = leaf(pos), leaf(neg)
                val = loss_fn(p, n, mk) if mk is not None else loss_fn(p, n)
                assert val.dim() == 0 or val.numel() == 1, (name, tuple(val.shape))
                val.reshape(()).backward()
                key = f"loss/{name}/{tag}/{mname}/{red}"
                out[f"{key}/loss"] = npy(val.reshape(()))
                out[f"{key}/gpos"], out[f"{key}/gneg"] = npy(p.grad), npy(n.grad)
    out["loss/margins"] = np.array([HINGE_MARGIN, ADAPTIVE_MARGIN, TRIPLET_MARGIN], dtype=np.float64)


def gen_miner(miners, out):
    for (B, K, E) in SHAPES:
        tag = f"{B}_{K}_{E}"
        g = torch.Generator().manual_seed(500 + B + K)
        anchor = torch.randint(0, 50, (B,), generator=g)
        target = torch.randint(0, 50, (B,), generator=g)
        seed = 1234 + B
        torch.manual_seed(seed)
        pos, neg = miners.UniformBatchMiner(K)({"ids": anchor}, {"ids": target})
        out[f"miner/{tag}/anchor"], out[f"miner/{tag}/target"] = npy(anchor), npy(target)
        out[f"miner/{tag}/pos"], out[f"miner/{tag}/neg"] = npy(pos["ids"]), npy(neg["ids"])
        out[f"miner/{tag}/seed"] = np.array(seed, dtype=np.int64)


def main():
    import_reference()
    models_emb = importlib.import_module("torecsys.models.emb")
    ops = importlib.import_module("torecsys.utils.operations")
    utils = importlib.import_module("torecsys.utils")
    ltr = importlib.import_module("torecsys.losses.ltr")
    ltr_pair = importlib.import_module("torecsys.losses.ltr.pairwise_ranking_loss")
    ltr_point = importlib.import_module("torecsys.losses.ltr.pointwise_ranking_loss")
    fn = importlib.import_module("torecsys.losses.ltr.functional")
    miners = importlib.import_module("torecsys.miners")

    class L:
        BayesianPersonalizedRankingLoss = ltr_pair.BayesianPersonalizedRankingLoss
        HingeLoss = ltr_pair.HingeLoss
        TripletLoss = ltr_pair.TripletLoss
        PointwiseLogisticLoss = ltr_point.PointwiseLogisticLoss

    out = {}
    gen_models(models_emb, ops, out)
    gen_losses(L, fn, utils, out)
    gen_miner(miners, out)
    path = os.path.join(HERE, "rank.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

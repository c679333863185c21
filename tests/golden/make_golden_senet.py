"""Golden vectors for ComposeExcitationNetworkLayer (layers/ctr/compose_excitation_network.py) and the two models built on
it (FiBiNET, FAT-DeepFFM), captured from the REAL reference in the build container (same stub import recipe as
make_golden.py).  CPU fp32, fixed seeds, dropout 0.
Run:  python tests/golden/make_golden_senet.py    (needs the reference checkout; writes tests/golden/senet.npz)

Inputs are 0.5 * randn(B, M, E) + randn(B, M, 1): the per-field offset makes the pooled means differ between samples, so
gates and hidden units are live for some samples and dead for others.  Every case is asserted to have a live-gate share in
[0.2, 0.8], a gate unit and a hidden unit that are live for some samples and dead for others, and no pre-activation
within 1e-4 of zero (no ReLU decision inside float noise).  A seed that misses a condition is changed, not the condition.
Fixtures hold data only (arrays and name lists)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference, npy, save  # noqa: E402
from senet_ref import (FAT_ARGS, FIBINET_ARGS, FIBINET_TYPES, MODEL_BATCH, PARAM_KEYS, SENET_SHAPES, fields, make_x,  # noqa: E402
                       pre_activations, shape_tag)

SEED_BUMP = {}          # shape tag -> added to the seed 7000 + B + N + E when that seed misses a condition below


def check_case(tag, x, params):
    _, u, v = pre_activations(x, *params)
    live = float((v > 0).float().mean())
    assert 0.2 <= live <= 0.8, (tag, "live gate share", live)
    mixed_gate = ((v > 0).any(0) & (v <= 0).any(0)).any()
    mixed_hidden = ((u > 0).any(0) & (u <= 0).any(0)).any()
    assert bool(mixed_gate) and bool(mixed_hidden), (tag, "no unit is live for some samples and dead for others")
    margin = min(float(u.abs().min()), float(v.abs().min()))
    assert margin >= 1e-4, (tag, "pre-activation within float noise of the kink", margin)
    return live, margin


def gen_layers(layers_mod, out):
    for s in SENET_SHAPES:
        B, N, E, r, squared = s
        tag = shape_tag(s)
        seed = 7000 + B + N + E + SEED_BUMP.get(tag, 0)
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(seed)
        m = layers_mod.SENETLayer(N, r, squared=squared)
        M = fields(N, squared)
        x = make_x(g, B, M, E).requires_grad_()
        gout = torch.randn(B, M, E, generator=g)
        y = m(x)
        (y.rename(None) * gout).sum().backward()
        sd = m.state_dict()
        live, margin = check_case(tag, x.detach(), [sd[k] for k in PARAM_KEYS])
        print(f"{tag}: seed {seed}, live gates {live:.2f}, smallest |pre-activation| {margin:.2e}")
        out[f"{tag}/x"] = npy(x)
        out[f"{tag}/gout"] = npy(gout)
        out[f"{tag}/out"] = npy(y)
        out[f"{tag}/names"] = np.array(list(y.names))
        out[f"{tag}/gx"] = npy(x.grad)
        out[f"{tag}/keys"] = np.array(list(sd.keys()))
        for k, p in m.named_parameters():
            out[f"{tag}/param/{k}"] = npy(p)
            out[f"{tag}/grad/{k}"] = npy(p.grad)


def gen_model(out, name, build, shape, senet_prefix, seed):
    """the first seed >= ``seed`` whose case meets the conditions of check_case (the search is part of the recipe)"""
    while True:
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(seed)
        model = build()
        x = make_x(g, *shape).requires_grad_()
        sd = model.state_dict()
        try:
            check_case(name, x.detach(), [sd[f"{senet_prefix}.{k}"] for k in PARAM_KEYS])
            break
        except AssertionError:
            seed += 1
    y = model(x)
    y.rename(None).sum().backward()
    out[f"model/{name}/x"] = npy(x)
    out[f"model/{name}/out"] = npy(y)
    out[f"model/{name}/gx"] = npy(x.grad)
    out[f"model/{name}/keys"] = np.array(list(sd.keys()))
    for k, p in sd.items():
        out[f"model/{name}/param/{k}"] = npy(p)
    print(f"model/{name}: seed {seed}, out {tuple(y.shape)}")


def gen_models(models_mod, out):
    ctr = models_mod.ctr
    for kind in FIBINET_TYPES:
        gen_model(out, f"fibinet_{kind}",
                  lambda: ctr.FeatureImportanceAndBilinearFeatureInteractionNetwork(bilinear_type=kind, **FIBINET_ARGS),
                  (MODEL_BATCH, FIBINET_ARGS["num_fields"], FIBINET_ARGS["embed_size"]), "senet", 7100)
    gen_model(out, "fat_deep_ffm", lambda: ctr.FieldAttentiveDeepFieldAwareFactorizationMachineModel(**FAT_ARGS),
              (MODEL_BATCH, FAT_ARGS["num_fields"] ** 2, FAT_ARGS["embed_size"]), "cen", 7200)


def main():
    _, layers_mod, models_mod = import_reference()
    d = {}
    gen_layers(layers_mod, d)
    gen_models(models_mod, d)
    save("senet.npz", d)


if __name__ == "__main__":
    main()

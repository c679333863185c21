"""Golden vectors for MixtureOfExpertsLayer (layers/ctr/mixture_of_experts.py) and the two models built on it (MMoE,
DeepMoE), captured from the REAL reference in the build container (same stub import recipe as make_golden.py).  CPU fp32,
fixed seeds, dropout off.
Run:  python tests/golden/make_golden_moe.py    (needs the reference checkout; writes tests/golden/moe.npz)

Every case is asserted to have no ReLU pre-activation (experts; in the models also the towers) within 1e-4 of zero, so that
no ReLU decision lies inside float noise: the first seed >= the case's starting seed that meets it is taken (the search
is part of the recipe).  Fixtures hold data only (arrays and name lists)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference, npy, save  # noqa: E402
from moe_ref import (DEEPMOE_ARGS, KINK_MARGIN, MMOE_ARGS, MODEL_BATCH, MOE_SHAPES, deep_moe, kink_margin, layer_kwargs,  # noqa: E402
                     mmoe, moe_layer, shape_tag)


def first_good_seed(seed, build, shape, restate):
    """(seed, module, input) of the first seed >= ``seed`` whose pre-activations all keep KINK_MARGIN from zero"""
    while True:
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(seed)
        m = build()
        x = torch.randn(*shape, generator=g)
        pre = []
        restate(x, {k: v.detach() for k, v in m.state_dict().items()}, pre=pre)
        if kink_margin(pre) >= KINK_MARGIN:
            return seed, m, x, g, kink_margin(pre)
        seed += 1


def gen_layers(layers_mod, out):
    for s in MOE_SHAPES:
        B, N, E, X, Oi, G, hidden = s
        tag = shape_tag(s)
        seed, m, x, g, margin = first_good_seed(9000 + B + N + E + X + G, lambda: layers_mod.MOELayer(
            expert_func=layers_mod.DNNLayer, **layer_kwargs(s)), (B, N, E), moe_layer)
        gout = torch.randn(B, G, X * Oi, generator=g)
        xin = x.clone().requires_grad_()          # the reference renames its argument in place: hand it a tensor of its own
        y = m(xin)
        (y.rename(None) * gout).sum().backward()
        sd = m.state_dict()
        print(f"{tag}: seed {seed}, smallest |pre-activation| {margin:.2e}, out {tuple(y.shape)} {y.names}")
        out[f"{tag}/x"] = npy(x)
        out[f"{tag}/gout"] = npy(gout)
        out[f"{tag}/out"] = npy(y)
        out[f"{tag}/names"] = np.array(list(y.names))
        out[f"{tag}/gx"] = npy(xin.grad).reshape(B, N, E)
        out[f"{tag}/keys"] = np.array(list(sd.keys()))
        for k, p in m.named_parameters():
            out[f"{tag}/param/{k}"] = npy(p)
            out[f"{tag}/grad/{k}"] = npy(p.grad)


def gen_model(out, name, build, shape, restate, seed):
    seed, model, x, g, margin = first_good_seed(seed, build, shape, restate)
    xin = x.clone().requires_grad_()
    sd = model.state_dict()
    y = model(xin)
    assert not y.has_names() and tuple(y.shape) == (shape[0], 1), (name, y.shape, y.names)
    y.sum().backward()
    out[f"model/{name}/x"] = npy(x)
    out[f"model/{name}/out"] = npy(y)
    out[f"model/{name}/gx"] = npy(xin.grad).reshape(shape)
    out[f"model/{name}/keys"] = np.array(list(sd.keys()))
    for k, p in sd.items():
        out[f"model/{name}/param/{k}"] = npy(p)
    print(f"model/{name}: seed {seed}, smallest |pre-activation| {margin:.2e}, out {tuple(y.shape)}")


def gen_models(models_mod, out):
    ctr = models_mod.ctr
    gen_model(out, "mmoe", lambda: ctr.MultiGateMixtureOfExpertsModel(**MMOE_ARGS),
              (MODEL_BATCH, MMOE_ARGS["num_fields"], MMOE_ARGS["embed_size"]), mmoe, 9100)
    gen_model(out, "deep_moe", lambda: ctr.DeepMixtureOfExpertsModel(**DEEPMOE_ARGS),
              (MODEL_BATCH, DEEPMOE_ARGS["num_fields"], DEEPMOE_ARGS["embed_size"]), deep_moe, 9200)


def main():
    _, layers_mod, models_mod = import_reference()
    d = {}
    gen_layers(layers_mod, d)
    gen_models(models_mod, d)
    save("moe.npz", d)


if __name__ == "__main__":
    main()

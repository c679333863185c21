"""Golden vectors for DynamicRoutingLayer (layers/ctr/dynamic_routing.py), captured from the REAL reference in the build
container (same stub import recipe as make_golden.py).  CPU fp32, fixed seeds.
Run:  python tests/golden/make_golden_dynamic_routing.py    (needs the reference checkout; writes
tests/golden/dynamic_routing.npz)

The layer draws its coupling noise with ``randn_like`` inside ``forward``.  To record it, the generator state is saved
before the call and restored after it, and ``torch.randn`` of the noise shape is drawn from the restored state: on the
CPU that is the same stream of values.  Fixtures hold data only (arrays and name lists)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference, npy, save  # noqa: E402
from dynamic_routing_ref import ROUTING_SHAPES, X_SCALE, num_caps, shape_tag  # noqa: E402


def gen(layers_mod, out):
    for s in ROUTING_SHAPES:
        B, N, E, R, caps, iters = s
        tag = shape_tag(s)
        g = torch.Generator().manual_seed(9700 + B + 3 * N + 5 * E + 7 * R + caps + iters)
        torch.manual_seed(9800 + B + N + E + R)
        m = layers_mod.DynamicRoutingLayer(embed_size=E, routed_size=R, max_num_caps=caps, num_iter=iters)
        x = X_SCALE * torch.randn(B, N, E, generator=g)
        xin = x.clone().requires_grad_()          # the reference renames its argument in place: a tensor of its own
        state = torch.get_rng_state()
        y = m(xin)
        torch.set_rng_state(state)
        K = m.num_caps
        assert K == num_caps(N, caps) and tuple(y.shape) == (B, K, R), (tag, K, y.shape)
        noise = torch.randn(B, K, N, R)
        gout = torch.randn(B, K, R, generator=g)
        (y.rename(None) * gout).sum().backward()
        print(f"{tag}: K' = {K}, out {tuple(y.shape)} {y.names}")
        out[f"{tag}/x"] = npy(x)
        out[f"{tag}/S"] = npy(m.S)
        out[f"{tag}/noise"] = npy(noise)
        out[f"{tag}/out"] = npy(y)
        out[f"{tag}/names"] = np.array(list(y.names))
        out[f"{tag}/gout"] = npy(gout)
        out[f"{tag}/gx"] = npy(xin.grad).reshape(B, N, E)
        out[f"{tag}/gS"] = npy(m.S.grad)
        out[f"{tag}/keys"] = np.array(list(m.state_dict().keys()))
        out[f"{tag}/num_caps"] = np.array([K], dtype=np.int64)


def main():
    _, layers_mod, _ = import_reference()
    d = {}
    gen(layers_mod, d)
    save("dynamic_routing.npz", d)


if __name__ == "__main__":
    main()

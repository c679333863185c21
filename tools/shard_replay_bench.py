#!/usr/bin/env python3
"""One-rank row-sharded DeepFM step with a capturable fused optimizer on the owner (developer tool): the same step
launched from Python and replayed from a hipGraph (graph.GraphedStep), ms per step of each.
    python tools/shard_replay_bench.py [--rows 125000000] [--optimizer adagrad|adam] [--steps 50]
The step is forward + loss + backward with the table rows updated inside the backward; the dense parameters receive
gradients and no optimizer step (bench.py's workload and index ring, BASELINE shape)."""
import argparse
import os
import socket
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from harness import ctr_models as M  # noqa: E402
from torecsys_amd import optim  # noqa: E402
from torecsys_amd.dist import RowShardedMultiIndicesEmbedding  # noqa: E402
from torecsys_amd.fused import BCEWithLogitsLoss  # noqa: E402
from torecsys_amd.graph import GraphedStep  # noqa: E402
from torecsys_amd.inputs import Inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--optimizer", default="adagrad", choices=["adagrad", "adam"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=65536)
    a = ap.parse_args()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(s.getsockname()[1]))
    s.close()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    B, N, E, dt = a.batch, 39, 64, torch.bfloat16
    sizes = bench.field_sizes(a.rows, N)
    gen = torch.Generator().manual_seed(1234)
    ring = [(bench.synth_indices(B, sizes, gen, False).to(dev), (torch.rand(B, 1, generator=gen) < 0.25).float().to(dev))
            for _ in range(4)]
    torch.manual_seed(7)
    emb = RowShardedMultiIndicesEmbedding(embed_size=E, field_sizes=sizes, fuse_fm=True, dtype=dt, device=dev)
    feat = RowShardedMultiIndicesEmbedding(embed_size=1, field_sizes=sizes, dtype=dt, device=dev)
    emb.set_schema(["c0"])
    feat.set_schema(["c0"])
    fo = (optim.FusedSparseAdagrad(0.01, capturable=True) if a.optimizer == "adagrad"
          else optim.FusedSparseAdam(1e-3, capturable=True))
    emb.set_fused_optimizer(fo)
    feat.set_fused_optimizer(fo)
    inputs = Inputs(schema={"emb_inputs": emb, "feat_inputs": feat}).to(dev).to(dt)
    model = M.DeepFactorizationMachineModel(embed_size=E, num_fields=N, deep_layer_sizes=[400, 400, 400],
                                            fm_dropout_p=0.0).to(dev).to(dt)
    crit = BCEWithLogitsLoss()
    params = [p for p in model.parameters() if p.requires_grad]

    def fn(ix, lab):
        loss = crit(model(**inputs({"c0": ix})), lab)
        loss.backward()
        return loss

    def timed(run):
        for k in range(5):
            run(k)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for k in range(a.steps):
            run(k)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.steps

    def eager(k):
        for p in params:
            p.grad = None
        fn(*ring[k % 4])

    ms_eager = timed(eager)
    for p in params:
        p.grad = None
    step = GraphedStep(fn, ring[0], params=params, warmup=2)
    ms_replay = timed(lambda k: step(*ring[k % 4]))
    print(f"one-rank sharded DeepFM step, {a.rows} rows, B={B}, fused {a.optimizer} (capturable): "
          f"eager {ms_eager:.4f} ms/step, replayed {ms_replay:.4f} ms/step, loss {float(step.output):.6f}", flush=True)
    step.release_outputs()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

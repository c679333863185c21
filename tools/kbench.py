#!/usr/bin/env python3
"""Kernel micro-benchmarks (developer tool): time each C-ABI kernel at the BASELINE shape with HIP events
on the launch stream and print algorithmic GB/s.  python tools/kbench.py [--dtype bf16] [--what a,b]
--what bag [--L 50] [--pad 0.3] [--exclude-padding] [--weighted]: the bag-pooling kernels against their two ATen baselines
(own inputs, see bench_bag); the two switches add the masked / weighted kernels as further candidates of the same rounds.
--what attn [--L 50] [--H 1] [--pad 0.3]: attention pooling of ListIndicesEmbedding, the fused path against the same module
with the switch off, and the two kernels alone (own inputs, see bench_attn).
--what senet: the SENET / compose-excitation layer, both kernel families, against the ATen composition of the same module
(own inputs, see bench_senet).
--what compact [--shard-rows 125000000]: device-side row compaction against torch.unique, and the owner-side fused update
of a large shard through either (own inputs, see bench_compact).
--what moe: the gate part of MixtureOfExpertsLayer against the ATen composition of the same module, the two gate kernels
alone, and the experts' share of the whole layer (own inputs, see bench_moe).
--what routing [--L 50] [--R 64] [--caps 8] [--routing-iters 3]: DynamicRoutingLayer over lists of L behaviours, the fused
path against the same module with the switch off, the two kernels alone, the noise draw and the peak allocations (own
inputs, see bench_routing).
--what seq [--L 50] [--cell lstm|gru|rnn]: SequenceIndicesEmbedding(output_method='avg_pooling') over ordered lists of L ids
with lengths uniform in [1, L], the fused path against the same module with the switch off, and the two kernels alone (own
inputs, see bench_seq).
--what rank [--neg 10] [--sim dot|cosine]: pair scores + ranking loss of the embedding models, the fused path against the
same module with the switch off and against the reference-shaped composition, and the four kernels alone (own inputs, see
bench_rank).
--what prm [--L 30] [--H 4] [--layers 2]: the residual self-attention block and PersonalizedReRankingModel over it, fp32 and
bf16, the fused path against the same modules with the switch off, and the two kernels alone (own inputs, see bench_prm).
--what bagshard [--L 50] [--world 8]: the four kernels of the sharded bag pooling alone with this process as rank 0 of
--world, the world-1 module against the unsharded ListIndicesEmbedding, fp32 and bf16, and the wire bytes per rank of the
partial-sum path against the rows path (own inputs, see bench_bagshard).
--what ragged [--shape fixed,uniform,longtail] [--modes sum,mean,max]: ragged bag pooling (ids + offsets) against bag_pool on
the same bags padded to the longest and against F.embedding_bag with offsets (own inputs, see bench_ragged).
--what raggedattn [--shape fixed,uniform,longtail]: attention pooling of ragged bags (max_length 50, H = 1 and 4) against
ListIndicesEmbedding(use_attn=True) on the same bags padded to 50 and against the ATen composition with a key_padding_mask;
then the two ragged kernels alone (own inputs, see bench_raggedattn).
--what raggedfields [--fields 4] [--modes sum,mean,max]: RaggedMultiListIndicesEmbedding -- F ragged fields of one table in
one pass -- against F RaggedListIndicesEmbedding calls plus the cat, and against bag_pool_ragged on pre-offset ids plus the
permute to (B, F, E) (own inputs, see bench_raggedfields).
--what rowwise [--shard-rows N]: the fused optimizer step alone (the update walk) for SGD, Adagrad, row-wise Adagrad and
Adam through gather_rows and embed_fm, uniform and Zipf indices, on a bf16 table plain and with stochastic rounding; with
--shard-rows also the mapped owner update (own inputs, see bench_rowwise)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torecsys_amd import functional as F_  # noqa: E402


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in evs)
    return ts[len(ts) // 2] * 1e-3, ts[0] * 1e-3


def bench_bag(a):
    """Bag pooling (csrc/bag.hip) at (B, L, E, V): forward and forward+backward of sum / mean / max, alternating in this
    process with two baselines on the same inputs -- the reference's composition (F.embedding -> transpose -> adaptive
    pooling; the sum has no pooling module: block.sum(1)) and torch.nn.functional.embedding_bag without padding_idx.
    Every figure is the median of ``--rounds`` per-round medians with their min..max; the candidates take turns inside a
    round.  ``--exclude-padding`` adds bag_pool(exclude_padding=True) to the candidates of every mode, ``--weighted`` the
    weighted sum (per_sample_weights requiring grad, so its backward includes dw; with both switches also the two
    together) to those of the sum -- they alternate with the unmasked kernel in the same rounds, so its spread is the
    yardstick.  Then the row-bucket build on a batch with 60 % padding against one without."""
    import torch.nn.functional as TF
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    s = 2 if dt == torch.bfloat16 else 4
    dev = torch.device("cuda:0")
    B, L, E, V = a.B, a.L, a.E, a.V
    g = torch.Generator(device=dev).manual_seed(1234)

    def bags(pad):
        idx = torch.randint(1, V, (B, L), generator=g, device=dev)
        if pad > 0:      # trailing padding, mean padded share = pad
            keep = torch.rand(B, 1, generator=g, device=dev) * 2 * (1 - pad) * L
            idx = torch.where(torch.arange(L, device=dev).view(1, L) < keep, idx, torch.zeros_like(idx))
        return idx

    idx = bags(a.pad)
    w = torch.randn(V, E, generator=g, device=dev, dtype=dt).requires_grad_()
    gout = torch.randn(B, 1, E, generator=g, device=dev, dtype=dt)
    print(f"bag pooling B={B} L={L} E={E} V={V} {a.dtype} table {V * E * s / 2**30:.2f} GiB, padded share "
          f"{float((idx == 0).float().mean()):.2f}, {a.rounds} rounds x {a.iters} launches", flush=True)
    alg = B * L * (8 + E * s) + B * E * s

    def ours(mode, **kw):
        return lambda: F_.bag_pool(w, idx, mode, padding_idx=0, **kw)

    psw = (torch.rand(B, L, generator=g, device=dev) * 2).to(dt).requires_grad_() if a.weighted else None

    def comp(mode):
        def f():
            block = TF.embedding(idx, w, padding_idx=0)
            if mode == "sum":
                return block.sum(1, keepdim=True)
            pool = TF.adaptive_max_pool1d if mode == "max" else TF.adaptive_avg_pool1d
            return pool(block.transpose(1, 2), 1).transpose(1, 2)
        return f

    def bag(mode):
        return lambda: TF.embedding_bag(idx, w, mode=mode).unsqueeze(1)

    def fwd_bwd(f):
        def run():
            F_.clear_caches()          # the row buckets of the batch are rebuilt every step, as in training
            w.grad = None
            if psw is not None:
                psw.grad = None
            f().backward(gout)
        return run

    for mode in ("sum", "mean", "max"):
        cands = [("bag_pool (HIP)", ours(mode)), ("composition (ATen)", comp(mode)), ("embedding_bag (ATen)", bag(mode))]
        if a.exclude_padding:
            cands.insert(1, ("bag_pool masked (HIP)", ours(mode, exclude_padding=True)))
        if a.weighted and mode == "sum":
            cands.insert(1, ("bag_pool wgt (HIP)", ours(mode, per_sample_weights=psw)))
            if a.exclude_padding:
                cands.insert(1, ("masked + wgt (HIP)", ours(mode, exclude_padding=True, per_sample_weights=psw)))
        live = []
        for name, f in cands:
            try:
                f().backward(gout)
                w.grad = None
                torch.cuda.synchronize()
                live.append((name, f))
            except Exception as e:      # noqa: BLE001 -- a mode / dtype this torch build does not serve
                print(f"{mode:5s} {name:22s} not supported on this torch build ({type(e).__name__}: {str(e)[:80]}); "
                      f"the other baseline stands alone for this case", flush=True)
        res = {}
        for what in ("fwd", "fwd+bwd"):
            per = {name: [] for name, _ in live}
            for _ in range(a.rounds):
                for name, f in live:
                    if what == "fwd":
                        with torch.no_grad():
                            per[name].append(timeit(f, iters=a.iters, warm=2)[0])
                    else:
                        per[name].append(timeit(fwd_bwd(f), iters=a.iters, warm=2)[0])
            for name, ts in per.items():
                ts = sorted(ts)
                res[(what, name)] = (ts[len(ts) // 2], ts[0], ts[-1])
                extra = ""
                if what == "fwd":
                    extra = f"  {alg / ts[len(ts) // 2] / 8e12 * 100:5.1f}% of 8 TB/s on {alg / 1e6:.0f} MB (alg)"
                print(f"{mode:5s} {what:8s} {name:22s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. "
                      f"{ts[-1] * 1e6:9.1f} us{extra}", flush=True)
        w.grad = None
    # the bucket build: does a padding-heavy batch (60 % of all positions on row 0) cost more than one without?
    nopad, pad60 = bags(0.0), bags(0.6)

    def csr(ix, skip=None):
        def run():
            F_.clear_caches()
            return F_.row_buckets(ix, None, V, skip_row=skip)
        return run
    cases = [("no padding", csr(nopad)), ("60 % padding", csr(pad60)),
             ("no padding, padding id skipped", csr(nopad, 0)), ("60 % padding, padding id skipped", csr(pad60, 0))]
    per = {name: [] for name, _ in cases}
    for _ in range(a.rounds):
        for name, f in cases:
            per[name].append(timeit(f, iters=a.iters, warm=2)[0])
    for name, ts in per.items():
        ts = sorted(ts)
        print(f"csr_build (B, L) {name:34s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us",
              flush=True)


def bench_ragged(a):
    """Ragged bag pooling (csrc/bag_ragged.hip) at B bags, E, V: forward and forward+backward (row buckets rebuilt every
    step) of sum / mean / max, alternating in this process with bag_pool(exclude_padding=True) on the same bags padded with
    id 0 to the longest one, and with torch.nn.functional.embedding_bag(ids, w, offsets) on the device.  Bag lengths from a
    seeded generator: ``fixed`` 50; ``uniform`` 0..100; ``longtail`` most bags under 10 ids, 300 bags of 2000..6000.  Every
    figure is the median of ``--rounds`` per-round medians with their min..max; the candidates take turns inside a round.
    The forward's share of 8 TB/s is on its algorithmic bytes n * (8 + E*s) + (B + 1) * 8 read, B * E*s written."""
    import torch.nn.functional as TF
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    s = 2 if dt == torch.bfloat16 else 4
    dev = torch.device("cuda:0")
    B, E, V = a.B, a.E, a.V
    g = torch.Generator(device=dev).manual_seed(4321)
    w = torch.randn(V, E, generator=g, device=dev, dtype=dt).requires_grad_()
    gout = torch.randn(B, 1, E, generator=g, device=dev, dtype=dt)
    print(f"ragged bag pooling B={B} E={E} V={V} {a.dtype} table {V * E * s / 2**30:.2f} GiB, long-bag threshold "
          f"T={F_.bag_ragged_long_len()}, {a.rounds} rounds x {a.iters} launches", flush=True)

    def lengths_of(shape):
        if shape == "fixed":
            return torch.full((B,), 50, dtype=torch.int64, device=dev)
        if shape == "uniform":
            return torch.randint(0, 101, (B,), generator=g, device=dev)
        ln = torch.randint(0, 10, (B,), generator=g, device=dev)
        hot = torch.randperm(B, generator=g, device=dev)[:300]
        ln[hot] = torch.randint(2000, 6001, (300,), generator=g, device=dev)
        return ln

    for shape in a.shape.split(","):
        ln = lengths_of(shape)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), ln.cumsum(0)])
        n, lmax = int(offsets[-1]), int(ln.max())
        ids = torch.randint(1, V, (n,), generator=g, device=dev)
        alg = n * (8 + E * s) + (B + 1) * 8 + B * E * s
        print(f"{shape}: n={n} ids, longest bag {lmax}, padded form B*L_max={B * lmax} ids "
              f"({n / max(B * lmax, 1) * 100:.1f} % live)", flush=True)
        padded = None
        if B * lmax < 2 ** 31 - 1:
            col = torch.arange(lmax, device=dev).view(1, lmax)
            padded = torch.zeros(B, lmax, dtype=torch.int64, device=dev)
            padded[col < ln.view(B, 1)] = ids                      # row-major: the bags in order
        else:
            print(f"{shape}: padded form not run (B*L_max does not fit the bucket build's int32 positions)", flush=True)
        off_b = offsets[:-1].contiguous()

        def fwd_bwd(f):
            def run():
                F_.clear_caches()          # the row buckets of the batch are rebuilt every step, as in training
                w.grad = None
                f().backward(gout)
            return run

        for mode in a.modes.split(","):
            cands = [("bag_pool_ragged (HIP)", lambda: F_.bag_pool_ragged(w, ids, offsets, mode, 0, exclude_padding=True,
                                                                          include_last_offset=True))]
            if padded is not None:
                cands.append(("bag_pool padded (HIP)", lambda: F_.bag_pool(w, padded, mode, 0, exclude_padding=True)))
            cands.append(("embedding_bag (ATen)", lambda: TF.embedding_bag(ids, w, off_b, mode=mode).unsqueeze(1)))
            live = {"fwd": [], "fwd+bwd": []}      # probed separately: a missing backward does not drop the forward
            for name, f in cands:
                for what in ("fwd", "fwd+bwd"):
                    try:
                        if what == "fwd":
                            with torch.no_grad():
                                f()
                        else:
                            f().backward(gout)
                            w.grad = None
                        torch.cuda.synchronize()
                        live[what].append((name, f))
                    except Exception as e:      # noqa: BLE001 -- a mode / dtype this torch build does not serve
                        print(f"{shape:8s} {mode:5s} {what:8s} {name:22s} not run ({type(e).__name__}: {str(e)[:80]})",
                              flush=True)
            for what in ("fwd", "fwd+bwd"):
                per = {name: [] for name, _ in live[what]}
                for _ in range(a.rounds):
                    for name, f in live[what]:
                        if what == "fwd":
                            with torch.no_grad():
                                per[name].append(timeit(f, iters=a.iters, warm=2)[0])
                        else:
                            per[name].append(timeit(fwd_bwd(f), iters=a.iters, warm=2)[0])
                for name, ts in per.items():
                    ts = sorted(ts)
                    extra = ""
                    if what == "fwd" and name.startswith("bag_pool_ragged"):
                        extra = f"  {alg / ts[len(ts) // 2] / 8e12 * 100:5.1f}% of 8 TB/s on {alg / 1e6:.0f} MB (alg)"
                    print(f"{shape:8s} {mode:5s} {what:8s} {name:22s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread "
                          f"{ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us{extra}", flush=True)
            w.grad = None
        del padded, ids


def bench_raggedfields(a):
    """F multi-valued fields over one table of V rows in all (csrc/bag_fields.hip) at B samples, E: forward and
    forward+backward (maps and row buckets rebuilt every step, as in training) of RaggedMultiListIndicesEmbedding,
    alternating in this process with two baselines on the same bags:
      (a) F RaggedListIndicesEmbedding(include_last_offset=True) modules, one per field on a table of the field's size, their
          (B, 1, E) results joined by torch.cat -- what a model does without the new module;
      (b) ONE bag_pool_ragged over all F * B bags on ids that already carry their field's row offset, then the permute of
          the field-major (F, B, E) result to a contiguous (B, F, E) -- one pass, but the copy stays.
    (a) against the module shows the launches and the copy together, (b) against the module the copy alone.  Bag lengths
    per field are the ``longtail`` of --what ragged scaled to the field (most bags under 10 ids, 300 / F bags of
    2000..6000); field sizes are V / F each.  Every figure is the median of ``--rounds`` per-round medians with their
    min..max; the candidates take turns inside a round."""
    from torecsys_amd.inputs import RaggedListIndicesEmbedding, RaggedMultiListIndicesEmbedding
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    dev = torch.device("cuda:0")
    B, E, NF = a.B, a.E, a.fields
    size = a.V // NF
    g = torch.Generator(device=dev).manual_seed(9876)
    ln = torch.randint(0, 10, (NF, B), generator=g, device=dev)
    hot_n = max(1, 300 // NF)
    for f in range(NF):
        hot = torch.randperm(B, generator=g, device=dev)[:hot_n]
        ln[f, hot] = torch.randint(2000, 6001, (hot_n,), generator=g, device=dev)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), ln.reshape(-1).cumsum(0)])
    n = int(offsets[-1])
    values = torch.randint(0, size, (n,), generator=g, device=dev)
    gout = torch.randn(B, NF, E, generator=g, device=dev, dtype=dt)
    print(f"ragged fields F={NF} B={B} E={E} V={size * NF} ({size} rows per field) {a.dtype}: n={n} ids, longest bag "
          f"{int(ln.max())}, {a.rounds} rounds x {a.iters} launches", flush=True)
    for mode in a.modes.split(","):
        method = {"sum": "sum", "mean": "avg_pooling", "max": "max_pooling"}[mode]
        multi = RaggedMultiListIndicesEmbedding(E, [size] * NF, output_method=method).to(dev).to(dt)
        w = multi.embedding.weight
        singles, parts = [], []
        for f in range(NF):
            m = RaggedListIndicesEmbedding(embed_size=E, field_size=size, padding_idx=None, output_method=method,
                                           include_last_offset=True).to(dev).to(dt)
            with torch.no_grad():
                m.embedding.weight.copy_(w[f * size:(f + 1) * size])
            beg, end = int(offsets[f * B]), int(offsets[(f + 1) * B])
            singles.append(m)
            parts.append((values[beg:end].contiguous(), (offsets[f * B:(f + 1) * B + 1] - beg).contiguous()))
        field_of = torch.repeat_interleave(torch.arange(NF, device=dev), ln.sum(1))
        shifted = values + field_of * size                                    # ids with their field's row offset

        def one_pass():
            return multi(values, offsets).rename(None)

        def per_field():
            return torch.cat([m(v, o).rename(None) for m, (v, o) in zip(singles, parts)], dim=1)

        def pre_offset():
            y = F_.bag_pool_ragged(w, shifted, offsets, mode, include_last_offset=True)      # (F*B, 1, E), field-major
            return y.view(NF, B, E).permute(1, 0, 2).contiguous()

        with torch.no_grad():
            ref = one_pass()
            assert torch.equal(ref, per_field()) and torch.equal(ref, pre_offset()), "the candidates disagree"
        params = [w] + [m.embedding.weight for m in singles]

        def fwd_bwd(f):
            def run():
                F_.clear_caches()          # maps and row buckets are rebuilt every step, as in training
                for p in params:
                    p.grad = None
                f().backward(gout)
            return run

        cands = [("fields module (HIP, one pass)", one_pass), (f"(a) {NF} ragged modules + cat", per_field),
                 ("(b) pre-offset ids + permute", pre_offset)]
        res = {}
        for what in ("fwd", "fwd+bwd"):
            per = {name: [] for name, _ in cands}
            for _ in range(a.rounds):
                for name, f in cands:
                    if what == "fwd":
                        with torch.no_grad():
                            per[name].append(timeit(f, iters=a.iters, warm=2)[0])
                    else:
                        per[name].append(timeit(fwd_bwd(f), iters=a.iters, warm=2)[0])
            for name, ts in per.items():
                ts = sorted(ts)
                res[name] = ts[len(ts) // 2]
                print(f"F={NF:<3d} {mode:5s} {what:8s} {name:30s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread "
                      f"{ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us", flush=True)
            print(f"F={NF:<3d} {mode:5s} {what:8s} (a) / module = {res[cands[1][0]] / res[cands[0][0]]:.2f}x, "
                  f"(b) / module = {res[cands[2][0]] / res[cands[0][0]]:.2f}x", flush=True)
        for p in params:
            p.grad = None


def bench_attn(a):
    """Attention pooling (csrc/attn_pool.hip) at (B, L, E, H, V): forward and forward+backward of
    ListIndicesEmbedding(use_attn=True, output_method='avg_pooling'), the fused path against the SAME module with the switch
    off (inputs.ATTN_POOL = False: HIP gather + nn.MultiheadAttention + mean in ATen, the path before the kernel), taking
    turns inside every round; then the two new kernels alone.  Every figure is the median of ``--rounds`` per-round medians
    with their min..max, and the forward's peak allocation of either path is printed."""
    from torecsys_amd import inputs as I
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    s = 2 if dt == torch.bfloat16 else 4
    dev = torch.device("cuda:0")
    B, L, E, V, H = a.B, a.L, a.E, a.V, a.H
    g = torch.Generator(device=dev).manual_seed(1234)
    idx = torch.randint(1, V, (B, L), generator=g, device=dev)
    if a.pad > 0:
        keep = torch.rand(B, 1, generator=g, device=dev) * 2 * (1 - a.pad) * L
        idx = torch.where(torch.arange(L, device=dev).view(1, L) < keep, idx, torch.zeros_like(idx))
    m = I.ListIndicesEmbedding(embed_size=E, field_size=V, use_attn=True, num_heads=H, output_method="avg_pooling")
    with torch.no_grad():
        m.attention.in_proj_bias.normal_(0, 0.1)
    m = m.to(dev).to(dt)
    gout = torch.randn(B, 1, E, generator=g, device=dev, dtype=dt)
    alg = B * L * (8 + E * s) + B * E * s + B * H * E * s
    flops = B * (4 * L * E * E + 2 * L * L * E)
    print(f"attention pooling B={B} L={L} E={E} H={H} V={V} {a.dtype} path {F_.attn_pool_path(L, E, H, dt)}, padded share "
          f"{float((idx == 0).float().mean()):.2f}, {a.rounds} rounds x {a.iters} launches; forward: {alg / 1e6:.0f} MB (alg), "
          f"{flops / 1e9:.1f} GFLOP", flush=True)

    def module(fused):
        def f():
            I.ATTN_POOL = fused
            return m(idx).rename(None)
        return f

    def fwd_bwd(f):
        def run():
            F_.clear_caches()          # the row buckets of the batch are rebuilt every step, as in training
            for p in m.parameters():
                p.grad = None
            f().backward(gout)
        return run

    cands = [("attn_pool (HIP)", module(True)), ("composition (ATen)", module(False))]
    for name, f in cands:
        F_.clear_caches()
        with torch.no_grad():
            f()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = f()
        torch.cuda.synchronize()
        print(f"{name:22s} forward peak allocation {(torch.cuda.max_memory_allocated() - base) / 2**20:9.1f} MiB "
              f"((B, L, E) block: {B * L * E * s / 2**20:.1f} MiB)", flush=True)
        del y
    res = {}
    for what in ("fwd", "fwd+bwd"):
        per = {name: [] for name, _ in cands}
        for _ in range(a.rounds):
            for name, f in cands:
                if what == "fwd":
                    with torch.no_grad():
                        per[name].append(timeit(f, iters=a.iters, warm=2)[0])
                else:
                    per[name].append(timeit(fwd_bwd(f), iters=a.iters, warm=2)[0])
        for name, ts in per.items():
            ts = sorted(ts)
            res[(what, name)] = ts[len(ts) // 2]
            print(f"{what:8s} {name:22s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. "
                  f"{ts[-1] * 1e6:9.1f} us", flush=True)
        print(f"{what:8s} composition / attn_pool = "
              f"{res[(what, 'composition (ATen)')] / res[(what, 'attn_pool (HIP)')]:.2f}x", flush=True)
    I.ATTN_POOL = True
    # the two kernels alone (the backward without the bucket walk behind it)
    from torecsys_amd._abi import call, index_dtype_code, ptr, size_query, stream_ptr, value_dtype_code
    w = m.embedding.weight.detach()
    wqk, bqk = m.attention.in_proj_weight.detach()[:2 * E].contiguous(), m.attention.in_proj_bias.detach()[:2 * E].contiguous()
    code = value_dtype_code(w)
    xt = torch.empty(B, H, E, dtype=dt, device=dev)
    gx = torch.randn(B, H, E, generator=g, device=dev, dtype=dt)
    blocks = size_query("trs_attn_pool_blocks", B, L, E, H, code, 1)
    dx = torch.empty(B, L, E, dtype=dt, device=dev)
    dwp = torch.empty(blocks, 2 * E, E, dtype=torch.float32, device=dev)
    dbp = torch.empty(blocks, 2 * E, dtype=torch.float32, device=dev)
    ws_bytes = size_query("trs_attn_pool_bwd_workspace_bytes", blocks, L, E, H)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)

    def k_fwd():
        call("trs_attn_pool_fwd", ptr(w), V, E, code, ptr(idx), index_dtype_code(idx), B, L, ptr(wqk), ptr(bqk), H, 1,
             ptr(xt), None, stream_ptr())

    def k_bwd():
        call("trs_attn_pool_bwd", ptr(w), V, E, code, ptr(idx), index_dtype_code(idx), B, L, ptr(wqk), ptr(bqk), H, 1,
             ptr(gx), ptr(dx), ptr(dwp), ptr(dbp), blocks, ptr(ws), ws_bytes, None, stream_ptr())

    for name, f, fl in (("trs_attn_pool_fwd", k_fwd, flops), ("trs_attn_pool_bwd", k_bwd, 4 * flops)):
        ts = sorted(timeit(f, iters=a.iters, warm=2)[0] for _ in range(a.rounds))
        med = ts[len(ts) // 2]
        print(f"kernel   {name:22s} med {med * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us  "
              f"{fl / med / 1e12:6.1f} TFLOP/s ({blocks} workgroups in the backward)", flush=True)


def bench_raggedattn(a):
    """Attention pooling of ragged bags (the ragged kernels of csrc/attn_pool.hip) at B bags, E, V, H = 1 and 4,
    max_length = 50: forward and forward + backward (row buckets rebuilt every step) of
    RaggedListIndicesEmbedding(use_attn=True, output_method='avg_pooling'), taking turns inside every round with
    ListIndicesEmbedding(use_attn=True) on the same bags padded with id 0 to 50 (the path before the ragged kernels; it
    attends to the padding too) and with the ATen composition on the padded bags (embedding, nn.MultiheadAttention with a
    key_padding_mask, masked mean); then the two new kernels alone.  Bag lengths are those of --what ragged (``fixed`` 50,
    ``uniform`` 0..100, ``longtail`` most bags under 10 ids and 300 bags of 2000..6000), clipped to 50.  Every figure is the
    median of ``--rounds`` per-round medians with their min..max."""
    from torecsys_amd import inputs as I
    from torecsys_amd._abi import call, index_dtype_code, ptr, size_query, stream_ptr, value_dtype_code
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    dev = torch.device("cuda:0")
    B, E, V, ML = a.B, a.E, a.V, 50
    g = torch.Generator(device=dev).manual_seed(4321)
    gout = torch.randn(B, 1, E, generator=g, device=dev, dtype=dt)

    def lengths_of(shape):
        if shape == "fixed":
            return torch.full((B,), 50, dtype=torch.int64, device=dev)
        if shape == "uniform":
            return torch.randint(0, 101, (B,), generator=g, device=dev).clamp_(max=ML)
        ln = torch.randint(0, 10, (B,), generator=g, device=dev)
        hot = torch.randperm(B, generator=g, device=dev)[:300]
        ln[hot] = torch.randint(2000, 6001, (300,), generator=g, device=dev)
        return ln.clamp_(max=ML)

    for H in (1, 4):
        rag = I.RaggedListIndicesEmbedding(embed_size=E, field_size=V, use_attn=True, num_heads=H, max_length=ML,
                                           include_last_offset=True)
        with torch.no_grad():
            rag.attention.in_proj_bias.normal_(0, 0.1)
        rag = rag.to(dev).to(dt)
        pad = I.ListIndicesEmbedding(embed_size=E, field_size=V, use_attn=True, num_heads=H, output_method="avg_pooling")
        pad.load_state_dict(rag.state_dict())
        pad = pad.to(dev).to(dt)
        params = list(rag.parameters()) + list(pad.parameters())
        for shape in a.shape.split(","):
            ln = lengths_of(shape)
            offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), ln.cumsum(0)])
            n = int(offsets[-1])
            ids = torch.randint(1, V, (n,), generator=g, device=dev)
            col = torch.arange(ML, device=dev).view(1, ML)
            live = col < ln.view(B, 1)
            padded = torch.zeros(B, ML, dtype=torch.int64, device=dev)
            padded[live] = ids                                         # row-major: the bags in order
            mask = ~live
            mask[:, 0] = False                                         # an empty bag keeps one key: no NaN rows in ATen
            cnt = ln.clamp(min=1).view(B, 1).to(dt)
            flops = int((4 * ln * E * E + 2 * ln * ln * E).sum())
            print(f"ragged attention pooling B={B} E={E} H={H} V={V} {a.dtype} max_length={ML} {shape}: n={n} ids "
                  f"({n / (B * ML) * 100:.1f} % of the padded positions), forward {flops / 1e9:.1f} GFLOP against "
                  f"{B * (4 * ML * E * E + 2 * ML * ML * E) / 1e9:.1f} padded, {a.rounds} rounds x {a.iters} launches", flush=True)

            def aten():
                seq = torch.nn.functional.embedding(padded, pad.embedding.weight).transpose(0, 1)
                o, _ = pad.attention(seq, seq, seq, key_padding_mask=mask, need_weights=False)
                return ((o.transpose(0, 1) * live.unsqueeze(-1)).sum(dim=1, keepdim=True) / cnt.unsqueeze(-1)).to(dt)

            cands = [("ragged module (HIP)", lambda: rag(ids, offsets).rename(None)),
                     ("padded module (HIP)", lambda: pad(padded).rename(None)), ("composition (ATen)", aten)]

            def fwd_bwd(f):
                def run():
                    F_.clear_caches()          # the row buckets of the batch are rebuilt every step, as in training
                    for p in params:
                        p.grad = None
                    f().backward(gout)
                return run

            res = {}
            for what in ("fwd", "fwd+bwd"):
                per = {name: [] for name, _ in cands}
                for _ in range(a.rounds):
                    for name, f in cands:
                        if what == "fwd":
                            with torch.no_grad():
                                per[name].append(timeit(f, iters=a.iters, warm=2)[0])
                        else:
                            per[name].append(timeit(fwd_bwd(f), iters=a.iters, warm=2)[0])
                for name, ts in per.items():
                    ts = sorted(ts)
                    res[name] = ts[len(ts) // 2]
                    print(f"H={H} {shape:8s} {what:8s} {name:22s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread "
                          f"{ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us", flush=True)
                print(f"H={H} {shape:8s} {what:8s} padded / ragged = "
                      f"{res['padded module (HIP)'] / res['ragged module (HIP)']:.2f}x, composition / ragged = "
                      f"{res['composition (ATen)'] / res['ragged module (HIP)']:.2f}x", flush=True)
            # the two new kernels alone (the backward without the zero-fill and the bucket walk around it)
            w = rag.embedding.weight.detach()
            wqk = rag.attention.in_proj_weight.detach()[:2 * E].contiguous()
            bqk = rag.attention.in_proj_bias.detach()[:2 * E].contiguous()
            code = value_dtype_code(w)
            xt = torch.empty(B, H, E, dtype=dt, device=dev)
            cn = torch.empty(B, dtype=torch.float32, device=dev)
            gx = torch.randn(B, H, E, generator=g, device=dev, dtype=dt)
            blocks = size_query("trs_attn_pool_ragged_blocks", B, ML, E, H, code, 1)
            dx = torch.zeros(n, E, dtype=dt, device=dev)
            dwp = torch.empty(blocks, 2 * E, E, dtype=torch.float32, device=dev)
            dbp = torch.empty(blocks, 2 * E, dtype=torch.float32, device=dev)
            ws_bytes = size_query("trs_attn_pool_ragged_bwd_workspace_bytes", blocks, ML, E, H)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
            oc = index_dtype_code(offsets)

            def k_fwd():
                call("trs_attn_pool_ragged_fwd", ptr(w), V, E, code, ptr(ids), index_dtype_code(ids), n, ptr(offsets), oc,
                     B + 1, B, ML, -1, ptr(wqk), ptr(bqk), H, 1, ptr(xt), ptr(cn), None, stream_ptr())

            def k_bwd():
                call("trs_attn_pool_ragged_bwd", ptr(w), V, E, code, ptr(ids), index_dtype_code(ids), n, ptr(offsets), oc,
                     B + 1, B, ML, -1, ptr(wqk), ptr(bqk), H, 1, ptr(gx), ptr(dx), ptr(dwp), ptr(dbp), blocks, ptr(ws),
                     ws_bytes, None, stream_ptr())

            for name, f, fl in (("trs_attn_pool_ragged_fwd", k_fwd, flops), ("trs_attn_pool_ragged_bwd", k_bwd, 4 * flops)):
                ts = sorted(timeit(f, iters=a.iters, warm=2)[0] for _ in range(a.rounds))
                med = ts[len(ts) // 2]
                print(f"H={H} {shape:8s} kernel   {name:26s} med {med * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. "
                      f"{ts[-1] * 1e6:9.1f} us  {fl / med / 1e12:6.1f} TFLOP/s ({blocks} workgroups in the backward)",
                      flush=True)
            del ids, padded, dx


def bench_prm(a):
    """Residual self-attention (csrc/self_attn.hip) at (B, L, E, H) and PersonalizedReRankingModel with ``--layers``
    encoder layers over it, fp32 and bf16: the block ``x + MHA(x)`` forward and forward + backward, and the whole harness
    model forward + backward, the fused default against the SAME modules with the switch off (fused.SELF_ATTN = False: the
    nn.MultiheadAttention composition a user of the reference runs today), taking turns inside every round; then the two
    kernels alone with algorithmic GB/s.  Every figure is the median of ``--rounds`` per-round medians with their min..max."""
    import torch.nn as nn
    from harness.ltr_models import PersonalizedReRankingModel
    from torecsys_amd import fused as FU
    from torecsys_amd._abi import call, ptr, size_query, stream_ptr, value_dtype_code
    dev = torch.device("cuda:0")
    B, L, E, H, layers = a.B, a.L, a.E, a.H, a.layers
    flops = B * (8 * L * E * E + 4 * L * L * E)
    switch = FU.SELF_ATTN
    for dt, s in ((torch.float32, 4), (torch.bfloat16, 2)):
        g = torch.Generator(device=dev).manual_seed(1234)
        mha = nn.MultiheadAttention(E, H)
        with torch.no_grad():
            mha.in_proj_bias.normal_(0, 0.1)
            mha.out_proj.bias.normal_(0, 0.1)
        mha = mha.to(dev).to(dt)
        x = torch.randn(B, L, E, generator=g, device=dev, dtype=dt).requires_grad_()
        gout = torch.randn(B, L, E, generator=g, device=dev, dtype=dt)
        torch.manual_seed(7)
        model = PersonalizedReRankingModel(embed_size=E, max_num_position=L, encoding_size=E, num_heads=H,
                                           num_layers=layers).to(dev).to(dt).train()
        gm = torch.randn(B, L, generator=g, device=dev, dtype=dt)
        alg_f = 2 * B * L * E * s + (4 * E * E + 4 * E) * s
        alg_b = 3 * B * L * E * s + (4 * E * E + 4 * E) * s
        print(f"self-attention B={B} L={L} E={E} H={H} layers={layers} {dt} path {F_.self_attn_path(L, E, H, dt)}, "
              f"{a.rounds} rounds x {a.iters} launches; block forward {alg_f / 1e6:.0f} MB (alg), {flops / 1e9:.1f} GFLOP",
              flush=True)

        def block(fused):
            def f():
                FU.SELF_ATTN = fused
                return FU.residual_self_attention(mha, x)
            return f

        def block_fb(fused):
            def run():
                FU.SELF_ATTN = fused
                x.grad = None
                for p in mha.parameters():
                    p.grad = None
                FU.residual_self_attention(mha, x).backward(gout)
            return run

        def model_fb(fused):
            def run():
                FU.SELF_ATTN = fused
                for p in model.parameters():
                    p.grad = None
                model(x.detach()).rename(None).backward(gm)
            return run

        names = ("self_attn (HIP)", "composition (ATen)")
        for what, mk in (("block fwd", block), ("block fwd+bwd", block_fb), ("model fwd+bwd", model_fb)):
            cands = list(zip(names, (mk(True), mk(False))))
            per = {n: [] for n in names}
            for _ in range(a.rounds):
                for n, f in cands:
                    if what == "block fwd":
                        with torch.no_grad():
                            per[n].append(timeit(f, iters=a.iters, warm=2)[0])
                    else:
                        per[n].append(timeit(f, iters=a.iters, warm=2)[0])
            med = {}
            for n, ts in per.items():
                ts = sorted(ts)
                med[n] = ts[len(ts) // 2]
                print(f"{what:14s} {n:20s} med {med[n] * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us",
                      flush=True)
            print(f"{what:14s} composition / self_attn = {med[names[1]] / med[names[0]]:.2f}x", flush=True)
        FU.SELF_ATTN = switch
        # the two kernels alone
        xd = x.detach()
        w_in, b_in = mha.in_proj_weight.detach(), mha.in_proj_bias.detach()
        w_out, b_out = mha.out_proj.weight.detach(), mha.out_proj.bias.detach()
        code = value_dtype_code(xd)
        y = torch.empty_like(xd)
        dx = torch.empty_like(xd)
        blocks = size_query("trs_self_attn_blocks", B, L, E, H, code, 1)
        ws_bytes = size_query("trs_self_attn_bwd_workspace_bytes", blocks, E)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def k_fwd():
            call("trs_self_attn_fwd", ptr(xd), B, L, E, H, code, ptr(w_in), ptr(b_in), ptr(w_out), ptr(b_out), ptr(y),
                 stream_ptr())

        def k_bwd():
            call("trs_self_attn_bwd", ptr(xd), B, L, E, H, code, ptr(w_in), ptr(b_in), ptr(w_out), ptr(b_out), ptr(gout),
                 ptr(dx), ptr(ws), ws_bytes, blocks, stream_ptr())

        for name, f, alg, fl in (("trs_self_attn_fwd", k_fwd, alg_f, flops), ("trs_self_attn_bwd", k_bwd, alg_b, 3 * flops)):
            ts = sorted(timeit(f, iters=a.iters, warm=2)[0] for _ in range(a.rounds))
            med = ts[len(ts) // 2]
            print(f"kernel         {name:20s} med {med * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us  "
                  f"{alg / med / 1e9:7.1f} GB/s (alg)  {fl / med / 1e12:5.1f} TFLOP/s ({blocks} workgroups in the backward)",
                  flush=True)
        del model, mha, x, gout, y, dx, ws


def bench_senet(a):
    """ComposeExcitationNetworkLayer (csrc/senet.hip): forward under no_grad and forward + backward, bf16 and fp32, the
    fused family at (65 536, 39, 64, reduction 3) and the general family at a FAT-DeepFFM-like (4096, 400, 16, reduction 4),
    each against the ATen composition of the SAME module on the same inputs (pool -> fc -> einsum,
    compose_excitation_network.py:85-107), the candidates taking turns inside every round."""
    import torch.nn as nn
    from torecsys_amd.layers import SENETLayer
    dev = torch.device("cuda:0")

    def aten(m):
        def run(x):
            pooled = m.pooling(x).flatten(1)
            return torch.einsum("ijk,ijh->ijk", x, m.fc(pooled).unsqueeze(-1))
        return run

    for (B, M, E, r, family) in ((65536, 39, 64, 3, "fused"), (4096, 400, 16, 4, "general")):
        for dt in (torch.bfloat16, torch.float32):
            s = 2 if dt == torch.bfloat16 else 4
            g = torch.Generator(device=dev).manual_seed(77)
            torch.manual_seed(78)
            m = SENETLayer(M, r, squared=False).to(dev).to(dt)
            x = (0.5 * torch.randn(B, M, E, generator=g, device=dev) + torch.randn(B, M, 1, generator=g, device=dev)).to(dt)
            gout = torch.randn(B, M, E, generator=g, device=dev).to(dt)
            xg = x.clone().requires_grad_()
            block = B * M * E * s
            cands = [("senet (HIP, %s)" % family, lambda t: m(t).rename(None)), ("composition (ATen)", aten(m))]
            with torch.no_grad():
                d = float((cands[0][1](x).float() - cands[1][1](x).float()).abs().max())
            print(f"senet B={B} M={M} H={M // r} E={E} {str(dt)[6:]} block {block / 1e6:.0f} MB; max |HIP - ATen| = {d:.3e}",
                  flush=True)

            def fwd(f):
                return lambda: f(x)

            def fwd_bwd(f):
                def run():
                    xg.grad = None
                    for p in m.parameters():
                        p.grad = None
                    f(xg).backward(gout)
                return run

            for what, alg in (("fwd", 2 * block), ("fwd+bwd", 5 * block)):
                per = {name: [] for name, _ in cands}
                for _ in range(a.rounds):
                    for name, f in cands:
                        if what == "fwd":
                            with torch.no_grad():
                                per[name].append(timeit(fwd(f), iters=a.iters, warm=2)[0])
                        else:
                            per[name].append(timeit(fwd_bwd(f), iters=a.iters, warm=2)[0])
                for name, ts in per.items():
                    ts = sorted(ts)
                    med = ts[len(ts) // 2]
                    print(f"{family:7s} {str(dt)[6:]:8s} {what:8s} {name:24s} med {med * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. "
                          f"{ts[-1] * 1e6:9.1f} us  {alg / med / 8e12 * 100:5.1f}% of 8 TB/s on {alg / 1e6:.0f} MB (alg)",
                          flush=True)
            if family == "general":
                # the share of the fp32 excitation (two Linear + ReLU on (B, M) / (B, H), forward and backward)
                z = torch.randn(B, M, device=dev, requires_grad=True)
                ga = torch.randn(B, M, device=dev)

                def exc():
                    z.grad = None
                    for p in m.parameters():
                        p.grad = None
                    red, add = m.fc.ReductionLinear, m.fc.AdditionLinear
                    h = torch.relu(nn.functional.linear(z, red.weight.float(), red.bias.float()))
                    torch.relu(nn.functional.linear(h, add.weight.float(), add.bias.float())).backward(ga)
                ts = sorted(timeit(exc, iters=a.iters, warm=2)[0] for _ in range(a.rounds))
                print(f"general {str(dt)[6:]:8s} fwd+bwd  fp32 excitation alone (ATen) med {ts[len(ts) // 2] * 1e6:9.1f} us  spread "
                      f"{ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us", flush=True)
            del x, gout, xg, m
            torch.cuda.empty_cache()


def bench_compact(a):
    """Owner side of a large row-sharded table: K = B * N received ids over ``--shard-rows`` rows, uniform and Zipf(1.05).
    First the compaction alone: functional.compact_rows (hash slots) and compact_rows_dense (densely numbered, what
    dist.py uses) against torch.unique(return_inverse=True), which also reads the distinct count on the host.  Then the
    whole owner update through each: compaction, bucket build over the compact rows, mapped Adagrad update of a
    (rows, E) table.  The candidates take turns inside a round; median of the per-round medians with their min..max."""
    from torecsys_amd.optim import FusedSparseAdagrad
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    dev = torch.device("cuda:0")
    K, V, E = a.B * a.N, a.shard_rows or 125_000_000, a.E
    g = torch.Generator(device=dev).manual_seed(1234)
    u = torch.rand(K, generator=g, device=dev, dtype=torch.float64)
    zipf = ((V ** -0.05 - 1.0) * u + 1.0) ** (1.0 / -0.05)      # Zipf(1.05) ranks: the continuous CDF inverted
    ids = {"uniform": torch.randint(0, V, (K,), generator=g, device=dev).to(torch.int32),
           "zipf(1.05)": (zipf.long() - 1).clamp_(0, V - 1).to(torch.int32)}
    table = torch.zeros(V, E, dtype=dt, device=dev)
    grad = torch.randn(K, E, generator=g, device=dev, dtype=dt)
    opt = FusedSparseAdagrad(0.01)
    opt.state_for(table, table)
    print(f"row compaction K={K} ids over {V} rows, E={E} {a.dtype}; {a.rounds} rounds x {a.iters} launches", flush=True)

    def unique_route(x):
        uniq, inv = torch.unique(x, return_inverse=True)
        return uniq.to(torch.int32), inv.to(torch.int32).view(-1, 1)

    def slot_route(x):
        row_map, inv = F_.compact_rows(x)
        return row_map, inv.view(-1, 1)

    def dense_route(x):
        dense_map, inv = F_.compact_rows_dense(x)
        return dense_map, inv.view(-1, 1)

    def update(route, x):
        def run():
            F_.clear_caches()          # the buckets are rebuilt every step, as in training
            row_map, inv = route(x)
            rb = F_.row_buckets(inv, None, row_map.numel())
            F_.scatter_rows_update_mapped(rb, table, opt, grad, row_map, key=table)
        return run

    routes = [("compact_rows", slot_route), ("compact_rows_dense", dense_route), ("torch.unique", unique_route)]
    for name, x in ids.items():
        cands = [(label, lambda route=route, x=x: route(x)) for label, route in routes]
        cands += [("owner update, " + label, update(route, x)) for label, route in routes]
        meds = {c: [] for c, _ in cands}
        for _ in range(a.rounds):
            for c, fn in cands:
                meds[c].append(timeit(fn, iters=a.iters, warm=2)[0])
        print(f"  {name}: {int(torch.unique(x).numel())} distinct rows", flush=True)
        for c, _ in cands:
            ts = sorted(meds[c])
            print(f"    {c:34s} med {ts[len(ts) // 2] * 1e6:9.1f} us   ({ts[0] * 1e6:.1f} .. {ts[-1] * 1e6:.1f})",
                  flush=True)


def bench_rowwise(a):
    """The fused optimizer step alone -- the bucket walk with the step as its sink -- for SGD, Adagrad, row-wise Adagrad
    and Adam on one (V, E) table: the backward of ``F_.gather_rows(..., opt=)`` (plain walk) and of
    ``F_.embed_fm(..., opt=)`` with the per-sample FM gradient of the models (the lean fm1 walk).  The forward runs once
    and the row buckets are built by it, so the timed launch is the update walk.  Uniform and Zipf-like indices; the
    optimizers take turns inside a round; median of the per-round medians with their min..max.  With ``--shard-rows`` on
    the command line also the owner side of a row-sharded table of that many rows: compaction, bucket build and the
    mapped update, as ``--what compact`` times it.  On a bf16 table every optimizer runs a second time with
    ``stochastic_rounding=True``."""
    from torecsys_amd.optim import FusedSparseAdagrad, FusedSparseAdam, FusedSparseRowWiseAdagrad, FusedSparseSGD
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    dev = torch.device("cuda:0")
    B, N, E, V = a.B, a.N, a.E, a.V
    g = torch.Generator().manual_seed(1234)
    per = V // N
    fs = [per] * (N - 1) + [V - per * (N - 1)]
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.tensor(fs), 0)[:-1]]).to(dev)
    zcols = [((f ** torch.rand(B, 1, generator=g, dtype=torch.float64) - 1).clamp_(0, f - 1)).long() for f in fs]
    indices = {"uniform": torch.cat([torch.randint(0, f, (B, 1), generator=g) for f in fs], 1).to(dev),
               "zipf": torch.cat(zcols, 1).to(dev)}
    ge = (torch.randn(B, N, E, generator=g) * 1e-2).to(dt).to(dev)
    gf1 = (torch.randn(B, 1, generator=g) * 1e-2).to(dt).to(dev)
    makers = [("sgd", lambda: FusedSparseSGD(1e-3)), ("adagrad", lambda: FusedSparseAdagrad(1e-3)),
              ("rowwise adagrad", lambda: FusedSparseRowWiseAdagrad(1e-3)), ("adam", lambda: FusedSparseAdam(1e-3))]
    if dt == torch.bfloat16:
        # the same walks with the new bf16 weights rounded stochastically (one Philox call per touched 16-byte vector);
        # they take turns with the plain ones inside every round
        sr = dict(stochastic_rounding=True, seed=1234)
        makers += [("sgd, stoch. rounding", lambda: FusedSparseSGD(1e-3, **sr)),
                   ("adagrad, stoch. rounding", lambda: FusedSparseAdagrad(1e-3, **sr)),
                   ("rowwise adagrad, stoch. rounding", lambda: FusedSparseRowWiseAdagrad(1e-3, **sr)),
                   ("adam, stoch. rounding", lambda: FusedSparseAdam(1e-3, **sr))]
    print(f"fused optimizer step alone, B={B} N={N} E={E} {a.dtype}, {V} rows; {a.rounds} rounds x {a.iters} launches",
          flush=True)

    def table():
        return (torch.randn(V, E, generator=g) * 0.1).to(dt).to(dev).requires_grad_()

    def show(title, cands):
        meds = {c: [] for c, _ in cands}
        for _ in range(a.rounds):
            for c, fn in cands:
                meds[c].append(timeit(fn, iters=a.iters, warm=2)[0])
        print(f"  {title}", flush=True)
        for c, _ in cands:
            ts = sorted(meds[c])
            print(f"    {c:34s} med {ts[len(ts) // 2] * 1e6:9.1f} us   ({ts[0] * 1e6:.1f} .. {ts[-1] * 1e6:.1f})", flush=True)

    for name, idx in indices.items():
        F_.clear_caches()
        plain, folded, keep = [], [], []
        for label, mk in makers:
            w = table()
            out = F_.gather_rows(w, idx, off, opt=mk())
            plain.append((label, lambda out=out: out.backward(ge, retain_graph=True)))
            w2 = table()
            emb, fm, _ = F_.embed_fm(w2, idx, off, None, True, opt=mk())
            folded.append((label, lambda emb=emb, fm=fm: torch.autograd.backward([emb, fm], [ge, gf1.expand(B, E)],
                                                                                 retain_graph=True)))
            keep += [w, w2]
        show(f"{name}: gather_rows backward (plain walk)", plain)
        show(f"{name}: embed_fm backward (per-sample FM gradient folded in)", folded)
        del plain, folded, keep
        torch.cuda.empty_cache()

    if a.shard_rows is None:
        return
    K, Vs = B * N, a.shard_rows
    gd = torch.Generator(device=dev).manual_seed(1234)
    u = torch.rand(K, generator=gd, device=dev, dtype=torch.float64)
    zipf = ((Vs ** -0.05 - 1.0) * u + 1.0) ** (1.0 / -0.05)      # Zipf(1.05) ranks: the continuous CDF inverted
    ids = {"uniform": torch.randint(0, Vs, (K,), generator=gd, device=dev).to(torch.int32),
           "zipf(1.05)": (zipf.long() - 1).clamp_(0, Vs - 1).to(torch.int32)}
    shard = torch.zeros(Vs, E, dtype=dt, device=dev)
    grad = (torch.randn(K, E, generator=gd, device=dev) * 1e-2).to(dt)
    print(f"owner update of a {Vs}-row shard (compaction, bucket build, mapped update), K={K} ids", flush=True)
    for name, x in ids.items():
        cands = []
        for label, mk in makers:
            opt = mk()

            def run(opt=opt, x=x):
                F_.clear_caches()          # the buckets are rebuilt every step, as in training
                row_map, inv = F_.compact_rows_dense(x)
                rb = F_.row_buckets(inv.view(-1, 1), None, row_map.numel())
                F_.scatter_rows_update_mapped(rb, shard, opt, grad, row_map, key=shard)
            cands.append((label, run))
        show(f"{name}: {int(torch.unique(x).numel())} distinct rows", cands)


def bench_moe(a):
    """MixtureOfExpertsLayer (csrc/moe.hip) at B = 65 536, D = 2496, 8 experts x 16 outputs (hidden layers 128, 64),
    G = 4 gates, bf16 and fp32.  The gate part -- everything behind the concatenated expert outputs: the stacking of the
    gate parameters, the GEMM, the kernel -- against the ATen composition of the SAME module (G x Linear + Softmax,
    unflatten, cat, einsum: mixture_of_experts.py:137-160), forward under no_grad and forward + backward, the candidates
    taking turns inside every round; every figure is the median over all rounds x iters timed launches (events on the
    launch stream) after 10 warm-ups.  Then the two kernels alone against their algorithmic bytes, and the experts' share
    of the whole layer's forward + backward."""
    from torecsys_amd.layers import DNNLayer, MOELayer
    dev = torch.device("cuda:0")
    B, N, E, X, Oi, G = 65536, 39, 64, 8, 16, 4
    D, K = N * E, X * Oi

    def samples(fn, iters):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for s0, s1 in evs:
            s0.record()
            fn()
            s1.record()
        torch.cuda.synchronize()
        return [s0.elapsed_time(s1) * 1e-3 for s0, s1 in evs]

    def race(cands):
        """{name: sorted seconds of rounds x iters launches}, 10 warm-ups each, the candidates taking turns"""
        per = {name: [] for name, _ in cands}
        for _, f in cands:
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for name, f in cands:
                per[name] += samples(f, a.iters)
        return {name: sorted(ts) for name, ts in per.items()}

    def show(tag, name, ts, alg=None):
        med = ts[len(ts) // 2]
        extra = "" if alg is None else f"  {alg / med / 1e9:7.1f} GB/s = {alg / med / 8e12 * 100:5.1f}% of 8 TB/s on {alg / 1e6:.0f} MB (alg)"
        print(f"{tag:22s} {name:26s} med {med * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us "
              f"({len(ts)} launches){extra}", flush=True)
        return med

    for dt in (torch.bfloat16, torch.float32):
        s = 2 if dt == torch.bfloat16 else 4
        name_dt = str(dt)[6:]
        g = torch.Generator(device=dev).manual_seed(91)
        torch.manual_seed(92)
        m = MOELayer(inputs_size=D, output_size=K, num_experts=X, expert_func=DNNLayer, num_gates=G,
                     expert_inputs_size=D, expert_output_size=Oi, expert_layer_sizes=[128, 64]).to(dev).to(dt)
        x = torch.randn(B, N, E, generator=g, device=dev).to(dt).requires_grad_()
        gout = torch.randn(B, G, K, generator=g, device=dev).to(dt)
        x2 = x.detach().reshape(B, D).requires_grad_()
        e = torch.randn(B, K, generator=g, device=dev).to(dt).requires_grad_()
        linears = [gate.Linear for gate in m.gates.values()]
        gate_params = [p for lin in linears for p in lin.parameters()]

        def gate_hip():
            return F_.moe_gate(x2, torch.cat([lin.weight for lin in linears]), torch.cat([lin.bias for lin in linears]), e)

        def gate_aten():
            w = torch.cat([torch.softmax(lin(x2), dim=1).unflatten(1, (1, K)) for lin in linears], dim=1)
            return torch.einsum("ik,ijk->ijk", e, w)

        def fwd_bwd(f, leaves):
            def run():
                for t in leaves:
                    t.grad = None
                f().backward(gout)
            return run

        with torch.no_grad():
            d = float((gate_hip().float() - gate_aten().float()).abs().max())
        print(f"moe B={B} D={D} experts {X} x {Oi} (K={K}) G={G} {name_dt}; max |HIP - ATen| of the gate part = {d:.3e}; "
              f"{a.rounds} rounds x {a.iters} launches", flush=True)
        cands = [("moe_gate (HIP)", gate_hip), ("composition (ATen)", gate_aten)]
        with torch.no_grad():
            for name, ts in race(cands).items():
                show(f"gate {name_dt} fwd", name, ts)
        leaves = [x2, e] + gate_params
        for name, ts in race([(n, fwd_bwd(f, leaves)) for n, f in cands]).items():
            show(f"gate {name_dt} fwd+bwd", name, ts)
        # the two kernels alone
        with torch.no_grad():
            logits = torch.randn(B, G * K, generator=g, device=dev)
            bias = torch.cat([lin.bias for lin in linears]).detach()
            ed = e.detach()
            res = race([("trs_moe_gate_fwd", lambda: F_.moe_gate_forward_raw(logits, bias, ed)),
                        ("trs_moe_gate_bwd", lambda: F_.moe_gate_backward_raw(logits, bias, ed, gout))])
            show(f"kernel {name_dt}", "trs_moe_gate_fwd", res["trs_moe_gate_fwd"], B * G * K * 4 + B * K * s + B * G * K * s)
            show(f"kernel {name_dt}", "trs_moe_gate_bwd", res["trs_moe_gate_bwd"],
                 B * G * K * (4 + s) + B * K * s + B * G * K * s + B * K * s)
            del logits
        # the experts' share of the whole layer
        gk = torch.randn(B, K, generator=g, device=dev).to(dt)

        def experts_only():
            return torch.cat([ex(x2).rename(None) for ex in m.experts.values()], dim=1)

        def layer():
            for t in [x] + list(m.parameters()):
                t.grad = None
            m(x).rename(None).backward(gout)

        def experts():
            for t in [x2] + list(m.experts.parameters()):
                t.grad = None
            experts_only().backward(gk)

        res = race([("whole layer", layer), ("experts alone", experts)])
        t_layer = show(f"layer {name_dt} fwd+bwd", "whole layer", res["whole layer"])
        t_exp = show(f"layer {name_dt} fwd+bwd", "experts alone (+ cat)", res["experts alone"])
        print(f"layer {name_dt}: the experts take {t_exp / t_layer * 100:.0f}% of the layer's forward + backward", flush=True)
        del m, x, x2, e, gout, gk
        torch.cuda.empty_cache()


def bench_routing(a):
    """Dynamic routing (csrc/dynamic_routing.hip) at (B, N, E, R, max_num_caps, num_iter): forward and forward+backward of
    DynamicRoutingLayer with its own noise draw, the fused path against the SAME module with the switch off
    (layers.DYNAMIC_ROUTING = False: the ATen composition), taking turns inside every round; the peak allocation of
    either; then the two kernels alone with their algorithmic bytes (the noise once per direction dominates) as a
    fraction of 8 TB/s, and the noise draw by itself.  Every figure is the median of ``--rounds`` per-round medians with
    their min..max."""
    from torecsys_amd import layers as L
    from torecsys_amd._abi import call, ptr, stream_ptr, value_dtype_code
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    s = 2 if dt == torch.bfloat16 else 4
    dev = torch.device("cuda:0")
    B, N, E, R, iters, launches = a.B, a.L, a.E, a.R, a.routing_iters, a.iters
    g = torch.Generator(device=dev).manual_seed(1234)
    m = L.DynamicRoutingLayer(E, R, a.caps, iters).to(dev).to(dt)
    K = m._dynamic_interest_number(N)
    x = (0.3 * torch.randn(B, N, E, generator=g, device=dev)).to(dt).requires_grad_()
    gout = torch.randn(B, K, R, generator=g, device=dev, dtype=dt)
    alg_f = B * (K * N * R * s + 4 * N * R + K * R * s + 4 * K * (N + R))
    alg_b = B * (K * N * R * s + 4 * K * (N + R) + K * R * s + N * R * s)
    print(f"dynamic routing B={B} N={N} E={E} R={R} K'={K} num_iter={iters} {a.dtype} path "
          f"{F_.dynamic_routing_path(N, R, K, dt)}, {a.rounds} rounds x {launches} launches; one (B, K', N, R) tensor: "
          f"{B * K * N * R * s / 2**20:.0f} MiB; exp per forward {B * K * N * R * iters / 1e9:.2f} G", flush=True)

    def module(fused):
        def f():
            L.DYNAMIC_ROUTING = fused
            return m(x).rename(None)
        return f

    def fwd_bwd(f):
        def run():
            x.grad = m.S.grad = None
            f().backward(gout)
        return run

    cands = [("dynamic_routing (HIP)", module(True)), ("composition (ATen)", module(False))]
    for name, f in cands:
        for what, run in (("fwd", f), ("fwd+bwd", fwd_bwd(f))):
            ctx = torch.no_grad() if what == "fwd" else torch.enable_grad()
            with ctx:
                run()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                y = run()
                torch.cuda.synchronize()
            print(f"{name:22s} {what:8s} peak allocation {(torch.cuda.max_memory_allocated() - base) / 2**20:9.1f} MiB",
                  flush=True)
            del y
    res = {}
    for what in ("fwd", "fwd+bwd"):
        per = {name: [] for name, _ in cands}
        for _ in range(a.rounds):
            for name, f in cands:
                if what == "fwd":
                    with torch.no_grad():
                        per[name].append(timeit(f, iters=launches, warm=2)[0])
                else:
                    per[name].append(timeit(fwd_bwd(f), iters=launches, warm=2)[0])
        for name, ts in per.items():
            ts = sorted(ts)
            res[(what, name)] = ts[len(ts) // 2]
            print(f"{what:8s} {name:22s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. "
                  f"{ts[-1] * 1e6:9.1f} us", flush=True)
        print(f"{what:8s} composition / dynamic_routing = "
              f"{res[(what, 'composition (ATen)')] / res[(what, 'dynamic_routing (HIP)')]:.2f}x", flush=True)
    L.DYNAMIC_ROUTING = True
    x.grad = m.S.grad = None
    # the two kernels alone, and the noise draw
    code = value_dtype_code(x)
    with torch.no_grad():
        pri = torch.mm(x.reshape(B * N, E).float(), m.S.float()).view(B, N, R)
    noise = torch.randn(B, K, N, R, dtype=dt, device=dev)
    out = torch.empty(B, K, R, dtype=dt, device=dev)
    c = torch.empty(B, K, N, dtype=torch.float32, device=dev)
    z = torch.empty(B, K, R, dtype=torch.float32, device=dev)
    dpri = torch.empty(B, N, R, dtype=dt, device=dev)

    def k_fwd():
        call("trs_dynamic_routing_fwd", ptr(pri), ptr(noise), B, N, R, K, iters, code, ptr(out), ptr(c), ptr(z), stream_ptr())

    def k_bwd():
        call("trs_dynamic_routing_bwd", ptr(noise), ptr(c), ptr(z), ptr(gout), B, N, R, K, code, ptr(dpri), stream_ptr())

    def draw():
        torch.randn(B, K, N, R, dtype=dt, device=dev)

    for name, f, alg in (("trs_dynamic_routing_fwd", k_fwd, alg_f), ("trs_dynamic_routing_bwd", k_bwd, alg_b),
                         ("torch.randn (noise)", draw, B * K * N * R * s)):
        ts = sorted(timeit(f, iters=launches, warm=2)[0] for _ in range(a.rounds))
        med = ts[len(ts) // 2]
        print(f"kernel   {name:24s} med {med * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us  "
              f"{alg / 1e6:8.0f} MB (alg) {alg / med / 1e12:5.2f} TB/s = {alg / med / 8e12:.2f} of 8 TB/s", flush=True)


def bench_seq(a):
    """Sequence embedding (csrc/seq_rnn.hip) at (B, L, E, V, cell): forward and forward+backward of
    SequenceIndicesEmbedding(output_method='avg_pooling') with lengths uniform in [1, L], the fused path against the SAME
    module with the switch off (inputs.SEQ_RNN_FUSED = False: HIP gather, the module's own nn.LSTM / nn.GRU / nn.RNN on a
    packed sequence with its host read of the lengths, ATen mean), taking turns inside every round; the forward's peak
    allocation of either; then the two kernels alone with their FMA rate.  Every figure is the median of ``--rounds``
    per-round medians with their min..max."""
    from torecsys_amd import inputs as I
    from torecsys_amd._abi import call, index_dtype_code, ptr, size_query, stream_ptr, value_dtype_code
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    s = 2 if dt == torch.bfloat16 else 4
    dev = torch.device("cuda:0")
    B, L, E, V, cell = a.B, a.L, a.E, a.V, a.cell
    G = F_.SEQ_RNN_GATES[F_.SEQ_RNN_CELLS[cell]]
    g = torch.Generator(device=dev).manual_seed(1234)
    lengths = torch.randint(1, L + 1, (B,), generator=g, device=dev)
    idx = torch.randint(1, V, (B, L), generator=g, device=dev)
    idx = torch.where(torch.arange(L, device=dev).view(1, L) < lengths.view(B, 1), idx, torch.zeros_like(idx))
    m = I.SequenceIndicesEmbedding(embed_size=E, field_size=V, rnn_method=cell, output_method="avg_pooling").to(dev).to(dt)
    gout = torch.randn(B, 1, E, generator=g, device=dev, dtype=dt)
    steps = int(lengths.sum())
    flops = 2.0 * steps * 2 * G * E * E                     # the two matrix-vector products of every live step
    alg = steps * (8 + E * s) + B * (8 + E * s) + 2 * G * E * E * s
    print(f"sequence embedding B={B} L={L} E={E} V={V} {cell} {a.dtype} path {F_.seq_rnn_path(cell, L, E, dt)}, live steps "
          f"{steps / (B * L):.2f} of B*L, {a.rounds} rounds x {a.iters} launches; forward: {alg / 1e6:.0f} MB (alg), "
          f"{flops / 1e9:.1f} GFLOP", flush=True)

    def module(fused):
        def f():
            I.SEQ_RNN_FUSED = fused
            return m(idx, lengths).rename(None)
        return f

    def fwd_bwd(f):
        def run():
            F_.clear_caches()          # the row buckets of the batch are rebuilt every step, as in training
            for p in m.parameters():
                p.grad = None
            f().backward(gout)
        return run

    cands = []
    for name, f in (("seq_rnn (HIP)", module(True)), ("composition (ATen)", module(False))):
        try:
            fwd_bwd(f)()
            torch.cuda.synchronize()
            cands.append((name, f))
        except Exception as e:      # noqa: BLE001 -- a cell / dtype this torch build does not serve
            print(f"{name:22s} not supported on this torch build ({type(e).__name__}: {str(e)[:120]})", flush=True)
    for name, f in cands:
        with torch.no_grad():
            f()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = f()
        torch.cuda.synchronize()
        print(f"{name:22s} forward peak allocation {(torch.cuda.max_memory_allocated() - base) / 2**20:9.1f} MiB "
              f"((B, L, E) block: {B * L * E * s / 2**20:.1f} MiB)", flush=True)
        del y
    res = {}
    for what in ("fwd", "fwd+bwd"):
        per = {name: [] for name, _ in cands}
        for _ in range(a.rounds):
            for name, f in cands:
                if what == "fwd":
                    with torch.no_grad():
                        per[name].append(timeit(f, iters=a.iters, warm=2)[0])
                else:
                    per[name].append(timeit(fwd_bwd(f), iters=a.iters, warm=2)[0])
        for name, ts in per.items():
            ts = sorted(ts)
            res[(what, name)] = ts[len(ts) // 2]
            print(f"{what:8s} {name:22s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. "
                  f"{ts[-1] * 1e6:9.1f} us", flush=True)
        if len(cands) == 2:
            print(f"{what:8s} composition / seq_rnn = "
                  f"{res[(what, 'composition (ATen)')] / res[(what, 'seq_rnn (HIP)')]:.2f}x", flush=True)
    I.SEQ_RNN_FUSED = True
    for p in m.parameters():
        p.grad = None
    # the two kernels alone (the backward without its GEMMs and the bucket walk behind it)
    w = m.embedding.weight.detach()
    wi, wh, bi, bh = (p.detach().contiguous() for p in m._rnn_params())
    code, ccode = value_dtype_code(w), F_.SEQ_RNN_CELLS[cell]
    out = torch.empty(B, E, dtype=dt, device=dev)
    scale = torch.empty(1, dtype=torch.float32, device=dev)
    h = torch.empty(B, L, E, dtype=dt, device=dev)
    c = torch.empty(B, L, E, dtype=torch.float32, device=dev) if cell == "lstm" else None
    dg = torch.empty(B, L, G * E, dtype=dt, device=dev)
    dgh = torch.empty(B, L, G * E, dtype=dt, device=dev) if cell == "gru" else None
    ws_bytes = size_query("trs_seq_rnn_workspace_bytes", ccode, E)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    g2 = gout.view(B, E)

    def k_fwd():
        call("trs_seq_rnn_fwd", ptr(w), V, E, code, ptr(idx), index_dtype_code(idx), ptr(lengths), index_dtype_code(lengths),
             B, L, ptr(wi), ptr(wh), ptr(bi), ptr(bh), ccode, 0, 1, ptr(scale), ptr(out), ptr(h), ptr(c), ptr(ws), ws_bytes,
             None, stream_ptr())

    def k_bwd():
        call("trs_seq_rnn_bwd", ptr(w), V, E, code, ptr(idx), index_dtype_code(idx), ptr(lengths), index_dtype_code(lengths),
             B, L, ptr(wi), ptr(wh), ptr(bi), ptr(bh), ccode, 0, ptr(scale), ptr(h), ptr(c), ptr(g2), ptr(dg), ptr(dgh),
             ptr(ws), ws_bytes, stream_ptr())

    for name, f, fl in (("trs_seq_rnn_fwd (saving h, c)", k_fwd, flops), ("trs_seq_rnn_bwd", k_bwd, 1.5 * flops)):
        ts = sorted(timeit(f, iters=a.iters, warm=2)[0] for _ in range(a.rounds))
        med = ts[len(ts) // 2]
        print(f"kernel   {name:30s} med {med * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us  "
              f"{fl / med / 1e12:6.1f} TFLOP/s", flush=True)


def bench_rank(a):
    """Pair scores + ranking loss (csrc/rank.hip) at (B, K, E, V): one shared table, Zipf(1.05) anchor and target ids,
    hinge loss (mean).  Forward + backward of (1) fused.EmbeddingPairScorer + losses.HingeLoss, (2) the same module with
    the switch off (functional.PAIR_SCORE = False: HIP gathers + ATen multiply / cosine, the HIP loss), (3) the
    reference-shaped composition -- the miner's (B (1+K), 2) id pairs, an aten::embedding gather of the (B (1+K), 2, E)
    block, the GMF / cosine on its halves, the hinge as ATen elementwise ops and the dense index_add gradient -- taking
    turns inside every round; then the score and loss kernels alone.  Every figure is the median of ``--rounds``
    per-round medians with their min..max."""
    import torch.nn.functional as TF
    from torecsys_amd.fused import EmbeddingPairScorer
    from torecsys_amd.losses import HingeLoss
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    s = 2 if dt == torch.bfloat16 else 4
    dev = torch.device("cuda:0")
    B, K, E, V, sim = a.B, a.neg, a.E, a.V, a.sim
    g = torch.Generator(device=dev).manual_seed(1234)
    cdf = torch.arange(1, V + 1, device=dev, dtype=torch.float64).pow(-1.05).cumsum(0)
    cdf /= cdf[-1].clone()

    def zipf(*shape):
        return torch.searchsorted(cdf, torch.rand(*shape, generator=g, device=dev, dtype=torch.float64)).clamp_(max=V - 1)

    a_idx, t_idx = zipf(B), zipf(B, 1 + K)
    m = EmbeddingPairScorer(E, V, None, sim).to(dev).to(dt)
    w = m.anchor.weight
    loss_fn = HingeLoss(margin=1.0, reduction="mean")
    alg = B * (2 + K) * (8 + E * s) + B * (1 + K) * s
    print(f"pair scores + ranking loss B={B} K={K} E={E} V={V} {sim} {a.dtype} path {F_.pair_score_path(E, dt)}, "
          f"{a.rounds} rounds x {a.iters} launches; forward: {alg / 1e6:.0f} MB (alg), reference block "
          f"{B * (1 + K) * 2 * E * s / 1e6:.0f} MB", flush=True)

    def module(fused):
        def f():
            F_.PAIR_SCORE = fused
            return loss_fn(m(a_idx, t_idx), None)
        return f

    pair_ids = torch.stack([a_idx.repeat_interleave(1 + K), t_idx.reshape(-1)], dim=1)      # what the miner hands over

    def reference_shaped():
        block = TF.embedding(pair_ids, w)                                                    # (B (1+K), 2, E)
        if sim == "dot":
            sc = (block[:, 0, :] * block[:, 1, :]).sum(dim=1)
        else:
            sc = TF.cosine_similarity(block[:, 0:1, :], block[:, 1:2, :], dim=2)
        sc = sc.view(B, 1 + K).float()
        return torch.clamp(1.0 - sc[:, :1] + sc[:, 1:], min=0.0).mean()

    def fwd_bwd(f):
        def run():
            F_.clear_caches()          # the row buckets of the batch are rebuilt every step, as in training
            w.grad = None
            f().backward()
        return run

    cands = [("pair_scores (HIP)", module(True)), ("switch off (gather+ATen)", module(False)),
             ("reference-shaped (ATen)", reference_shaped)]
    for name, f in cands:
        fwd_bwd(f)()
    torch.cuda.synchronize()
    res = {}
    for what in ("fwd", "fwd+bwd"):
        per = {name: [] for name, _ in cands}
        for _ in range(a.rounds):
            for name, f in cands:
                if what == "fwd":
                    with torch.no_grad():
                        per[name].append(timeit(f, iters=a.iters, warm=2)[0])
                else:
                    per[name].append(timeit(fwd_bwd(f), iters=a.iters, warm=2)[0])
        for name, ts in per.items():
            ts = sorted(ts)
            res[(what, name)] = ts[len(ts) // 2]
            print(f"{what:8s} {name:26s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. "
                  f"{ts[-1] * 1e6:9.1f} us", flush=True)
        for name in ("switch off (gather+ATen)", "reference-shaped (ATen)"):
            print(f"{what:8s} {name} / pair_scores = {res[(what, name)] / res[(what, 'pair_scores (HIP)')]:.2f}x", flush=True)
    F_.PAIR_SCORE = True
    w.grad = None
    # the kernels alone
    wd = w.detach()
    scores = F_.pair_scores_forward_raw(wd, a_idx, wd, t_idx, sim=sim)
    gs = torch.randn(B, 1 + K, generator=g, device=dev, dtype=dt)
    _, denom = F_.rank_loss_forward_raw(scores, None, "hinge", 1.0, None, "mean")
    kernels = [("trs_embed_pair_score_fwd", lambda: F_.pair_scores_forward_raw(wd, a_idx, wd, t_idx, sim=sim), alg),
               ("trs_embed_pair_score_bwd", lambda: F_.pair_scores_backward_raw(wd, a_idx, wd, t_idx, gs, sim=sim),
                B * (2 + K) * (8 + 2 * E * s) + B * (1 + K) * s),
               ("trs_rank_loss_fwd", lambda: F_.rank_loss_forward_raw(scores, None, "hinge", 1.0, None, "mean"),
                B * (1 + K) * s),
               ("trs_rank_loss_bwd", lambda: F_.rank_loss_backward_raw(scores, None, "hinge", 1.0, None, "mean", None, denom),
                2 * B * (1 + K) * s)]
    for name, f, nbytes in kernels:
        ts = sorted(timeit(f, iters=a.iters, warm=2)[0] for _ in range(a.rounds))
        med = ts[len(ts) // 2]
        print(f"kernel   {name:26s} med {med * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us  "
              f"{nbytes / med / 1e9:7.0f} GB/s = {nbytes / med / 8e12 * 100:5.1f}% of 8 TB/s on {nbytes / 1e6:.0f} MB (alg)",
              flush=True)


def bench_bagshard(a):
    """Sharded bag pooling (csrc/bag_shard.hip) on ONE GPU at (B, L, E, V), fp32 and bf16: the four kernels alone with this
    process playing rank 0 of ``--world`` (it routes its batch over W owners, pools the segments W senders with batches like
    its own would send to it, combines W slabs, expands W*B output gradients); the world-1 module forward + backward
    against the unsharded ListIndicesEmbedding (needs an nccl group of one rank, started here); and the wire bytes per
    rank of the partial-sum path against the rows path, from the formulas (byte counts, not measurements)."""
    import torch.distributed as dist
    from torecsys_amd.dist import HipOps, RowShardedListIndicesEmbedding, segment_starts, shard_ranges
    from torecsys_amd.inputs import ListIndicesEmbedding
    dev = torch.device("cuda:0")
    B, L, E, V, W = a.B, a.L, a.E, a.V, a.world
    ops = HipOps()
    g = torch.Generator(device=dev).manual_seed(1234)
    idx = torch.randint(0, V, (B, L), generator=g, device=dev)
    per, ranges = shard_ranges(V, W)
    lo, hi = ranges[0]
    print(f"sharded bag pooling B={B} L={L} E={E} V={V} world={W} (this process: rank 0, rows [{lo}, {hi})), "
          f"{a.rounds} rounds x {a.iters} launches", flush=True)
    for s in (4, 2):
        rows, parts, gback = (W - 1) / W * B * L * E * s, (W - 1) * B * E * 4, (W - 1) * B * E * s
        print(f"wire bytes per rank ({'fp32' if s == 4 else 'bf16'} table): forward rows {rows / 1e6:.1f} MB -> fp32 partials "
              f"{parts / 1e6:.1f} MB (x{rows / max(parts, 1):.2f}); backward rows {rows / 1e6:.1f} MB -> output gradient "
              f"{gback / 1e6:.1f} MB (x{rows / max(gback, 1):.2f})", flush=True)

    def report(name, fns):
        per_ = {n: [] for n, _ in fns}
        for _ in range(a.rounds):
            for n, f in fns:
                per_[n].append(timeit(f, iters=a.iters, warm=2)[0])
        for n, ts in per_.items():
            ts = sorted(ts)
            print(f"{name:5s} {n:44s} med {ts[len(ts) // 2] * 1e6:9.1f} us  spread {ts[0] * 1e6:9.1f} .. {ts[-1] * 1e6:9.1f} us",
                  flush=True)

    counts, seg_start, send_ids = ops.bag_route(idx, V, per, W)
    # what rank 0 receives: its own segment from each of W senders with batches like its own
    n0 = int(seg_start[B])
    ids = send_ids[:n0].repeat(W)
    rseg = segment_starts(counts[0].unsqueeze(0).expand(W, B).contiguous())
    for dt in (torch.float32, torch.bfloat16):
        name = "fp32" if dt == torch.float32 else "bf16"
        shard = torch.randn(hi - lo, E, generator=g, device=dev, dtype=dt)
        slabs = torch.randn(W, B, E, generator=g, device=dev)
        g_all = torch.randn(W * B, E, generator=g, device=dev, dtype=dt)
        report(name, [
            ("route (count + scan + place)", lambda: ops.bag_route(idx, V, per, W)),
            (f"pool_segments ({W * B} segments, {ids.numel()} ids)", lambda: ops.bag_pool_segments(shard, hi - lo, ids, rseg)),
            (f"combine ({W} slabs)", lambda: ops.bag_combine(slabs, 1.0 / L, dt)),
            ("expand_grad", lambda: ops.bag_expand_grad(g_all, ids, rseg, hi - lo, 0)),
        ])
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        for dt in (torch.float32, torch.bfloat16):
            name = "fp32" if dt == torch.float32 else "bf16"
            gout = torch.randn(B, 1, E, generator=g, device=dev, dtype=dt)
            plain = ListIndicesEmbedding(E, V, padding_idx=0, output_method="avg_pooling").to(dev).to(dt)
            shd = RowShardedListIndicesEmbedding(E, V, padding_idx=0, output_method="avg_pooling", dtype=dt, device=dev)

            def step(m):
                def run():
                    F_.clear_caches()
                    m.embedding.weight.grad = None
                    m(idx).rename(None).backward(gout)
                return run
            report(name, [("fwd+bwd ListIndicesEmbedding (unsharded)", step(plain)),
                          ("fwd+bwd RowShardedListIndicesEmbedding (world 1)", step(shd))])
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--N", type=int, default=39)
    ap.add_argument("--E", type=int, default=64)
    ap.add_argument("--V", type=int, default=1_000_000)
    ap.add_argument("--zipf", action="store_true")
    ap.add_argument("--what", default="all")
    ap.add_argument("--L", type=int, default=50, help="bag / attn / routing / seq: list length")
    ap.add_argument("--H", type=int, default=1, help="attn: attention heads")
    ap.add_argument("--pad", type=float, default=0.3, help="bag: share of padded positions")
    ap.add_argument("--exclude-padding", action="store_true", help="bag: also time bag_pool(exclude_padding=True)")
    ap.add_argument("--weighted", action="store_true", help="bag: also time the weighted sum (per_sample_weights)")
    ap.add_argument("--rounds", type=int, default=5, help="bag / senet / compact / moe / routing: alternating rounds")
    ap.add_argument("--iters", type=int, default=10, help="bag / senet / compact / moe / routing: timed launches per round")
    ap.add_argument("--routing-iters", type=int, default=3, help="routing: num_iter of the layer")
    ap.add_argument("--R", type=int, default=64, help="routing: routed size")
    ap.add_argument("--caps", type=int, default=8, help="routing: max_num_caps")
    ap.add_argument("--shard-rows", type=int, default=None,
                    help="rows of the owner's shard; compact: 125 000 000 when not given; rowwise: the mapped update runs "
                         "only when given")
    ap.add_argument("--cell", default="lstm", choices=["lstm", "gru", "rnn"], help="seq: the recurrent cell")
    ap.add_argument("--neg", type=int, default=10, help="rank: sampled negatives per sample")
    ap.add_argument("--sim", default="dot", choices=["dot", "cosine"], help="rank: the similarity")
    ap.add_argument("--layers", type=int, default=2, help="prm: encoder layers of the model")
    ap.add_argument("--world", type=int, default=8, help="bagshard: the world size whose rank 0 this process plays")
    ap.add_argument("--shape", default="fixed,uniform,longtail", help="ragged: bag-length distributions to run")
    ap.add_argument("--modes", default="sum,mean,max", help="ragged / raggedfields: pooling modes to run")
    ap.add_argument("--fields", type=int, default=4, help="raggedfields: the number of multi-valued fields F")
    a = ap.parse_args()
    if a.what == "ragged":       # own inputs (ids + offsets, and the same bags padded): not part of "all"
        return bench_ragged(a)
    if a.what == "raggedfields":  # own inputs and modules: not part of "all"
        return bench_raggedfields(a)
    if a.what == "raggedattn":   # own inputs and modules: not part of "all"
        return bench_raggedattn(a)
    if a.what == "bagshard":     # own inputs and modules: not part of "all"
        return bench_bagshard(a)
    if a.what == "rank":        # own inputs and modules: not part of "all"
        return bench_rank(a)
    if a.what == "seq":          # own inputs and module: not part of "all"
        return bench_seq(a)
    if a.what == "routing":      # own inputs and module: not part of "all"
        return bench_routing(a)
    if a.what == "compact":      # own inputs (a 125 M-row table and its Adagrad state): not part of "all"
        return bench_compact(a)
    if a.what == "rowwise":      # own inputs (one table and state per optimizer): not part of "all"
        return bench_rowwise(a)
    if a.what == "bag":          # own inputs (a 4 GiB table is generated on the device): not part of "all"
        return bench_bag(a)
    if a.what == "attn":         # own inputs and module: not part of "all"
        return bench_attn(a)
    if a.what == "prm":          # own inputs and modules: not part of "all"; the list and head defaults of the paper
        a.L = a.L if any(v.startswith("--L") for v in sys.argv) else 30
        a.H = a.H if any(v.startswith("--H") for v in sys.argv) else 4
        return bench_prm(a)
    if a.what == "senet":        # own inputs and modules: not part of "all"
        return bench_senet(a)
    if a.what == "moe":          # own inputs and modules: not part of "all"
        return bench_moe(a)
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    s = 2 if dt == torch.bfloat16 else 4
    dev = torch.device("cuda:0")
    B, N, E, V = a.B, a.N, a.E, a.V
    g = torch.Generator().manual_seed(1234)
    per = V // N
    fs = [per] * (N - 1) + [V - per * (N - 1)]
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.tensor(fs), 0)[:-1]]).to(dev)
    if a.zipf:
        cols = []
        for f in fs:
            r = torch.rand(B, 1, generator=g, dtype=torch.float64)
            # Zipf(1.05)-like via inverse power transform
            cols.append(((f ** r - 1).clamp_(0, f - 1)).long())
        idx = torch.cat(cols, 1).to(dev)
    else:
        idx = torch.cat([torch.randint(0, f, (B, 1), generator=g) for f in fs], 1).to(dev)
    w = torch.randn(V, E, generator=g).to(dt).to(dev)
    w1 = torch.randn(V, 1, generator=g).to(dt).to(dev)
    what = a.what.split(",")

    def want(k):
        return "all" in what or k in what

    def report(name, t, nbytes):
        print(f"{name:34s} med {t[0]*1e6:9.1f} us  min {t[1]*1e6:9.1f} us  {nbytes/t[0]/1e9:8.1f} GB/s (alg) "
              f"{nbytes/t[0]/8e12*100:5.1f}% of 8TB/s", flush=True)

    rd = B * N * (8 + E * s)
    if want("gather"):
        t = timeit(lambda: F_._GatherRows.apply(w, idx, off, None))
        report("gather_rows", t, rd + B * N * E * s)
    if want("embed_fm"):
        t = timeit(lambda: F_._EmbedFM.apply(w, idx, off, None, False))
        report("embed_fm (fm only)", t, rd + B * E * s + B * E * 4)
        t = timeit(lambda: F_._EmbedFM.apply(w, idx, off, None, True))
        report("embed_fm (+emb block)", t, rd + B * N * E * s + B * E * s + B * E * 4)
        t = timeit(lambda: F_._EmbedFM.apply(w, idx, off, w1, True))
        report("embed_fm (+emb +first)", t, rd + B * N * s + B * N * E * s + B * E * s + B * E * 4)
        t = timeit(lambda: F_._EmbedFM.apply(w, idx, off, w1, False))
        report("embed_fm (fm+first, no block)", t, rd + B * N * s + B * E * s + B * E * 4)
    if want("fm"):
        x = torch.randn(B, N, E, generator=g).to(dt).to(dev)
        t = timeit(lambda: F_._FMLayer.apply(x))
        report("fm_fwd (block)", t, B * N * E * s + B * E * s + B * E * 4)
    if want("csr"):
        def csr():
            F_.clear_caches()
            return F_.row_buckets(idx, off, V)
        t = timeit(csr)
        report("csr_build", t, B * N * (8 + 4 + 4 + 4) + 2 * (V + 1) * 4 * 2)
    if want("scatter"):
        rb = F_.row_buckets(idx, off, V)
        ge = torch.randn(B, N, E, generator=g).to(dt).to(dev)
        gf = torch.randn(B, E, generator=g).to(dt).to(dev)
        S = torch.randn(B, E, generator=g).to(dev)
        t = timeit(lambda: F_.scatter_rows(rb, w, g_rows=ge))
        report("scatter_rows (g_rows)", t, B * N * (E * s + 4) + V * E * s + V * 4)
        t = timeit(lambda: F_.scatter_rows(rb, w, g_rows=ge, g_bcast=gf, fm_sum=S))
        report("scatter_rows (g_rows + fm)", t, B * N * (E * s + 4) + V * E * s * 2 + V * 4)
        g1 = gf[:, :1].contiguous()
        t = timeit(lambda: F_.scatter_rows(rb, w, g_rows=ge, g_bcast=g1, fm_sum=S))
        report("scatter_rows (g_rows + fm, g constant along E)", t, B * N * (E * s + 4) + V * E * s * 2 + V * 4)
        t = timeit(lambda: F_.scatter_rows(rb, w1, g_bcast=gf[:, :1].contiguous()))
        report("scatter_rows (first-order E=1)", t, B * N * (4) + V * s + V * 4)
    if want("cross"):
        L = 6
        x = (0.5 * torch.randn(B, N, E, generator=g)).to(dt).to(dev).requires_grad_()
        W = (torch.randn(L, E, E, generator=g) / E ** 0.5).to(dt).to(dev).requires_grad_()
        bb = (0.1 * torch.randn(L, E, generator=g)).to(dt).to(dev).requires_grad_()
        t = timeit(lambda: F_._Cross.apply(x.detach(), W.detach(), bb.detach(), True), iters=5, warm=1)
        report(f"cross_fwd L={L}", t, 2 * B * N * E * s)
        print(f"    -> {2*B*N*E*E*L/t[0]/1e12:.1f} TFLOP/s")
        y = F_._Cross.apply(x, W, bb, True)
        gy = torch.randn_like(y)
        t = timeit(lambda: torch.autograd.grad(y, (x, W, bb), gy, retain_graph=True), iters=3, warm=1)
        report(f"cross_bwd L={L}", t, 3 * B * N * E * s)
    if want("ipn"):
        x = torch.randn(B, N, E, generator=g).to(dt).to(dev).requires_grad_()
        t = timeit(lambda: F_._PairDot.apply(x.detach()), iters=10)
        report("pair_dot_fwd", t, B * N * E * s + B * (N * (N - 1) // 2) * s)
        y = F_._PairDot.apply(x)
        gy = torch.randn_like(y)
        t = timeit(lambda: torch.autograd.grad(y, x, gy, retain_graph=True), iters=10)
        report("pair_dot_bwd", t, 2 * B * N * E * s + B * (N * (N - 1) // 2) * s)
        Pn = N * (N - 1) // 2
        with torch.no_grad():
            t = timeit(lambda: F_.gather_rows(w, idx, off), iters=10)
            t2 = timeit(lambda: F_.embed_ipn(w, idx, off, want_emb=True), iters=10)
            report("gather_rows alone (for comparison)", t, B * N * (8 + 2 * E * s))
            report("embed_ipn (lookup + inner products, block written)", t2, B * N * (8 + 2 * E * s) + B * Pn * s)
            t3 = timeit(lambda: F_.embed_ipn(w, idx, off, want_emb=False), iters=10)
            report("embed_ipn (no block: inference)", t3, B * N * (8 + E * s) + B * Pn * s)
    if want("pairx"):
        from torecsys_amd.layers import (AttentionalFactorizationMachineLayer, BilinearInteractionLayer,
                                         OuterProductNetworkLayer)
        P = N * (N - 1) // 2
        Bp = a.B // 8 if a.B >= 8192 else a.B          # the (B,NC2,E) outputs are 6.2 GB at B = 65536
        x = (0.5 * torch.randn(Bp, N, E, generator=g)).to(dt).to(dev).requires_grad_()
        fl_bil = 2.0 * Bp * P * E * E

        def run(name, lay, out_elems, flops):
            lay = lay.to(dev).to(dt)
            f = lambda: lay(x.detach())
            t = timeit(f, iters=3, warm=1)
            yb = out_elems * s + Bp * N * E * s
            print(f"{name:34s} fwd med {t[0]*1e6:9.1f} us  {yb/t[0]/1e9:7.1f} GB/s (alg)  {flops/t[0]/1e12:7.1f} TFLOP/s",
                  flush=True)
            y = lay(x)
            y = y[0] if isinstance(y, tuple) else y
            gy = torch.randn_like(y.rename(None))
            ins = (x,) + tuple(lay.parameters())
            t = timeit(lambda: torch.autograd.grad(y.rename(None), ins, gy, retain_graph=True), iters=3, warm=1)
            print(f"{'':34s} bwd med {t[0]*1e6:9.1f} us  {2*flops/t[0]/1e12:7.1f} TFLOP/s", flush=True)

        print(f"pair layers at B={Bp} N={N} E={E}")
        run("opn vec", OuterProductNetworkLayer(E, N, "vec"), Bp * P, 3.0 * Bp * P * E)
        run("opn num", OuterProductNetworkLayer(E, N, "num"), Bp * P, 2.0 * Bp * P * E)
        run("opn mat", OuterProductNetworkLayer(E, N, "mat"), Bp * P, fl_bil)
        run("bilinear all", BilinearInteractionLayer(E, N, "all"), Bp * P * E, 2.0 * Bp * N * E * E)
        run("bilinear each", BilinearInteractionLayer(E, N, "each"), Bp * P * E, fl_bil)
        run("afm A=64", AttentionalFactorizationMachineLayer(E, N, 64, 0.0), Bp * E + Bp * P, 2.0 * Bp * P * E * 64)
    if want("cin"):
        Bc = a.B // 8 if a.B >= 8192 else a.B
        import os as _os
        only = _os.environ.get("TRS_KB_CIN_H")
        for (H, C) in ((39, 256), (128, 256)):
            if only and int(only) != H:
                continue
            ld0 = ((N + 31) // 32) * 32
            x0T = torch.zeros(Bc, E, ld0, dtype=dt, device=dev)
            x0T[:, :, :N] = (0.5 * torch.randn(Bc, E, N, generator=g)).to(dt).to(dev)
            xkT = x0T if H == N else (0.5 * torch.randn(Bc, E, H, generator=g)).to(dt).to(dev)
            W = (torch.randn(C, N * H, generator=g) / (N * H) ** 0.5).to(dt).to(dev)
            bias = torch.zeros(C, dtype=dt, device=dev)
            t = timeit(lambda: F_._CINContractCL.apply(x0T, xkT, W, bias, N, H), iters=5, warm=1)
            fl = 2.0 * Bc * E * C * N * (H + 1)
            print(f"cin_cl_fwd B={Bc} N={N} H={H} C={C}: med {t[0]*1e3:.3f} ms  {fl/t[0]/1e12:.1f} TFLOP/s "
                  f"({fl/t[0]/2.5e15*100:.1f}% of 2.5 PF)", flush=True)
            x0r, xkr, Wr = x0T.clone().requires_grad_(), (None if H == N else xkT.clone().requires_grad_()), W.clone().requires_grad_()
            yT = F_._CINContractCL.apply(x0r, x0r if H == N else xkr, Wr, bias, N, H)
            gy = torch.randn_like(yT)
            ins = (x0r, Wr) if H == N else (x0r, xkr, Wr)
            t = timeit(lambda: torch.autograd.grad(yT, ins, gy, retain_graph=True), iters=3, warm=1)
            print(f"cin_cl_bwd (data+dW+transposes): med {t[0]*1e3:.3f} ms  {2*fl/t[0]/1e12:.1f} TFLOP/s", flush=True)
            t = timeit(lambda: torch.autograd.grad(yT, ins[:-1], gy, retain_graph=True), iters=5, warm=1)
            print(f"cin_cl_bwd data only H={H}: med {t[0]*1e3:.3f} ms  {fl/t[0]/1e12:.1f} TFLOP/s", flush=True)
            t = timeit(lambda: torch.autograd.grad(yT, ins[-1:], gy, retain_graph=True), iters=5, warm=1)
            print(f"cin_cl_bwd dW only (+transposes) H={H}: med {t[0]*1e3:.3f} ms  {fl/t[0]/1e12:.1f} TFLOP/s", flush=True)
    if want("mlp"):
        C = 400
        gy = torch.randn(B, C, generator=g).to(dt).to(dev)
        yy = torch.relu(torch.randn(B, C, generator=g)).to(dt).to(dev)
        t = timeit(lambda: F_.relu_bwd_bias(gy, yy))
        report("relu_bwd_bias (fused)", t, 3 * B * C * s)
        def aten():
            gz = torch.ops.aten.threshold_backward(gy, yy, 0)
            return gz, gz.sum(0)
        t = timeit(aten)
        report("ATen threshold_backward + sum", t, 4 * B * C * s)
    if want("mlpf"):
        rows_ = B * N
        widths = [64, 400, 400, 400, 64]
        Ws = [(torch.randn(o, i, generator=g) / i ** 0.5).to(dt).to(dev).requires_grad_() for i, o in zip(widths[:-1], widths[1:])]
        bs = [(0.1 * torch.randn(o, generator=g)).to(dt).to(dev).requires_grad_() for o in widths[1:]]
        xx = torch.randn(rows_, 64, generator=g).to(dt).to(dev).requires_grad_()
        fl = 2.0 * rows_ * sum(i * o for i, o in zip(widths[:-1], widths[1:]))
        t = timeit(lambda: F_.fused_mlp(xx.detach(), [w.detach() for w in Ws], [b_.detach() for b_ in bs]), iters=5, warm=1)
        print(f"fused MLP fwd  rows={rows_} {widths}: med {t[0]*1e3:.3f} ms  {fl/t[0]/1e12:.1f} TFLOP/s", flush=True)
        y = F_.fused_mlp(xx, Ws, bs)
        gy = torch.randn_like(y)
        t = timeit(lambda: torch.autograd.grad(y, (xx,), gy, retain_graph=True), iters=5, warm=1)
        print(f"fused MLP bwd (data only): med {t[0]*1e3:.3f} ms  {fl/t[0]/1e12:.1f} TFLOP/s", flush=True)
        t = timeit(lambda: torch.autograd.grad(y, (xx, *Ws, *bs), gy, retain_graph=True), iters=3, warm=1)
        print(f"fused MLP bwd (data + weight gradients): med {t[0]*1e3:.3f} ms  {2*fl/t[0]/1e12:.1f} TFLOP/s", flush=True)
    if want("mlpf") or want("wgrad"):
        # dW = g^T x over the rows: the hand-written kernel against the batched library GEMM it replaces
        for rows_, M_, N_ in [(B * N, 416, 416), (B * N, 416, 64), (B * N, 64, 416), (B, 416, 416), (B, 416, 2496)]:
            gg = torch.randn(rows_, M_, generator=g).to(dt).to(dev)
            xx2 = torch.randn(rows_, N_, generator=g).to(dt).to(dev)
            fl = 2.0 * rows_ * M_ * N_
            by = (M_ + N_) * 2.0 * rows_
            for on in (True, False):
                F_.WGRAD_ROWS = on
                t = timeit(lambda: F_._wgrad_rows(gg, xx2, M_, N_, dt), iters=5, warm=2)
                print(f"wgrad {'trs_wgrad_rows' if on else 'bmm split-K  '} rows={rows_} {M_}x{N_}: med {t[0]*1e6:8.1f} us  "
                      f"{fl/t[0]/1e12:6.1f} TFLOP/s  {by/t[0]/1e9:7.1f} GB/s (operands once)", flush=True)
            F_.WGRAD_ROWS = True
            del gg, xx2
    if "ffm" in what:         # (not part of "all": 5 GB of tables + 12.8 GB + 6.2 GB tensors at the BASELINE shape)
        # the fused field-aware lookup + FFM reads B*N*8 + B*N*N*E*s (12.8 GB at S) and writes B*NC2*E*s (6.2 GB)
        P = N * (N - 1) // 2
        tabs = [(torch.rand(V, E, generator=g) - 0.5).to(dt).to(dev) for _ in range(N)]
        rd_fa = B * N * 8 + B * N * N * E * s
        with torch.no_grad():
            t = timeit(lambda: F_.fa_gather_rows(tabs, idx, off), iters=5, warm=1)
            report("fa_gather_rows (B,N*N,E)", t, rd_fa + B * N * N * E * s)
            xfa = F_.fa_gather_rows(tabs, idx, off)
            t = timeit(lambda: F_.ffm_layer(xfa, N), iters=5, warm=1)
            report("ffm_fwd on the materialised block", t, 2 * B * P * E * s + B * P * E * s)
            t = timeit(lambda: F_.ffm_fused(tabs, idx, off), iters=5, warm=1)
            report("ffm_fused_fwd (lookup + FFM)", t, rd_fa + B * P * E * s)
            print(f"    -> SURVEY 8d bytes {(rd_fa + B * P * E * s) / 1e9:.2f} GB; 8 TB/s floor "
                  f"{(rd_fa + B * P * E * s) / 8e12 * 1e3:.2f} ms", flush=True)
        xr = xfa.detach().requires_grad_()
        y = F_.ffm_layer(xr, N)
        gy = torch.randn(B, P, E, dtype=dt, device=dev)
        t = timeit(lambda: torch.autograd.grad(y, xr, gy, retain_graph=True), iters=3, warm=1)
        report("ffm_bwd on the materialised block", t, 3 * B * P * E * s + B * N * N * E * s)
        del y, xr, xfa
        tr = [w_.requires_grad_() for w_ in tabs]
        y = F_.ffm_fused(tr, idx, off)
        t = timeit(lambda: torch.autograd.grad(y, tr, gy, retain_graph=True), iters=3, warm=1)
        report("ffm_fused_bwd (all N table grads)", t, 2 * B * N * N * E * s // 1 + N * V * E * s)
        del y, gy, tr, tabs
    if want("copy"):
        x = torch.empty(512 * 1024 * 1024 // 4, dtype=torch.float32, device=dev)
        y = torch.empty_like(x)
        t = timeit(lambda: y.copy_(x))
        report("torch copy 512MB (r+w)", t, 2 * x.numel() * 4)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the collapsed Gibbs engine (pylda_gibbs_sweep) on the corpus of bench.py's cfg 3 (synth100k), one GPU.
Prints ONE JSON line (with --sharded RCCL writes its start-up banner to standard output ahead of it: the record is the
last line; --output FILE writes the JSON line alone to a file as well).

    python tools/gibbs_bench.py [--warmup 2] [--steps 5] [--workloads synth100k] [--blocks 1,16,64] [--docs N] [--sharded] [--output FILE]

Per workload and number of blocks: ms per sweep (wall time of `steps` enqueued sweeps and one wait), token-steps/s, the
device time of the sweep's kernels (profiling bracket around the rounds), the kernel launches a sweep makes, and the log
posterior after the timed sweeps.  The chain goes on from one setting to the next (the timings do not depend on where it
is).  The yardstick is the hybrid sampler's per-sweep time of tools/hybrid_bench.py taken in the same session.

--sharded adds, per number of blocks, the same sweeps through the sharded path in a world of ONE
rank over RCCL: round_sample, the all-gather on the library's buffers, round_apply.  Against pylda_gibbs_sweep in the same
run that is the fixed price of the sharded path - the pack kernel, the apply pass over every token's record and two more
launches per round - not scaling: "sharded" holds ms per sweep, the device time of the sampler, and of the pack and
record-apply kernels together."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sharded_sweeps(ctx, corpus, group, alpha, beta, blocks, warmup, steps, stream):
    """(ms per sweep, sampler ms per sweep, pack + record-apply ms per sweep, last stream) of the sharded path."""
    from pylda_amd import distributed
    rounds = max(1, min(blocks, corpus.D))
    capacity = ctx.gibbs_round_tokens(corpus, rounds, 0)
    send, recv = ctx.gibbs_exchange_prepare(corpus, rounds, 0, 1, 0, capacity)

    def sweep(stream):
        for g in range(rounds):
            if capacity[g] == 0:
                continue
            ctx.gibbs_round_sample(corpus, alpha, beta, rounds, g, 1, stream, 0)
            distributed.allgather_gibbs_records(ctx, send, recv, capacity[g], group)
            ctx.gibbs_round_apply(corpus, g)
    for _ in range(warmup):
        stream += 1
        sweep(stream)
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.kernel_time()
    t0 = time.perf_counter()
    for _ in range(steps):
        stream += 1
        sweep(stream)
    ctx.synchronize()
    wall = (time.perf_counter() - t0) / steps
    sampler_ms, exchange_ms, _ = ctx.kernel_time()
    ctx.set_profiling(False)
    return wall * 1e3, sampler_ms / steps, exchange_ms / steps, stream


def run(name, warmup, steps, docs, blocks_list, sharded=False):
    import bench
    from pylda_amd import _capi
    wl = bench.build_workload(name, 0, 1, 0, docs)
    ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
    D = len(ptr) - 1
    tokens = int(np.sum(cts, dtype=np.int64))
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    ctx = _capi.Context(K, V)
    group = None
    if sharded:
        import torch
        import torch.distributed as dist
        from pylda_amd import distributed
        if not dist.is_initialized():
            import socket
            probe = socket.socket()                          # a free port: the rendezvous of this one-rank world
            probe.bind(("127.0.0.1", 0))
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(probe.getsockname()[1]))
            probe.close()
        torch.cuda.set_device(0)
        if not dist.is_initialized():
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        group = dist.group.WORLD
        distributed.bind_to_torch_stream(ctx)
    corpus = ctx.corpus(ptr, ids, cts)
    t0 = time.perf_counter()
    ctx.gibbs_init(corpus, 1)
    ctx.synchronize()
    out = {"workload": name, "cfg": wl.get("cfg"), "documents": D, "nnz": int(len(ids)), "tokens": tokens, "K": K, "V": V,
           "init_ms": (time.perf_counter() - t0) * 1e3, "log_posterior_start": ctx.gibbs_log_posterior(corpus, alpha, beta),
           "blocks": []}
    stream = 0
    for blocks in blocks_list:
        for _ in range(warmup):
            stream += 1
            ctx.gibbs_sweep(corpus, alpha, beta, blocks, 1, stream)
        ctx.synchronize()
        ctx.set_profiling(True)
        ctx.kernel_time()
        t0 = time.perf_counter()
        for _ in range(steps):
            stream += 1
            ctx.gibbs_sweep(corpus, alpha, beta, blocks, 1, stream)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) / steps
        kernel_ms, _, _ = ctx.kernel_time()
        ctx.set_profiling(False)
        t1 = time.perf_counter()
        lp = ctx.gibbs_log_posterior(corpus, alpha, beta)
        out["blocks"].append({"blocks": blocks, "ms_per_sweep": wall * 1e3, "token_steps_per_s": tokens / wall,
                              "kernels_ms_per_sweep": kernel_ms / steps, "launches_per_sweep": 2 * min(blocks, D),
                              "log_posterior": lp, "log_posterior_ms": (time.perf_counter() - t1) * 1e3})
        if sharded:
            ms, sampler_ms, exchange_ms, stream = sharded_sweeps(ctx, corpus, group, alpha, beta, blocks, warmup, steps, stream)
            out["blocks"][-1]["sharded"] = {"world": 1, "backend": "nccl", "ms_per_sweep": ms, "sampler_ms_per_sweep": sampler_ms,
                                            "pack_and_record_apply_ms_per_sweep": exchange_ms,
                                            "launches_per_sweep": 3 * min(blocks, D), "collectives_per_sweep": min(blocks, D),
                                            "log_posterior": ctx.gibbs_log_posterior(corpus, alpha, beta)}
    corpus.close()
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--workloads", default="synth100k")
    ap.add_argument("--blocks", default="1,16,64")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sharded", action="store_true")
    ap.add_argument("--output", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    blocks = [int(b) for b in args.blocks.split(",")]
    out = {"tool": "gibbs_bench", "warmup": args.warmup, "steps": args.steps,
           "results": [run(w, args.warmup, args.steps, args.docs, blocks, args.sharded) for w in args.workloads.split(",")]}
    if args.sharded:
        import torch.distributed as dist
        dist.destroy_process_group()
    if args.output:
        with open(args.output, "w") as stream:
            stream.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

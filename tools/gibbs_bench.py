#!/usr/bin/env python3
"""Timing of the collapsed Gibbs engine (pylda_gibbs_sweep) on the corpus of bench.py's cfg 3 (synth100k), one GPU.
Prints ONE JSON line.

    python tools/gibbs_bench.py [--warmup 2] [--steps 5] [--workloads synth100k] [--blocks 1,16,64] [--docs N]

Per workload and number of blocks: ms per sweep (wall time of `steps` enqueued sweeps and one wait), token-steps/s, the
device time of the sweep's kernels (profiling bracket around the rounds), the kernel launches a sweep makes, and the log
posterior after the timed sweeps.  The chain goes on from one setting to the next (the timings do not depend on where it
is).  The yardstick is the hybrid sampler's per-sweep time of tools/hybrid_bench.py taken in the same session."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(name, warmup, steps, docs, blocks_list):
    import bench
    from pylda_amd import _capi
    wl = bench.build_workload(name, 0, 1, 0, docs)
    ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
    D = len(ptr) - 1
    tokens = int(np.sum(cts, dtype=np.int64))
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    ctx = _capi.Context(K, V)
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
    args = ap.parse_args(argv)
    blocks = [int(b) for b in args.blocks.split(",")]
    out = {"tool": "gibbs_bench", "warmup": args.warmup, "steps": args.steps,
           "results": [run(w, args.warmup, args.steps, args.docs, blocks) for w in args.workloads.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

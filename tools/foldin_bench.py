#!/usr/bin/env python3
"""Timing of the held-out fold-in (pylda_foldin) on the corpus of bench.py's cfg 3 (synth100k), one GPU.  Prints ONE JSON line.

    python tools/foldin_bench.py [--warmup 2] [--steps 5] [--samples 10] [--train 3] [--workloads synth100k] [--docs N]

The model is the corpus' own Gibbs state after `train` sweeps of 16 rounds; the same documents, uploaded as a corpus of their
own, are folded in: `steps` timed calls of `samples` sweeps each (burn-in samples // 2), every call with its start, its
likelihood and its one wait.  Reported: ms per call and per fold-in sweep (call / samples), token-steps/s, the device time
of the sampler (profiling bracket), the time of pylda_foldin_set_model.  The yardstick is a training sweep with one round
(G = 1) on the same corpus, timed here the way tools/gibbs_bench.py times it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(name, warmup, steps, samples, train, docs):
    import bench
    from pylda_amd import _capi
    wl = bench.build_workload(name, 0, 1, 0, docs)
    ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
    tokens = int(np.sum(cts, dtype=np.int64))
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    ctx = _capi.Context(K, V)
    trained = ctx.corpus(ptr, ids, cts)
    ctx.gibbs_init(trained, 1)
    stream = 0
    for _ in range(train):
        stream += 1
        ctx.gibbs_sweep(trained, alpha, beta, 16, 1, stream)
    for timed in (False, True):                 # the yardstick: a training sweep of one round
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps if timed else warmup):
            stream += 1
            ctx.gibbs_sweep(trained, alpha, beta, 1, 1, stream)
        ctx.synchronize()
        training_sweep = (time.perf_counter() - t0) / steps
    t0 = time.perf_counter()
    ctx.foldin_set_model(beta, trained=trained)
    set_model = time.perf_counter() - t0
    heldout = ctx.corpus(ptr, ids, cts)
    call = 0
    for _ in range(warmup):
        call += 1
        ctx.foldin(heldout, alpha, samples, samples // 2, 1, 2 ** 31 + call)
    ctx.set_profiling(True)
    ctx.kernel_time()
    t0 = time.perf_counter()
    for _ in range(steps):
        call += 1
        total = ctx.foldin(heldout, alpha, samples, samples // 2, 1, 2 ** 31 + call)
    wall = (time.perf_counter() - t0) / steps
    kernel_ms, _, _ = ctx.kernel_time()
    ctx.set_profiling(False)
    out = {"workload": name, "cfg": wl.get("cfg"), "documents": len(ptr) - 1, "nnz": int(len(ids)), "tokens": tokens, "K": K, "V": V,
           "samples": samples, "ms_per_call": wall * 1e3, "ms_per_sweep": wall * 1e3 / samples,
           "token_steps_per_s": tokens * samples / wall, "sampler_ms_per_call": kernel_ms / steps,
           "set_model_ms": set_model * 1e3, "training_sweep_g1_ms": training_sweep * 1e3,
           "words_log_likelihood_per_token": total / tokens}
    heldout.close()
    trained.close()
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--train", type=int, default=3)
    ap.add_argument("--workloads", default="synth100k")
    ap.add_argument("--docs", type=int, default=None)
    args = ap.parse_args(argv)
    out = {"tool": "foldin_bench", "warmup": args.warmup, "steps": args.steps,
           "results": [run(w, args.warmup, args.steps, args.samples, args.train, args.docs) for w in args.workloads.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

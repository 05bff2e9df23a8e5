#!/usr/bin/env python3
"""Timing of the left-to-right held-out likelihood (pylda_left_to_right) on the corpus of bench.py's cfg 3 (synth100k), one
GPU.  Prints ONE JSON line.

    python tools/ltr_bench.py [--warmup 2] [--steps 5] [--particles 4] [--train 3] [--workloads synth100k] [--docs N] [--step_budget B]

The model is built as tools/foldin_bench.py builds it: the corpus' own Gibbs state after `train` sweeps of 16 rounds, its
predictive table by pylda_foldin_set_model.  The same documents, uploaded as a corpus of their own, are scored with
`particles` particles, first without resampling (N_d token-steps per document and particle), then with it
(N_d (N_d - 1) / 2 + N_d): `steps` timed calls each, every call with its launches, its reduction and its one wait.  Reported
per mode: ms per call, token-steps/s, the device time of the kernels (profiling bracket).  The yardstick, in the same
session, is a fold-in sweep over the same corpus (10 sweeps a call, as tools/foldin_bench.py), whose token-step does the same
work - leave, K weights, scan, draw, enter - and `step_rate_over_fold_in` is the ratio of the two rates."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(name, warmup, steps, particles, train, docs, step_budget):
    import bench
    from pylda_amd import _capi
    wl = bench.build_workload(name, 0, 1, 0, docs)
    ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
    tokens = int(np.sum(cts, dtype=np.int64))
    n = np.diff(np.concatenate([[0], np.cumsum(cts, dtype=np.int64)])[np.asarray(ptr, dtype=np.int64)]).astype(np.float64)
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    ctx = _capi.Context(K, V)
    trained = ctx.corpus(ptr, ids, cts)
    ctx.gibbs_init(trained, 1)
    for sweep in range(train):
        ctx.gibbs_sweep(trained, alpha, beta, 16, 1, 1 + sweep)
    ctx.foldin_set_model(beta, trained=trained)
    heldout = ctx.corpus(ptr, ids, cts)
    out = {"workload": name, "cfg": wl.get("cfg"), "documents": len(ptr) - 1, "nnz": int(len(ids)), "tokens": tokens, "K": K, "V": V,
           "particles": particles, "step_budget": step_budget, "longest_document": int(n.max())}
    # the yardstick: fold-in sweeps
    samples, call = 10, 0
    for timed in (False, True):
        t0 = time.perf_counter()
        for _ in range(steps if timed else warmup):
            call += 1
            ctx.foldin(heldout, alpha, samples, samples // 2, 1, 2 ** 31 + call)
        fold_in = (time.perf_counter() - t0) / steps
    out["fold_in"] = {"samples": samples, "ms_per_sweep": fold_in * 1e3 / samples, "token_steps_per_s": tokens * samples / fold_in}
    call = 0
    for resample in (0, 1):
        token_steps = float(particles * np.sum(n * (n - 1) / 2 + n if resample else n))
        for _ in range(warmup):
            ctx.left_to_right(heldout, alpha, particles, resample, 1, (3 << 30) + 256 * call, 0, step_budget)
            call += 1
        ctx.set_profiling(True)
        ctx.kernel_time()
        t0 = time.perf_counter()
        for _ in range(steps):
            total, counted = ctx.left_to_right(heldout, alpha, particles, resample, 1, (3 << 30) + 256 * call, 0, step_budget)
            call += 1
        wall = (time.perf_counter() - t0) / steps
        kernel_ms, _, _ = ctx.kernel_time()
        ctx.set_profiling(False)
        assert counted == tokens
        rate = token_steps / wall
        out["resample_%d" % resample] = {"ms_per_call": wall * 1e3, "kernels_ms_per_call": kernel_ms / steps, "token_steps": token_steps,
                                         "token_steps_per_s": rate, "step_rate_over_fold_in": rate / out["fold_in"]["token_steps_per_s"],
                                         "log_likelihood_per_token": total / tokens}
    heldout.close()
    trained.close()
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--particles", type=int, default=4)
    ap.add_argument("--train", type=int, default=3)
    ap.add_argument("--workloads", default="synth100k")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--step_budget", type=int, default=0)
    args = ap.parse_args(argv)
    out = {"tool": "ltr_bench", "warmup": args.warmup, "steps": args.steps,
           "results": [run(w, args.warmup, args.steps, args.particles, args.train, args.docs, args.step_budget)
                       for w in args.workloads.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

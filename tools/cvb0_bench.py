#!/usr/bin/env python3
"""Timing of the collapsed variational Bayes engine (pylda_cvb0_*) on the corpus of bench.py's cfg 3 (synth100k), one GPU.
Prints ONE JSON line.

    python tools/cvb0_bench.py [--warmup 1] [--steps 3] [--blocks 1,16,64] [--workloads synth100k] [--docs N]

Per number of blocks G: ms per sweep (`steps` sweeps enqueued back to back, one wait at the end; the blocks' postings are
built by the warm-up sweep) and the rate the byte model implies - a sweep moves about five streams of nnz x stride x 8
bytes: g read and written, delta written and read, the rows of T gathered.  Then the likelihood pass (ms per call, its one
wait included) and the held-out fold-in over the same documents as a corpus of their own (10 sweeps a call, ms per sweep).
The yardsticks, taken in the same session on the same corpus: a collapsed Gibbs sweep of 16 rounds (pylda_gibbs_sweep) and
a hybrid iteration (Hybrid.learning, as tools/hybrid_bench.py times it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, warmup, steps, call):
    for _ in range(warmup):
        call()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    ctx.synchronize()
    return (time.perf_counter() - t0) / steps


def run(name, warmup, steps, blocks, docs, yardsticks):
    import bench
    from pylda_amd import _capi
    wl = bench.build_workload(name, 0, 1, 0, docs)
    ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
    tokens = int(np.sum(cts, dtype=np.int64))
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    ctx = _capi.Context(K, V)
    stride = int(ctx._lib.pylda_table_stride(ctx._h))
    stream_bytes = float(len(ids)) * stride * 8.0
    out = {"workload": name, "cfg": wl.get("cfg"), "documents": len(ptr) - 1, "nnz": int(len(ids)), "tokens": tokens, "K": K, "V": V,
           "table_stride": stride, "g_bytes": stream_bytes, "model_bytes_per_sweep": 5.0 * stream_bytes, "sweeps": {}}
    corpus = ctx.corpus(ptr, ids, cts)
    ctx.cvb0_init(corpus, 1)
    for G in blocks:
        t0 = time.perf_counter()
        ctx.cvb0_sweep(corpus, alpha, beta, G)         # (builds the blocks' postings on the host)
        ctx.synchronize()
        first = time.perf_counter() - t0
        wall = timed(ctx, warmup, steps, lambda: ctx.cvb0_sweep(corpus, alpha, beta, G))
        ll, change = ctx.cvb0_log_likelihood(corpus, alpha, beta)
        out["sweeps"][str(G)] = {"ms_per_sweep": wall * 1e3, "first_sweep_with_postings_ms": first * 1e3,
                                 "model_bytes_per_s": 5.0 * stream_bytes / wall, "log_likelihood_per_token": ll / tokens,
                                 "change_per_token": change / tokens}
    out["likelihood_ms_per_call"] = timed(ctx, 1, steps, lambda: ctx.cvb0_log_likelihood(corpus, alpha, beta)) * 1e3
    n_kv = ctx.cvb0_get_state(corpus, True, False)[0]
    ctx.set_eta(n_kv + beta[np.newaxis, :])
    ctx.completion_set_model()
    heldout = ctx.corpus(ptr, ids, cts)
    calls = [0]

    def fold():
        calls[0] += 1
        ctx.cvb0_foldin(heldout, alpha, 10, 1, 2 ** 31 + calls[0])
    out["fold_in"] = {"sweeps_per_call": 10, "ms_per_sweep": timed(ctx, 1, steps, fold) * 1e3 / 10}
    heldout.close()
    corpus.close()
    if yardsticks:
        gibbs = ctx.corpus(ptr, ids, cts)
        ctx.gibbs_init(gibbs, 1)
        sweep = [0]

        def gibbs_sweep():
            sweep[0] += 1
            ctx.gibbs_sweep(gibbs, alpha, beta, 16, 1, sweep[0])
        out["gibbs_sweep_16_blocks_ms"] = timed(ctx, warmup, steps, gibbs_sweep) * 1e3
        gibbs.close()
    ctx.close()
    if yardsticks:
        from pylda_amd.hybrid import Hybrid
        m = Hybrid(seed=1)
        m._verbose = False
        m._initialize_parsed(ptr, ids, cts, V, K, 1.0 / K, 1.0 / V, eta=np.random.default_rng(1).gamma(100.0, 0.01, (K, V)))
        out["hybrid_iteration_ms"] = timed(m._context(), warmup, steps, m.learning) * 1e3
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--blocks", default="1,16,64")
    ap.add_argument("--workloads", default="synth100k")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--yardsticks", type=int, default=1)
    args = ap.parse_args(argv)
    blocks = [int(b) for b in args.blocks.split(",")]
    out = {"tool": "cvb0_bench", "warmup": args.warmup, "steps": args.steps,
           "results": [run(w, args.warmup, args.steps, blocks, args.docs, bool(args.yardsticks)) for w in args.workloads.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

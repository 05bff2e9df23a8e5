#!/usr/bin/env python3
"""Timing of the hybrid engine (pylda_amd/hybrid.py): Hybrid.learning() on the corpora of bench.py's cfg 3 (synth100k)
and cfg 4 (synth1m), one GPU.  Prints ONE JSON line.

    python tools/hybrid_bench.py [--warmup 2] [--steps 5] [--workloads synth100k,synth1m] [--docs N]

Per workload: ms per outer iteration (hybrid E-step + device M-step + alpha update, the one host wait included),
documents/s, token-steps/s (tokens x number_of_samples per iteration), the sampler and statistics kernels' device time
(profiling brackets), the bytes the sampler gathers from the table (one row per distinct (document, term) pair and sweep)
and their rate, and the single-core rate of the numpy restatement (tests/hybrid_restatement.py) on a sample of the
corpus - the CPU statement of the same chain, not a tuned CPU sampler."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(name, warmup, steps, docs):
    import bench
    from pylda_amd.hybrid import Hybrid
    wl = bench.build_workload(name, 0, 1, 0, docs)
    ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
    D = len(ptr) - 1
    tokens = int(np.sum(cts, dtype=np.int64))
    eta = np.random.default_rng(1).gamma(100.0, 0.01, (K, V))
    m = Hybrid(seed=1)
    m._verbose = False
    m._initialize_parsed(ptr, ids, cts, V, K, 1.0 / K, 1.0 / V, eta=eta)
    for _ in range(warmup):
        m.learning()
    ctx = m._context()
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.kernel_time()
    t0 = time.perf_counter()
    lls = [m.learning() for _ in range(steps)]
    ctx.synchronize()
    wall = (time.perf_counter() - t0) / steps
    sampler_ms, stats_ms, calls = ctx.kernel_time()
    ctx.set_profiling(False)
    stride = int(ctx._lib.pylda_table_stride(ctx._h))
    samples = m._number_of_samples
    # one table row per distinct (document, term) pair and sweep: the c_n copies of a term reuse it
    gathered = float(len(ids)) * samples * min(stride, 64 * ((K + 63) // 64)) * 8.0
    # CPU restatement of the same chain on a sample of the documents (one core)
    import hybrid_restatement as spec
    from conftest import csr_slice
    sample = list(range(min(D, 200)))
    sp, si, sc = csr_slice(ptr, ids, cts, sample)
    t1 = time.perf_counter()
    spec.hybrid_estep(sp, si, sc, m._alpha_alpha, m._eta, 1, stream=1)
    cpu_s = time.perf_counter() - t1
    n = max(calls, 1)
    return {"workload": name, "cfg": wl.get("cfg"), "documents": D, "nnz": int(len(ids)), "tokens": tokens, "K": K, "V": V,
            "ms_per_iteration": wall * 1e3, "documents_per_s": D / wall, "token_steps_per_s": tokens * samples / wall,
            "sampler_kernel_ms": sampler_ms / n, "statistics_kernel_ms": stats_ms / n,
            "gathered_bytes": gathered, "gathered_GBps": gathered / (sampler_ms / n * 1e-3) / 1e9 if sampler_ms > 0 else None,
            "cpu_restatement_documents_per_s": len(sample) / cpu_s,
            "joint_log_likelihood_last": lls[-1]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--workloads", default="synth100k,synth1m")
    ap.add_argument("--docs", type=int, default=None)
    args = ap.parse_args(argv)
    out = {"tool": "hybrid_bench", "warmup": args.warmup, "steps": args.steps,
           "results": [run(w, args.warmup, args.steps, args.docs) for w in args.workloads.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the document-completion held-out likelihood on the corpus of bench.py's cfg 3 (synth100k), one GPU.  Prints ONE
JSON line.

    python tools/completion_bench.py [--warmup 2] [--steps 5] [--train 2] [--workloads synth100k] [--docs N]

The model is eta after `train` full-batch iterations (E-step, device M-step) from the usual random start; the same documents
are split into their observed and held halves (pylda_amd.corpus.split_for_completion) and uploaded as two corpora.  Timed, each
with `warmup` calls first and `steps` calls in the window, every call ending in its one wait:
    the held-out E-step on the observed halves (pylda_estep + pylda_estep_results),
    pylda_completion_set_model (+ a wait),
    pylda_completion_score from the observed corpus' device gamma; its kernel alone through the profiling bracket.
The byte model of the score kernel is the gathered rows, nnz_held x table stride x 8 bytes; reported: the achieved TB/s
of the kernel against it, and the score's share of the whole call (E-step + table + score)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

def _timed(call, wait, warmup, steps):
    for _ in range(warmup):
        call()
    wait()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    wait()
    return (time.perf_counter() - t0) / steps * 1e3


def run(name, warmup, steps, train, docs):
    import bench
    from pylda_amd import _capi
    from pylda_amd.corpus import split_for_completion
    wl = bench.build_workload(name, 0, 1, 0, docs)
    ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    ctx = _capi.Context(K, V)
    ctx.set_alpha(alpha)
    ctx.set_eta(np.random.default_rng(1).gamma(100.0, 0.01, (K, V)))
    trained = ctx.corpus(ptr, ids, cts)
    for _ in range(train):
        ctx.estep(trained, 50, 1e-6, False)
        ctx.mstep(trained, beta)
    trained.close()
    observed_csr, held_csr = split_for_completion(ptr, ids, cts)
    observed, held = ctx.corpus(*observed_csr), ctx.corpus(*held_csr)
    ldk = int(ctx._lib.pylda_table_stride(ctx._h))

    def estep():
        ctx.estep(observed, 50, 1e-6, True)
        ctx.estep_results(observed)
    estep_ms = _timed(estep, ctx.synchronize, warmup, steps)
    set_model_ms = _timed(lambda: (ctx.completion_set_model(), ctx.synchronize()), ctx.synchronize, warmup, steps)
    gathered = int(len(held_csr[1])) * ldk * 8
    out = {"workload": name, "cfg": wl.get("cfg"), "documents": len(ptr) - 1, "K": K, "V": V, "table_stride": ldk,
           "nnz_observed": int(len(observed_csr[1])), "nnz_held": int(len(held_csr[1])),
           "tokens_observed": int(np.sum(observed_csr[2], dtype=np.int64)), "tokens_held": int(np.sum(held_csr[2], dtype=np.int64)),
           "observed_estep_ms": estep_ms, "set_model_ms": set_model_ms, "gathered_bytes": gathered}
    result = []
    wall_ms = _timed(lambda: result.append(ctx.completion_score(held, observed=observed)), ctx.synchronize, warmup, steps)
    ctx.set_profiling(True)
    ctx.kernel_time()
    for _ in range(steps):
        ctx.completion_score(held, observed=observed)
    kernel_ms = ctx.kernel_time()[0] / steps
    ctx.set_profiling(False)
    total, tokens = result[-1]
    out["score"] = {"call_ms": wall_ms, "kernel_ms": kernel_ms, "achieved_tb_per_s": gathered / (kernel_ms * 1e-3) / 1e12,
                    "share_of_whole_call": wall_ms / (estep_ms + set_model_ms + wall_ms),
                    "held_log_likelihood": total, "held_tokens": tokens, "per_word_perplexity": float(np.exp(-total / tokens))}
    held.close()
    observed.close()
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--train", type=int, default=2)
    ap.add_argument("--workloads", default="synth100k")
    ap.add_argument("--docs", type=int, default=None)
    args = ap.parse_args(argv)
    out = {"tool": "completion_bench", "warmup": args.warmup, "steps": args.steps, "train": args.train,
           "results": [run(w, args.warmup, args.steps, args.train, args.docs) for w in args.workloads.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

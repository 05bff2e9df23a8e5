#!/usr/bin/env python3
"""Timing of stochastic collapsed variational Bayes (pylda_scvb_*) on the corpora of bench.py's cfg 3 (synth100k) and cfg 4
(synth1m), one GPU.  Prints ONE JSON line per workload and writes it to profiles/scvb_bench_<cfg>.json.

    python tools/scvb_bench.py [--workloads synth100k,synth1m] [--batches 16,64] [--burn_in 0,1] [--warmup 1] [--epochs 5]
                               [--docs N] [--cvb0 1] [--write 1]

Per number of minibatches B and burn_in P: the first epoch of a new B (the blocks' postings are built on the host in its
first step), then ms per epoch - B steps enqueued back to back, ONE wait at the end, the median of `epochs` epochs after
`warmup` - and ms per step (that median / B).  With --cvb0 1 (where the CVB0 rows fit) the CVB0 engine's sweep at the same
numbers of blocks, in the same session on the same corpus, as tools/cvb0_bench.py times it.  The device memory free before
the corpus, after the start and after the first epoch is recorded; a start that does not fit is recorded as such with the
library's message, not raised."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def free_bytes():
    """Free device memory as the runtime reports it (None where torch is missing)"""
    try:
        import torch
        return int(torch.cuda.mem_get_info(0)[0])
    except Exception:
        return None


def epoch(ctx, corpus, alpha, beta, tokens, batch_tokens, B, P, first_step, tau0=10.0, kappa=0.9):
    """B steps from step `first_step`, enqueued back to back; the parameters as StochasticCollapsedVariationalBayes forms them"""
    from pylda_amd.online_vb import step_size
    for t in range(first_step, first_step + B):
        b, e = t % B, t // B
        if batch_tokens[b] == 0:
            continue
        rho = step_size(tau0, kappa, t)
        rho_theta = [step_size(tau0, kappa, e * (P + 1) + p) for p in range(P + 1)]
        ctx.scvb_step(corpus, b, B, alpha, beta, 1.0 - rho, rho * (float(tokens) / float(batch_tokens[b])), rho_theta)


def run(name, batches, burn_ins, warmup, epochs, docs, cvb0):
    import bench
    from pylda_amd import _capi
    t0 = time.perf_counter()
    wl = bench.build_workload(name, 0, 1, 0, docs)
    built = time.perf_counter() - t0
    ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
    tokens = int(np.sum(cts, dtype=np.int64))
    offsets = np.concatenate([[0], np.cumsum(cts, dtype=np.int64)])
    doc_tokens = offsets[ptr[1:]] - offsets[ptr[:-1]]
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    ctx = _capi.Context(K, V)
    stride = int(ctx._lib.pylda_table_stride(ctx._h))
    D, nnz = len(ptr) - 1, int(len(ids))
    out = {"workload": name, "cfg": wl.get("cfg"), "documents": D, "nnz": nnz, "tokens": tokens, "K": K, "V": V, "table_stride": stride,
           "corpus_build_host_s": built, "cvb0_rows_bytes": float(nnz) * stride * 8.0,
           "state_bytes": {"table": float(V) * stride * 8.0, "n_dk": float(D) * K * 8.0}, "free_bytes": {"before_corpus": free_bytes()},
           "runs": {}}
    corpus = ctx.corpus(ptr, ids, cts)
    out["free_bytes"]["after_corpus"] = free_bytes()
    try:
        ctx.scvb_init(corpus, 1)
        ctx.synchronize()
        out["initialises"] = True
    except _capi.PyldaError as refused:
        out["initialises"] = False
        out["refusal"] = str(refused)
        corpus.close()
        ctx.close()
        return out
    out["free_bytes"]["after_start"] = free_bytes()
    ll, _ = ctx.cvb0_log_likelihood(corpus, alpha, beta)
    out["start_log_likelihood_per_token"] = ll / tokens
    for B in batches:
        batch_tokens = np.bincount(np.arange(D, dtype=np.int64) % B, weights=doc_tokens, minlength=B).astype(np.int64)
        batch_slots = np.bincount(np.arange(D, dtype=np.int64) % B, weights=np.diff(ptr), minlength=B)
        for P in burn_ins:
            ctx.scvb_init(corpus, 1)
            ctx.synchronize()
            t0 = time.perf_counter()
            epoch(ctx, corpus, alpha, beta, tokens, batch_tokens, B, P, 0)
            ctx.synchronize()
            first = time.perf_counter() - t0
            record = {"first_epoch_ms": first * 1e3, "first_epoch_builds_postings": bool(P == burn_ins[0]),
                      "free_bytes_after_first_epoch": free_bytes(),
                      "delta_rows_bytes": float(np.max(batch_slots)) * stride * 8.0}
            for e in range(1, 1 + warmup):
                epoch(ctx, corpus, alpha, beta, tokens, batch_tokens, B, P, e * B)
            ctx.synchronize()
            walls = []
            for e in range(1 + warmup, 1 + warmup + epochs):
                t0 = time.perf_counter()
                epoch(ctx, corpus, alpha, beta, tokens, batch_tokens, B, P, e * B)
                ctx.synchronize()
                walls.append(time.perf_counter() - t0)
            ll, change = ctx.cvb0_log_likelihood(corpus, alpha, beta)
            median = statistics.median(walls)
            record.update({"ms_per_epoch": median * 1e3, "ms_per_epoch_min": min(walls) * 1e3, "ms_per_epoch_max": max(walls) * 1e3,
                           "ms_per_step": median * 1e3 / B, "epochs_timed": epochs, "epochs_run": 1 + warmup + epochs,
                           "log_likelihood_per_token": ll / tokens, "change_per_token": change / tokens})
            out["runs"]["B=%d,burn_in=%d" % (B, P)] = record
            print("# %s B=%d burn_in=%d: first epoch %.1f ms, then %.2f ms per epoch" % (name, B, P, first * 1e3, median * 1e3),
                  file=sys.stderr, flush=True)
    out["likelihood_ms_per_call"] = statistics.median(_timed_calls(ctx, 3, lambda: ctx.cvb0_log_likelihood(corpus, alpha, beta))) * 1e3
    corpus.close()
    if cvb0:
        out["cvb0_sweeps"] = {}
        try:
            other = ctx.corpus(ptr, ids, cts)
            ctx.cvb0_init(other, 1)
            for G in batches:
                ctx.cvb0_sweep(other, alpha, beta, G)          # (builds the blocks' postings on the host)
                for _ in range(warmup):
                    ctx.cvb0_sweep(other, alpha, beta, G)
                ctx.synchronize()
                walls = _timed_calls(ctx, epochs, lambda: ctx.cvb0_sweep(other, alpha, beta, G))
                out["cvb0_sweeps"][str(G)] = {"ms_per_sweep": statistics.median(walls) * 1e3, "sweeps_timed": epochs}
            other.close()
        except _capi.PyldaError as refused:
            out["cvb0_sweeps"]["refusal"] = str(refused)
    ctx.close()
    return out


def _timed_calls(ctx, n, call):
    walls = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        walls.append(time.perf_counter() - t0)
    return walls


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="synth100k")
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--burn_in", default="0,1")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--cvb0", type=int, default=1)
    ap.add_argument("--write", type=int, default=1)
    args = ap.parse_args(argv)
    batches = [int(b) for b in args.batches.split(",")]
    burn_ins = [int(p) for p in args.burn_in.split(",")]
    for name in args.workloads.split(","):
        result = run(name, batches, burn_ins, args.warmup, args.epochs, args.docs, bool(args.cvb0))
        out = {"tool": "scvb_bench", "warmup": args.warmup, "epochs": args.epochs, "result": result}
        line = json.dumps(out)
        print(line, flush=True)
        if args.write and args.docs is None and result.get("cfg"):
            with open(os.path.join(ROOT, "profiles", "scvb_bench_%s.json" % result["cfg"]), "w") as stream:
                stream.write(line + "\n")


if __name__ == "__main__":
    main()

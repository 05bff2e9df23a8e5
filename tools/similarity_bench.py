#!/usr/bin/env python3
"""Timing of the nearest-documents pass at the size of bench.py's cfg 3 - 100k documents, K = 128 - on
one GPU.  Prints ONE JSON line.

    python tools/similarity_bench.py [--warmup 1] [--steps 3] [--docs 100000] [--topics 128] [--queries 10000,1] [--top 10]
                                     [--all_pairs 1] [--host_queries 200]

The rows are rng.gamma(0.1) + 0.01, the shape a trained gamma has (a few large entries over a floor); base and queries are
scored as sqrt(theta) (transform 2, the Hellinger affinity), the queries being the first Q rows of the base, each left out
of its own list.  Timed per Q, each with `warmup` calls first and `steps` calls in the window:
    pylda_similar_documents          the call (upload of the queries, kernels, read-back, one wait), and its kernels alone
                                     (profiling brackets: transform + top-N, and the merge)
Reported: fp64 multiply and add instructions per second of the top-N pass (2 Q D K per call) against the vector fp64 rate
(bench.FP64_VECTOR_PEAK_TFLOPS counts an FMA as two operations: the same number of instructions per second is half of it).
--all_pairs 1 adds ONE call with every document as a query.
Yardsticks, the same problem on the same rows (transformed by numpy once, outside the window):
    torch     a chunked fp64 matmul (the matrix unit, through rocBLAS) + topk on the same GPU, queries and base resident;
              the ids are compared with the device's (they may differ where two scores differ in the last bits)
    numpy     a chunked product + argpartition + sort on this host, on --host_queries queries, scaled to Q"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(call, warmup, steps):
    """every call ends in its own wait"""
    for _ in range(warmup):
        call()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    return (time.perf_counter() - t0) / steps * 1e3


def _torch_yardstick(base_t, queries_t, self_ids, N, warmup, steps, chunk=2048):
    import torch
    device = torch.device("cuda", 0)
    b = torch.from_numpy(base_t).to(device)
    a = torch.from_numpy(queries_t).to(device)
    own = torch.from_numpy(self_ids.astype(np.int64)).to(device)

    def call():
        ids = []
        for q0 in range(0, len(a), chunk):
            score = a[q0:q0 + chunk] @ b.T
            score[torch.arange(len(score), device=device), own[q0:q0 + chunk]] = -float("inf")
            ids.append(torch.topk(score, N, dim=1).indices)
        out = torch.cat(ids)
        torch.cuda.synchronize()
        return out
    ms = _timed(call, warmup, steps)
    return ms, call().cpu().numpy()


def _numpy_yardstick(base_t, queries_t, self_ids, N, chunk=50):
    t0 = time.perf_counter()
    for q0 in range(0, len(queries_t), chunk):
        score = queries_t[q0:q0 + chunk] @ base_t.T
        score[np.arange(len(score)), self_ids[q0:q0 + chunk]] = -np.inf
        part = np.argpartition(-score, N, axis=1)[:, :N]
        np.take_along_axis(part, np.argsort(-np.take_along_axis(score, part, axis=1), axis=1), axis=1)
    return (time.perf_counter() - t0) * 1e3


def run(args):
    import bench
    from pylda_amd import _capi
    D, K, N = args.docs, args.topics, args.top
    rng = np.random.default_rng(18)
    base = rng.gamma(0.1, size=(D, K)) + 0.01
    theta = base / base.sum(axis=1)[:, None]
    base_t = np.sqrt(theta)
    ctx = _capi.Context(K, 8)
    out = {"documents": D, "K": K, "top": N, "compute_units": ctx.compute_units(),
           "fp64_vector_peak_tflops": bench.FP64_VECTOR_PEAK_TFLOPS, "by_queries": {}}
    out["set_base_call_ms"] = _timed(lambda: ctx.similarity_set_base(base, 2), 1, 2)
    sizes = [int(q) for q in args.queries.split(",")] + ([D] if args.all_pairs else [])
    for i, Q in enumerate(sizes):
        whole = args.all_pairs and i == len(sizes) - 1
        warmup, steps = (0, 1) if whole else (args.warmup, args.steps)
        queries, own = base[:Q], np.arange(Q, dtype=np.int32)
        call_ms = _timed(lambda: ctx.similar_documents(queries, N, 2, own), warmup, steps)
        ctx.set_profiling(True)
        ctx.kernel_time()
        for _ in range(steps):
            ids, scores = ctx.similar_documents(queries, N, 2, own)
        topn_ms, merge_ms, _ = ctx.kernel_time()
        ctx.set_profiling(False)
        topn_ms, merge_ms = topn_ms / steps, merge_ms / steps
        instructions = 2.0 * Q * D * K
        rate = instructions / (topn_ms * 1e-3)
        entry = {"call_ms": call_ms, "transform_and_topn_kernel_ms": topn_ms, "merge_kernel_ms": merge_ms,
                 "multiply_and_add_instructions": instructions, "instructions_per_s": rate,
                 "fraction_of_vector_fp64_instruction_rate": rate / (bench.FP64_VECTOR_PEAK_TFLOPS * 1e12 / 2),
                 "mean_nearest_hellinger": float(np.mean(np.sqrt(np.maximum(0.0, 1.0 - scores[:, 0]))))}
        if not whole:
            torch_ms, torch_ids = _torch_yardstick(base_t, base_t[:Q], own, N, warmup, steps)
            host_q = min(Q, args.host_queries)
            numpy_ms = _numpy_yardstick(base_t, base_t[:host_q], own[:host_q], N)
            entry["torch_matmul_topk"] = {"ms": torch_ms, "rows_with_the_same_ids": float(np.mean(np.all(torch_ids == ids, axis=1))),
                                          "ratio_to_device_call": torch_ms / call_ms}
            entry["numpy_host"] = {"queries_timed": host_q, "ms": numpy_ms, "ms_scaled_to_Q": numpy_ms * Q / host_q,
                                   "ratio_to_device_call": numpy_ms * Q / host_q / call_ms}
        out["by_queries"][str(Q)] = entry
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--docs", type=int, default=100000)
    ap.add_argument("--topics", type=int, default=128)
    ap.add_argument("--queries", default="10000,1")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--all_pairs", type=int, default=0)
    ap.add_argument("--host_queries", type=int, default=200)
    args = ap.parse_args(argv)
    out = {"tool": "similarity_bench", "warmup": args.warmup, "steps": args.steps, "results": [run(args)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

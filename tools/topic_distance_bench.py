#!/usr/bin/env python3
"""Timing of the topic distances on one GPU: a model against itself at the table of bench.py's cfg 3
(K = 128, V = 50 000) and at K = 1024, V = 100 000, both metrics.  Prints ONE JSON line.

    python tools/topic_distance_bench.py [--warmup 1] [--steps 3] [--window_ms 500] [--shapes 128x50000,1024x100000] [--host_rows 2]
                                         [--host_full_below 1000000000]

The table is rng.gamma(0.05) + 1e-3 per entry, the shape a trained eta has (a few large entries over a floor).  Timed per
shape and metric, each with `warmup` calls first and then at least `steps` calls and `window_ms` of them in the window:
    pylda_topic_distances     the call (upload, transform, pair sums, read-back, one wait), and its kernels alone (profiling
                              brackets: the transform, and the pair sums with their combine)
Reported: pair-words per second of the pair pass, counting the K K V of the whole matrix (the pass computes the tiles on
or above the diagonal only: tile_pair_words is what it really walks), and for hellinger the multiply and add instructions
per second against the vector fp64 rate (bench.FP64_VECTOR_PEAK_TFLOPS counts an FMA as two operations: the same number
of instructions per second is half of it).  For jensen_shannon the figure is logs per second; the fraction of the fp64
rate follows from the instructions a pair-word costs, counted in the kernel's code.
Yardstick: the same formula in vectorised numpy on this host, on the whole matrix where it has at most --host_full_below
pair-words, else on the first --host_rows rows of a against all of b, scaled to K rows.  The device's numbers are compared
with the host's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = (("hellinger", 0), ("jensen_shannon", 1))


def _timed(call, warmup, steps, window_ms):
    """(ms per call, calls timed): every call ends in its own wait; at least `steps` calls and `window_ms` of them"""
    for _ in range(warmup):
        call()
    t0 = time.perf_counter()
    call()
    one_ms = (time.perf_counter() - t0) * 1e3
    steps = int(min(500, max(steps, np.ceil(window_ms / max(one_ms, 1e-3)))))
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    return (time.perf_counter() - t0) / steps * 1e3, steps


def _host_rows(table, rows, metric):
    """(transform ms, rows ms, values (rows, K)): the first `rows` rows of the table against all of it, the device's formula
    in numpy; the transform of the whole table is timed apart, since it does not grow with the rows"""
    t0 = time.perf_counter()
    p = table / table.sum(axis=1)[:, None]
    if metric == "hellinger":
        root = np.sqrt(p)
    else:
        with np.errstate(divide="ignore"):
            lp = np.where(p == 0.0, 0.0, np.log(p))
    t1 = time.perf_counter()
    out = np.empty((rows, len(table)))
    if metric == "hellinger":
        out[:] = root[:rows] @ root.T
    else:
        for i in range(rows):
            m = 0.5 * (p[i][None, :] + p)
            lm = np.log(m)
            out[i] = 0.5 * np.sum(p[i][None, :] * (lp[i][None, :] - lm) + p * (lp - lm), axis=1)
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, out


def run(K, V, args):
    import bench
    from pylda_amd import _capi
    rng = np.random.default_rng(20)
    table = rng.gamma(0.05, size=(K, V)) + 1e-3
    ctx = _capi.Context(2, V)
    tiles = (K + 31) // 32
    out = {"K": K, "V": V, "compute_units": ctx.compute_units(), "fp64_vector_peak_tflops": bench.FP64_VECTOR_PEAK_TFLOPS,
           "pair_words": float(K) * K * V, "tile_pair_words": float(tiles * (tiles + 1) // 2) * 1024 * V, "by_metric": {}}
    for metric, code in METRICS:
        call_ms, steps = _timed(lambda: ctx.topic_distances(table, None, code), args.warmup, args.steps, args.window_ms)
        ctx.set_profiling(True)
        ctx.kernel_time()
        for _ in range(steps):
            values = ctx.topic_distances(table, None, code)
        transform_ms, pair_ms, _ = ctx.kernel_time()
        ctx.set_profiling(False)
        transform_ms, pair_ms = transform_ms / steps, pair_ms / steps
        entry = {"calls_timed": steps, "call_ms": call_ms, "transform_kernel_ms": transform_ms, "pair_and_combine_kernel_ms": pair_ms,
                 "pair_words_per_s": out["pair_words"] / (pair_ms * 1e-3), "tile_pair_words_per_s": out["tile_pair_words"] / (pair_ms * 1e-3)}
        if metric == "hellinger":
            rate = 2.0 * out["tile_pair_words"] / (pair_ms * 1e-3)
            entry["multiply_and_add_instructions_per_s"] = rate
            entry["fraction_of_vector_fp64_instruction_rate"] = rate / (bench.FP64_VECTOR_PEAK_TFLOPS * 1e12 / 2)
        full = out["pair_words"] <= args.host_full_below
        rows = K if full else min(K, args.host_rows)
        host_transform_ms, host_ms, host_values = _host_rows(table, rows, metric)
        scaled_ms = host_transform_ms + host_ms * K / rows
        entry["numpy_host"] = {"rows_timed": rows, "transform_ms": host_transform_ms, "rows_ms": host_ms, "ms_scaled_to_K_rows": scaled_ms,
                               "ratio_to_device_call": scaled_ms / call_ms,
                               "largest_difference_from_device": float(np.max(np.abs(host_values - values[:rows])))}
        out["by_metric"][metric] = entry
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--window_ms", type=float, default=500.0)
    ap.add_argument("--shapes", default="128x50000,1024x100000")
    ap.add_argument("--host_rows", type=int, default=2)
    ap.add_argument("--host_full_below", type=float, default=1e9)
    args = ap.parse_args(argv)
    shapes = [tuple(int(x) for x in shape.split("x")) for shape in args.shapes.split(",")]
    out = {"tool": "topic_distance_bench", "warmup": args.warmup, "steps": args.steps, "window_ms": args.window_ms, "results": [run(K, V, args) for K, V in shapes]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

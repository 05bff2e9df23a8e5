"""The cases of tests/test_gpu_work_counters.py, shared with tests/golden/make_work_counters_golden.py (which recorded
them on the commit whose work counter was ONE workgroup walking all documents): two profiled E-steps of

    K256x96   the K = 256 model of tests/live_exit_cases.py: 96 documents, most of them finished by the live-topic kernel
              (hand-over counts, tile columns, skipped and formed stop sums all non-zero), one row of partial sums
    D1        a single document                                     (one row, 1023 idle threads)
    D1025     1025 short documents at K = 10, dense kernels only     (two rows: 1024 documents and one)

then ONE read of the counters.  Plain module, no GPU."""
import numpy as np

import live_exit_cases

CASES = ("K256x96", "D1", "D1025")
FIELDS = ("inner_iterations", "inner_iteration_terms", "tile_entries", "handed_over", "stop_sums_skipped", "stop_sums_formed")
SHORT_K, SHORT_V = 10, 40


def short_corpus(D, seed=11):
    """D documents of one to three distinct terms of 40, counts 1 .. 50."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 4, D)
    ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    ids = np.concatenate([np.sort(rng.choice(SHORT_V, size=int(m), replace=False)) for m in n]).astype(np.int32)
    cts = rng.integers(1, 51, ids.size).astype(np.int32)
    return ptr, ids, cts


def inputs(case):
    """K, V, ptr, ids, cts, eta, alpha"""
    if case == "K256x96":
        ptr, ids, cts, eta, alpha = live_exit_cases.inputs("K256")
        return live_exit_cases.MODELS["K256"], live_exit_cases.V, ptr, ids, cts, eta, alpha
    D = {"D1": 1, "D1025": 1025}[case]
    rng = np.random.default_rng(1200 + D)
    ptr, ids, cts = short_corpus(D)
    return SHORT_K, SHORT_V, ptr, ids, cts, rng.gamma(100.0, 0.01, (SHORT_K, SHORT_V)), rng.uniform(0.05, 1.0, SHORT_K)


def run(capi, case):
    """dict of FIELDS, and the two clock spans, after two profiled E-steps of a case."""
    import ctypes
    K, V, ptr, ids, cts, eta, alpha = inputs(case)
    ctx = capi.Context(K, V)
    ctx.set_alpha(alpha)
    ctx.set_eta(eta)
    corpus = ctx.corpus(ptr, ids, cts)
    ctx.set_profiling(True)
    ctx.work_counters()
    ctx.estep(corpus)
    ctx.estep(corpus)
    out = dict(zip(FIELDS, ctx.work_counters() + ctx.executed_work() + ctx.stop_sum_counters()))
    shader, wall, hz = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    ctx._check(ctx._lib.pylda_clock_counters(ctx._h, ctypes.byref(shader), ctypes.byref(wall), ctypes.byref(hz)))
    out["clock_spans"] = (shader.value, wall.value, hz.value)
    corpus.close()
    ctx.close()
    return out

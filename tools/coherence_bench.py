#!/usr/bin/env python3
"""Timing of topic coherence on the corpus of bench.py's cfg 3 (synth100k), one GPU.  Prints ONE JSON
line.

    python tools/coherence_bench.py [--warmup 2] [--steps 5] [--train 2] [--top_words 10,20] [--workloads synth100k] [--docs N]

The model is a VariationalBayes engine's eta after `train` full-batch iterations from the usual random start; the reference
corpus is the training corpus.  Timed per M, each with `warmup` calls first and `steps` calls in the window:
    pylda_top_words on the device eta              the call, and the selection kernel alone (profiling bracket)
    pylda_codocument_counts                        the call, and its mark and pair passes alone (profiling brackets)
    the engine's topic_coherence()                 the whole call, host scores included
Byte models: selection K V 8 (the table once), mark nnz 8 (a term id and its share of the slot map per pair - the bitmaps'
atomics are not in it), pair K M D / 8 (every topic's M bitmap rows once).  Reported: each kernel's GB/s against its model.
The yardstick, timed ONCE in the same process: the same integers on the host with numpy / scipy - a stable argsort of -eta,
then a sparse presence matrix of the documents over the distinct top words times itself - checked equal to the device's."""
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


def _host_yardstick(eta, M, ptr, ids):
    import scipy.sparse
    D, V = len(ptr) - 1, eta.shape[1]
    t0 = time.perf_counter()
    top_ids = np.argsort(-eta, axis=1, kind="stable")[:, :M]
    t1 = time.perf_counter()
    words, slot = np.unique(top_ids, return_inverse=True)
    slot = slot.reshape(top_ids.shape)
    presence = scipy.sparse.csr_matrix((np.ones(len(ids), dtype=np.int64), ids, ptr), shape=(D, V))
    presence.sum_duplicates()
    presence.data[:] = 1
    X = presence[:, words]
    co = np.asarray((X.T @ X).todense(), dtype=np.int64)
    co_doc_freq = co[slot[:, :, None], slot[:, None, :]]
    t2 = time.perf_counter()
    return top_ids.astype(np.int32), co_doc_freq, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def run(name, warmup, steps, train, docs, top_words):
    import bench
    from pylda_amd.variational_bayes import VariationalBayes
    wl = bench.build_workload(name, 0, 1, 0, docs)
    ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
    np.random.seed(1)
    engine = VariationalBayes()
    engine._verbose = False
    engine._initialize_parsed(ptr, ids, cts, V, K, 1.0 / K, 1.0 / V)
    for _ in range(train):
        engine.learning()
    ctx, corpus = engine._context(), engine._training_corpus()
    D, nnz = len(ptr) - 1, int(len(ids))
    eta = np.array(engine._eta)
    out = {"workload": name, "cfg": wl.get("cfg"), "documents": D, "K": K, "V": V, "nnz": nnz, "by_top_words": {}}
    for M in top_words:
        top_ids = ctx.top_words(M)[0]
        select_call_ms = _timed(lambda: ctx.top_words(M), warmup, steps)
        counts_call_ms = _timed(lambda: ctx.codocument_counts(corpus, top_ids), warmup, steps)
        whole_ms = _timed(lambda: engine.topic_coherence(top_words=M), warmup, steps)
        ctx.set_profiling(True)
        ctx.kernel_time()
        for _ in range(steps):
            ctx.top_words(M)
        select_ms = ctx.kernel_time()[0] / steps
        for _ in range(steps):
            doc_freq, co = ctx.codocument_counts(corpus, top_ids)
        mark_ms, pair_ms, _ = ctx.kernel_time()
        mark_ms, pair_ms = mark_ms / steps, pair_ms / steps
        ctx.set_profiling(False)
        host_ids, host_co, argsort_ms, product_ms = _host_yardstick(eta, M, ptr, ids)
        bytes_select, bytes_mark, bytes_pair = K * V * 8, nnz * 8, K * M * D // 8
        result = engine.topic_coherence(top_words=M)
        out["by_top_words"][str(M)] = {
            "distinct_top_words": int(len(np.unique(top_ids))),
            "select": {"call_ms": select_call_ms, "kernel_ms": select_ms, "model_bytes": bytes_select,
                       "gb_per_s": bytes_select / (select_ms * 1e-3) / 1e9},
            "mark": {"kernel_ms": mark_ms, "model_bytes": bytes_mark, "gb_per_s": bytes_mark / (mark_ms * 1e-3) / 1e9},
            "pair": {"kernel_ms": pair_ms, "model_bytes": bytes_pair, "gb_per_s": bytes_pair / (pair_ms * 1e-3) / 1e9},
            "codocument_counts_call_ms": counts_call_ms,
            "topic_coherence_call_ms": whole_ms,
            "host_yardstick": {"argsort_ms": argsort_ms, "presence_product_ms": product_ms,
                               "same_integers": bool(np.array_equal(host_ids, top_ids) and np.array_equal(host_co, co))},
            "ratio_host_to_device_calls": (argsort_ms + product_ms) / (select_call_ms + counts_call_ms),
            "umass_mean": result.umass_mean, "npmi_mean": result.npmi_mean, "undefined_pairs": int(result.undefined_pairs.sum())}
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--train", type=int, default=2)
    ap.add_argument("--top_words", default="10,20")
    ap.add_argument("--workloads", default="synth100k")
    ap.add_argument("--docs", type=int, default=None)
    args = ap.parse_args(argv)
    top_words = [int(m) for m in args.top_words.split(",")]
    out = {"tool": "coherence_bench", "warmup": args.warmup, "steps": args.steps, "train": args.train,
           "results": [run(w, args.warmup, args.steps, args.train, args.docs, top_words) for w in args.workloads.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

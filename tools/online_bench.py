#!/usr/bin/env python3
"""Timing of online variational Bayes (pylda_amd/online_vb.py) on the corpus of bench.py's cfg 3 (synth100k: 100k
documents, K = 128, V = 50k), one GPU.  Prints ONE JSON line (--output FILE writes it to a file as well).

    python tools/online_bench.py [--batches 1,10,100] [--warmup-epochs 1] [--epochs 3] [--docs N] [--no-memory] [--output FILE]

Per number of minibatches B: one warm-up epoch (B steps: every minibatch's corpus is uploaded and builds its plan and
postings on its first visit), then `epochs` timed epochs - wall time around learning() calls, each of which ends in its
one host wait.  Reported: ms per step, ms per epoch, documents/s, and the fixed cost of a step,
(epoch ms at B - epoch ms at B = 1) / B: what a step pays whatever its minibatch holds (prepare tables of the K x V eta,
the blend, the topic term, launches, the wait).  The yardstick, taken first in the same session: VariationalBayes.learning()
on the whole corpus with alpha never updated - one epoch of full-batch VB.

Device memory per minibatch corpus is the drop of the device's free memory over the warm-up epoch, divided by B (the
context and its K x V tables exist before it); --no-memory skips it (it imports torch for the one query).  Some layout facts
of minibatch 0 (pylda_corpus_layout) are recorded beside it."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def free_device_bytes():
    import torch
    return int(torch.cuda.mem_get_info(0)[0])


def release(engine):
    for corpus in getattr(engine, "_batch_corpora", {}).values():
        corpus.close()
    if engine._train_corpus is not None:
        engine._train_corpus.close()
    if engine._ctx is not None:
        engine._ctx.close()
    gc.collect()


def yardstick(wl, eta, warmup, steps):
    """ms per full-batch iteration of VariationalBayes.learning(), alpha fixed."""
    from pylda_amd.variational_bayes import VariationalBayes
    K, V = wl["K"], wl["V"]
    engine = VariationalBayes(hyper_parameter_optimize_interval=10 ** 9)
    engine._verbose = False
    engine._initialize_parsed(wl["ptr"], wl["ids"], wl["cts"], V, K, 1.0 / K, 1.0 / V, eta=eta.copy())
    for _ in range(warmup):
        engine.learning()
    t0 = time.perf_counter()
    objective = [engine.learning() for _ in range(steps)]
    wall = time.perf_counter() - t0
    release(engine)
    return {"ms_per_iteration": wall / steps * 1e3, "documents_per_s": (len(wl["ptr"]) - 1) * steps / wall,
            "iterations": steps, "warmup": warmup, "objective_last": objective[-1]}


def online(wl, eta, batches, warmup_epochs, epochs, memory):
    from pylda_amd.online_vb import OnlineVariationalBayes
    K, V = wl["K"], wl["V"]
    D = len(wl["ptr"]) - 1
    engine = OnlineVariationalBayes(batches)
    engine._verbose = False
    engine._initialize_parsed(wl["ptr"], wl["ids"], wl["cts"], V, K, 1.0 / K, 1.0 / V, eta=eta.copy())
    ctx = engine._context()
    engine._push_model()
    ctx.synchronize()
    free_before = free_device_bytes() if memory else None
    t0 = time.perf_counter()
    for _ in range(warmup_epochs * batches):
        engine.learning()
    first_epochs_ms = (time.perf_counter() - t0) * 1e3
    out = {"batches": batches, "documents_per_batch": D / batches, "warmup_epochs_ms": first_epochs_ms}
    if memory:
        out["device_bytes_per_batch_corpus"] = (free_before - free_device_bytes()) / batches
    first = engine._batch_corpora[0]
    out["batch_0_layout"] = {name: first.layout(name) for name in ("gather_live", "gather_blocks", "gather_segments",
                                                                    "gather_partial_rows", "quad_slot_bytes")}
    out["batch_0"] = {"documents": first.D, "nnz": first.nnz}
    t0 = time.perf_counter()
    objective = [engine.learning() for _ in range(epochs * batches)]
    wall = time.perf_counter() - t0
    out.update({"ms_per_step": wall / (epochs * batches) * 1e3, "ms_per_epoch": wall / epochs * 1e3,
                "documents_per_s": D * epochs / wall, "epochs": epochs, "objective_last": objective[-1]})
    release(engine)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,10,100")
    ap.add_argument("--warmup-epochs", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--docs", type=int, default=None, help="override the corpus size (smoke and profiling runs)")
    ap.add_argument("--no-memory", action="store_true", help="skip the device-memory query")
    ap.add_argument("--output", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    import bench
    from pylda_amd import _capi
    _capi.load()
    if _capi.device_count() < 1:
        raise SystemExit("online_bench: no HIP device visible")
    wl = bench.build_workload("synth100k", 0, 1, 0, args.docs)
    eta = np.random.default_rng(1234).gamma(100.0, 0.01, (wl["K"], wl["V"]))
    out = {"tool": "online_bench", "workload": "synth100k", "cfg": wl.get("cfg"), "documents": len(wl["ptr"]) - 1,
           "nnz": int(len(wl["ids"])), "K": wl["K"], "V": wl["V"], "tau0": 1.0, "kappa": 0.7,
           "full_batch": yardstick(wl, eta, args.warmup_epochs, args.epochs), "online": []}
    for batches in (int(b) for b in args.batches.split(",")):
        out["online"].append(online(wl, eta, batches, args.warmup_epochs, args.epochs, not args.no_memory))
    base = next((r for r in out["online"] if r["batches"] == 1), None)
    for r in out["online"]:
        if base is not None and r["batches"] > 1:
            r["fixed_ms_per_step"] = (r["ms_per_epoch"] - base["ms_per_epoch"]) / r["batches"]
    if args.output:
        with open(args.output, "w") as stream:
            stream.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

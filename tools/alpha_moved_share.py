#!/usr/bin/env python3
"""Share of gamma_dk that equals alpha_k bit for bit at the end of an E-step - what the M-step's alpha statistics
(mstep_alpha_ss_moved_kernel) take from their table of psi(alpha_k) - after given outer iterations of a bench.py workload,
from its seeded start.  One reduction over gamma on the host after the iteration; nothing of it is in a timed path.

    python tools/alpha_moved_share.py [--workload synth1m] [--docs N] [--at 4 8] [--out FILE]

alpha is the one the E-step ran with (and the M-step compares against): the iteration's alpha BEFORE its Newton update."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="synth1m")
ap.add_argument("--docs", type=int, default=None)
ap.add_argument("--at", type=int, nargs="+", default=[4, 8])
ap.add_argument("--out", default=None)
args = ap.parse_args()

import bench  # noqa: E402
from pylda_amd.variational_bayes import VariationalBayes  # noqa: E402

import torch  # noqa: E402
wl = bench.build_workload(args.workload, 0, 1, torch.device("cuda", 0), args.docs)
ptr, ids, cts, V, K = wl["ptr"], wl["ids"], wl["cts"], wl["V"], wl["K"]
np.random.seed(0)
eta0 = wl.get("eta")
if eta0 is None:
    eta0 = np.random.gamma(100., 1. / 100., (K, V))
vb = VariationalBayes(hyper_parameter_optimize_interval=1, device=0)
vb._verbose = False
vb._initialize_parsed(ptr, ids, cts, V, K, 1.0 / K, 1.0 / V, eta=eta0)
if "alpha" in wl:
    vb._alpha_alpha = wl["alpha"].copy()
record = {"workload": args.workload, "documents": len(ptr) - 1, "K": K, "iterations": {}}
for it in range(1, max(args.at) + 1):
    alpha = np.array(vb._alpha_alpha, dtype=np.float64)
    vb.learning()
    if it in args.at:
        gamma = np.asarray(vb._gamma, dtype=np.float64)
        same = gamma.view(np.uint64) == alpha.view(np.uint64)[None, :]
        moved = K - same.sum(axis=1)
        record["iterations"][str(it)] = {
            "share_gamma_equals_alpha": float(same.mean()), "moved_per_document_mean": float(moved.mean()),
            "moved_per_document_max": int(moved.max()), "documents_above_63_moved": int((moved > 63).sum())}
        print("outer iteration %d: %s" % (it, record["iterations"][str(it)]), flush=True)
        del gamma, same
line = json.dumps(record)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")

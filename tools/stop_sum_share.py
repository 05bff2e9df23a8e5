"""How often the live-topic kernel skips its stop sum (estep_limits.h live_stop_shortcut) on a bench workload.

    python tools/stop_sum_share.py synth1m|synth100k|nips|ap [docs] [outer ...]

Runs learning() iterations from the seeded start as bench.py does and, for every count in `outer` (default 3 7), profiles
the E-step of that model (the one the next outer iteration starts with): iterations of the live-topic kernel whose stop
sum was skipped and formed (Context.stop_sum_counters), documents handed over.  One JSON line.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    name = sys.argv[1]
    docs = int(sys.argv[2]) if len(sys.argv) > 2 and int(sys.argv[2]) > 0 else None
    outers = sorted(int(a) for a in sys.argv[3:]) or [3, 7]
    import torch
    from pylda_amd.variational_bayes import VariationalBayes
    wl = bench.build_workload(name, 0, 1, torch.device("cuda", 0), docs)
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
    ctx = vb._context()
    out = {"workload": name, "docs": len(ptr) - 1, "K": K, "models": []}
    done = 0
    for outer in outers:
        while done < outer:
            vb.learning()
            done += 1
        vb._push_model()
        ctx.set_option("doc_values", 0)
        ctx.set_profiling(True)
        ctx.work_counters()
        ctx.estep(vb._train_corpus, 50, 1e-6, False)
        iterations = ctx.work_counters()[0]
        handed = ctx.executed_work()[1]
        skipped, formed = ctx.stop_sum_counters()
        ctx.set_profiling(False)
        out["models"].append({"outer_iterations_before": outer, "handed_over": handed, "inner_iterations": iterations,
                              "stop_sums_skipped": skipped, "stop_sums_formed": formed,
                              "share_skipped": skipped / max(1.0, skipped + formed)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

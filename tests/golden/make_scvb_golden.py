"""Regenerates tests/golden/scvb_rehearsal.json: the training plug-in log-likelihood of the SCVB0 restatement
(tests/scvb_restatement.py) at the start and after each of 25 epochs over the first 300 associated-press documents of
ap_train_k10.npz, K = 10, alpha = 1/K, beta = 1/V, seed 5, the default schedule (tau0 = theta_tau0 = 10, kappa =
theta_kappa = 0.9), for 1, 8 and 300 minibatches and burn_in 0 and 1 - recorded results that tests/test_scvb_host.py pins.

    python tests/golden/make_scvb_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import scvb_restatement as spec  # noqa: E402
from conftest import csr_slice, load_golden  # noqa: E402

SEED, EPOCHS, DOCUMENTS, K = 5, 25, 300, 10
BATCHES, BURN_IN = (1, 8, 300), (0, 1)


def rehearsal(batches, burn_in, epochs=EPOCHS):
    """(the chain, the log-likelihood at the start and after every epoch)"""
    g = load_golden("ap_train_k10.npz")
    csr = csr_slice(g["doc_ptr"], g["term_id"], g["term_ct"], range(DOCUMENTS))
    V = len(g["words"])
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    chain = spec.ScvbChain(*csr, K, V)
    chain.init(SEED)
    trace = [chain.log_likelihood(alpha, beta)[0]]
    for _ in range(epochs):
        chain.epoch(alpha, beta, batches, burn_in=burn_in)
        trace.append(chain.log_likelihood(alpha, beta)[0])
    return chain, trace


if __name__ == "__main__":
    out = {"seed": SEED, "epochs": EPOCHS, "documents": DOCUMENTS, "topics": K, "log_likelihood": {}}
    for batches in BATCHES:
        for burn_in in BURN_IN:
            _, trace = rehearsal(batches, burn_in)
            out["log_likelihood"]["%d/%d" % (batches, burn_in)] = trace
            rises = all(b > a for a, b in zip(trace, trace[1:]))
            print(batches, burn_in, trace[0], trace[1], trace[-1], "rises on every epoch" if rises else "does not rise on every epoch")
    with open(os.path.join(HERE, "scvb_rehearsal.json"), "w") as stream:
        json.dump(out, stream, indent=1, sort_keys=True)
        stream.write("\n")

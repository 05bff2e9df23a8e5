"""Regenerates tests/golden/cvb0_rehearsal.json: the training plug-in log-likelihood of the CVB0 restatement
(tests/cvb0_restatement.py) after 25 sweeps over the first 300 associated-press documents of ap_train_k10.npz, K = 10,
alpha = 1/K, beta = 1/V, seed 5, for 1, 16 and 300 blocks - recorded results that tests/test_cvb0_host.py pins.

    python tests/golden/make_cvb0_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import cvb0_restatement as spec  # noqa: E402
from conftest import csr_slice, load_golden  # noqa: E402

SEED, SWEEPS, DOCUMENTS, K = 5, 25, 300, 10


def rehearsal(blocks, remove_own=True):
    """(the chain, the log-likelihood at the start and after every sweep)"""
    g = load_golden("ap_train_k10.npz")
    csr = csr_slice(g["doc_ptr"], g["term_id"], g["term_ct"], range(DOCUMENTS))
    V = len(g["words"])
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    chain = spec.Cvb0Chain(*csr, K, V, remove_own=remove_own)
    chain.init(SEED)
    trace = [chain.log_likelihood(alpha, beta)[0]]
    for _ in range(SWEEPS):
        chain.sweep(alpha, beta, blocks)
        trace.append(chain.log_likelihood(alpha, beta)[0])
    return chain, trace


if __name__ == "__main__":
    out = {"seed": SEED, "sweeps": SWEEPS, "documents": DOCUMENTS, "topics": K, "log_likelihood": {}}
    for blocks in (1, 16, 300):
        _, trace = rehearsal(blocks)
        out["start"] = trace[0]
        out["log_likelihood"][str(blocks)] = trace[-1]
        print(blocks, trace[0], trace[-1])
    with open(os.path.join(HERE, "cvb0_rehearsal.json"), "w") as stream:
        json.dump(out, stream, indent=1, sort_keys=True)
        stream.write("\n")

"""The hand-over timing sweep of tests/test_gpu_quad_handover.py, shared with tests/golden/make_quad_handover_golden.py
(which recorded it on the commit BEFORE the quad kernel decided the hand-over at the bottom of an inner iteration):
K = 256, the 96 documents of test_gpu_quad_slots.boundary_corpus, inner-iteration caps 1 .. 12 crossed with four stop
thresholds, at hand-over counts 4 and 56 (option compact_cap).  Per case: the iteration counts, the executed work (tile
entries, documents handed over - Context.executed_work) and the SHA-256 of gamma's bytes."""
import hashlib

import numpy as np

K = 256
CAPS = (4, 56)
TOLS = (1e-1, 1e-2, 1e-3, 1e-6)            # (the last one is the default of the E-step)
MAX_ITERS = tuple(range(1, 13))


def sweep(capi, inputs, V, options, tol):
    """One context and corpus, the E-step at every cap of MAX_ITERS: list of dicts (iters, gamma, tile_entries, handed_over)."""
    ptr, ids, cts, eta, alpha = inputs
    ctx = capi.Context(K, V)
    for name, value in options:
        ctx.set_option(name, value)
    corpus = ctx.corpus(ptr, ids, cts)
    ctx.set_profiling(True)
    outs = []
    for max_iter in MAX_ITERS:
        ctx.work_counters()
        out = ctx.estep_host(corpus, alpha, eta, max_iter, tol, False)
        ctx.work_counters()
        entries, handed = ctx.executed_work()
        outs.append({"iters": out["iters"].copy(), "gamma": out["gamma"].copy(), "tile_entries": entries, "handed_over": handed,
                     "flagged": ctx.estep_results(corpus)[2]})
    corpus.close()
    ctx.close()
    return outs


def gamma_digest(gamma):
    return hashlib.sha256(np.ascontiguousarray(gamma, dtype=np.float64).tobytes()).hexdigest()


# ---- the boundary-length corpora of tests/test_gpu_quad_slots.py at the strides of the packed prologue: what an E-step
#      gives, as SHA-256 of each array's bytes (tests/test_gpu_quad_prologue.py) ----
BOUNDARY_KS = (129, 256)
BOUNDARY_FIELDS = ("gamma", "doc_ll", "iters", "sstats")


def array_digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def boundary_digests(out, heldout):
    return {name: array_digest(out[name]) for name in BOUNDARY_FIELDS if not (heldout and name == "sstats")}

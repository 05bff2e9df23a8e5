"""The cases of tests/test_gpu_quad_handover_pairs.py, shared with tests/golden/make_quad_handover_pairs_golden.py
(which recorded them on the commit BEFORE the hand-over tile went out in slot pairs, estep_limits.h quad_handover_pairs):
one document of every length 161 .. 256, K = 256 and 129 (table stride 256, the second with padding topics), hand-over
counts 4, the default and 56 (option compact_cap), on the training fast path and with per-document values."""
import hashlib

import numpy as np

V, D = 2000, 96
KS = (256, 129)
CAPS = (4, 0, 56)                          # (0: what the class' register tile holds, 40 or 56 columns)
PATHS = ("fast", "values")                 # training fast path (doc_values = 0) / per-document values
LENGTHS = tuple(range(256, 160, -1))       # longest first, as the schedule sorts them: the tile of the 161 terms lies last
DEFAULT_CAP_LAST = 56                      # columns of a document of at most 192 terms at table stride 256


def corpus(K):
    """96 documents in the style of test_gpu_quad_slots.boundary_corpus, one topic of its own per row of eta: a document
    draws its words from 3 .. 8 of them (4: the last one) and a little from everywhere, counts 2 .. 6 - all but one or
    two dozen topics of a document die within ten iterations, so every document reaches the hand-over count of 56; a
    non-uniform alpha with three topics at 0.05."""
    rng = np.random.default_rng(9000 + K)
    beta = rng.dirichlet(np.full(V, 0.05), size=K)
    ptr, ids, cts = [0], [], []
    for n in LENGTHS:
        m = 4 if n == 161 else int(rng.integers(3, 9))
        theta = np.zeros(K)
        theta[rng.choice(K, size=m, replace=False)] = rng.dirichlet(np.full(m, 2.0))
        p = theta @ beta + 1e-3 / V
        u = np.sort(rng.choice(V, size=n, replace=False, p=p / p.sum()))
        ids.append(u.astype(np.int32))
        cts.append(rng.integers(2, 7, size=n).astype(np.int32))
        ptr.append(ptr[-1] + n)
    eta = rng.gamma(100.0, 0.01, (K, V))
    for k in range(K):
        eta[k] += 40.0 * V * beta[k] * rng.uniform(0.2, 1.0)
    alpha = rng.uniform(0.5, 1.5, K) / K
    alpha[rng.choice(K, size=3, replace=False)] = 0.05
    return np.array(ptr, np.int64), np.concatenate(ids), np.concatenate(cts), eta, alpha


def run(capi, K, inputs, cap, path, options=(), max_iter=50):
    """One E-step: gamma, iteration counts, statistics, the joint value, executed work (tile entries, documents handed
    over), documents flagged for the log-space kernel, the launch classes."""
    ptr, ids, cts, eta, alpha = inputs
    ctx = capi.Context(K, V)
    ctx.set_option("compact_cap", cap)
    for name, value in options:
        ctx.set_option(name, value)
    c = ctx.corpus(ptr, ids, cts)
    ctx.set_profiling(True)
    ctx.work_counters()
    out = ctx.estep_host(c, alpha, eta, max_iter, 1e-6, False, want_doc_values=path == "values")
    ctx.work_counters()
    if path == "fast":
        out["iters"] = ctx.get_doc_values(c, want_ll=False)[2]
    out["joint"] = np.array([out["document_log_likelihood"], out["words_log_likelihood"]])
    out["work"] = np.array(ctx.executed_work())
    out["flagged"] = ctx.estep_results(c)[2]
    out["plan"] = c.plan()
    c.close()
    ctx.close()
    return out


def last_document(inputs):
    """The corpus' last document (161 terms) as a corpus of its own."""
    ptr, ids, cts, eta, alpha = inputs
    lo = ptr[-2]
    return np.array([0, ptr[-1] - lo], np.int64), ids[lo:], cts[lo:], eta, alpha


def live_counts(capi, K, inputs, upto=24):
    """Topics of the FIRST document with gamma != alpha after 1 .. upto inner iterations of the dense kernels alone
    (compact = 0, the iteration cap as the stop): what the quad kernel counts at the bottom of each iteration - a dead
    topic stays at alpha_k bit for bit, and the count never grows."""
    ptr, ids, cts, eta, alpha = inputs
    ctx = capi.Context(K, V)
    ctx.set_option("compact", 0)
    c = ctx.corpus(ptr, ids, cts)
    counts = []
    for max_iter in range(1, upto + 1):
        out = ctx.estep_host(c, alpha, eta, max_iter, 1e-6, False)
        assert out["iters"][0] == max_iter
        counts.append(int(np.count_nonzero(out["gamma"][0] != alpha)))
    c.close()
    ctx.close()
    return counts


def cap_met_exactly(counts, columns=DEFAULT_CAP_LAST):
    """The first live count that fits `columns`: as option compact_cap it makes the document leave the dense kernel in
    that very iteration (the count before was larger) with EVERY column of its tile in use."""
    assert all(a >= b for a, b in zip(counts, counts[1:])), counts
    return next(n for n in counts if n <= columns)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def key(K, cap, path, field):
    return "%d/%d/%s/%s" % (K, cap, path, field)

"""Generate the hybrid-engine goldens from the reference's own hybrid.py (container-only: needs the reference tree).

    python tests/golden/make_hybrid_golden.py moments        -> hybrid_moments_k8.npz
    python tests/golden/make_hybrid_golden.py trace SEED     -> hybrid_trace_part_SEED.npz (one numpy seed; minutes)
    python tests/golden/make_hybrid_golden.py merge SEEDS..  -> hybrid_trace_k10.npz (the parts, one row per seed)

hybrid.py is translated in memory by lib2to3 on top of _ref_loader.load_reference() (which provides inferencer and
variational_bayes, and stubs nltk); nothing of the reference is written anywhere.  The committed files hold numbers only.

moments: fixed eta (K=8, V=40), a stretched alpha, one document of 60 tokens in grouped order (the copies of a term back
to back, the order the device visits) replicated 4000 times and run as 20 batches of 200, in training and in held-out
mode.  Recorded: per-topic mean and variance of gamma over the 4000 documents, the per-batch mean statistics of the
document's terms, the per-batch totals of the document and words log-likelihoods.

trace: Hybrid.learning() on the first 300 associated-press documents, K=10, 15 iterations, alpha 1/K, beta 1/V, the
initial eta pinned (numpy default_rng(3).gamma(100, 1/100)); per iteration the joint log-likelihood and alpha.
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

MOMENT_K, MOMENT_V, REPLICAS, BATCHES = 8, 40, 4000, 20
MOMENT_ALPHA = np.array([0.02, 0.05, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2])
TRACE_DOCS, TRACE_K, TRACE_ITERATIONS = 300, 10, 15


def moment_model():
    """(eta (K, V), the document's distinct terms, their counts) of the moments golden."""
    rng = np.random.default_rng(20240917)
    eta = rng.gamma(2.0, 1.0, (MOMENT_K, MOMENT_V)) + 0.05
    terms = np.array([3, 7, 11, 2, 19, 23, 29, 31, 5, 37, 13, 17, 0, 39])
    counts = np.array([9, 1, 4, 7, 2, 6, 3, 5, 1, 8, 2, 4, 3, 5])
    assert counts.sum() == 60
    return eta, terms, counts


def trace_eta(V):
    return np.random.default_rng(3).gamma(100.0, 1.0 / 100.0, (TRACE_K, V))


def load_hybrid():
    from _ref_loader import REFERENCE_ROOT, load_reference
    load_reference()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from lib2to3 import refactor
    fixers = [f for f in refactor.get_fixers_from_package("lib2to3.fixes") if not f.endswith("fix_import")]
    path = os.path.join(REFERENCE_ROOT, "hybrid.py")
    with open(path) as fh:
        tree = refactor.RefactoringTool(fixers).refactor_string(fh.read() + "\n", path)
    mod = types.ModuleType("hybrid")
    mod.__file__ = path
    sys.modules["hybrid"] = mod
    exec(compile(str(tree), path, "exec"), mod.__dict__)
    return mod


def _model(hybrid, K, V, alpha, eta, word_idss):
    m = hybrid.Hybrid()
    m._type_to_index = {str(v): v for v in range(V)}
    m._index_to_type = {v: str(v) for v in range(V)}
    m._number_of_types = V
    m._counter = 0
    m._number_of_topics = K
    m._alpha_alpha = np.array(alpha, dtype=np.float64)
    m._alpha_beta = np.zeros(V) + 1.0 / V
    m._parsed_corpus = word_idss
    m._number_of_documents = len(word_idss)
    m._gamma = np.tile(m._alpha_alpha + 1.0 * V / K, (len(word_idss), 1))
    m._eta = np.array(eta, dtype=np.float64)
    return m


def make_moments():
    import contextlib
    import io
    hybrid = load_hybrid()
    eta, terms, counts = moment_model()
    doc = [int(t) for t, c in zip(terms, counts) for _ in range(c)]
    per = REPLICAS // BATCHES
    out = {"eta": eta, "alpha": MOMENT_ALPHA, "terms": terms, "counts": counts, "replicas": np.int64(REPLICAS),
           "batches": np.int64(BATCHES)}
    np.random.seed(11)
    for mode in ("train", "heldout"):
        gammas, batch_stats, batch_ll = [], [], []
        for _ in range(BATCHES):
            batch = [list(doc) for _ in range(per)]
            m = _model(hybrid, MOMENT_K, MOMENT_V, MOMENT_ALPHA, eta, batch)
            with contextlib.redirect_stdout(io.StringIO()):
                if mode == "train":
                    ll, sstats = m.e_step()
                    gamma = m._gamma
                    batch_stats.append(sstats[:, terms] / per)
                else:
                    ll, gamma = m.e_step(batch)
            gammas.append(np.array(gamma))
            batch_ll.append(ll)
        g = np.concatenate(gammas)
        out[mode + "_gamma_mean"] = g.mean(axis=0)
        out[mode + "_gamma_var"] = g.var(axis=0, ddof=1)
        out[mode + "_batch_ll"] = np.array(batch_ll)
        if batch_stats:
            out[mode + "_batch_stats"] = np.array(batch_stats)
    np.savez_compressed(os.path.join(HERE, "hybrid_moments_k8.npz"), **out)


def make_trace_part(seed):
    import contextlib
    import io
    hybrid = load_hybrid()
    g = np.load(os.path.join(HERE, "ap_train_k10.npz"))
    V = len(g["words"])
    ptr, ids, cts = g["doc_ptr"], g["term_id"], g["term_ct"]
    docs = [[int(t) for t, c in zip(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]]) for _ in range(int(c))]
            for d in range(TRACE_DOCS)]
    np.random.seed(seed)
    m = _model(hybrid, TRACE_K, V, np.zeros(TRACE_K) + 1.0 / TRACE_K, trace_eta(V), docs)
    m._hyper_parameter_optimize_interval = 1
    lls, alphas = [], []
    for _ in range(TRACE_ITERATIONS):
        with contextlib.redirect_stdout(io.StringIO()):
            lls.append(m.learning())
        alphas.append(np.array(m._alpha_alpha))
    np.savez_compressed(os.path.join(HERE, "hybrid_trace_part_%d.npz" % seed), joint_ll=np.array(lls), alpha=np.array(alphas))


def merge(seeds):
    parts = [np.load(os.path.join(HERE, "hybrid_trace_part_%d.npz" % s)) for s in seeds]
    np.savez_compressed(os.path.join(HERE, "hybrid_trace_k10.npz"), seeds=np.array(seeds),
                        joint_ll=np.stack([p["joint_ll"] for p in parts]), alpha=np.stack([p["alpha"] for p in parts]),
                        documents=np.int64(TRACE_DOCS), iterations=np.int64(TRACE_ITERATIONS))
    for s in seeds:
        os.remove(os.path.join(HERE, "hybrid_trace_part_%d.npz" % s))


if __name__ == "__main__":
    if sys.argv[1] == "moments":
        make_moments()
    elif sys.argv[1] == "trace":
        make_trace_part(int(sys.argv[2]))
    else:
        merge([int(s) for s in sys.argv[2:]])

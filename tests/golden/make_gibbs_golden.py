"""Generate the collapsed-Gibbs goldens from the reference's own monte_carlo.py (container-only: needs the reference tree).

    python tests/golden/make_gibbs_golden.py posterior              -> gibbs_posterior.npz
    python tests/golden/make_gibbs_golden.py sequential FIRST COUNT -> gibbs_sequential_part_FIRST.npz (numpy seeds FIRST..)
    python tests/golden/make_gibbs_golden.py sequential-merge FIRSTS.. -> gibbs_sequential_k3.npz
    python tests/golden/make_gibbs_golden.py trace SEED             -> gibbs_trace_part_SEED.npz (one numpy seed; ten minutes)
    python tests/golden/make_gibbs_golden.py merge SEEDS..          -> gibbs_trace_k10.npz

monte_carlo.py is translated in memory by lib2to3 on top of _ref_loader.load_reference(); nothing of the reference is
written anywhere and the committed files hold numbers only.  The reference indexes its count arrays with the float
topics that random_initialize() leaves in _k_dn, which this numpy refuses; the maker casts those arrays (data of the
loaded object) to int64 right after the initial assignment.

posterior: two hand-made count states (A: K=5, V=30, D=12; B: K=10, V=2000, D=300) with vector alpha and vector beta, the
reference's log_posterior on them, and the alpha, beta its optimize_hyperparameters() leaves from numpy seeds 0 and 1
(A with the symmetric switches on and off, B with the launcher's default, on).

sequential: 6 documents, V=12, K=3, 40 tokens, alpha 0.5, beta 0.1, no hyper-parameter step; per numpy seed after
iterations 10, 20, 30 the log posterior, the sorted n_k and sum_d max_k n_dk (stored as float32: the counts are exact,
the log posterior keeps seven digits, far below its spread over the seeds).

trace: the first 300 associated-press documents, K=10, alpha 1/K, beta 1/V, 60 iterations, no hyper-parameter step;
the log posterior after every iteration.
"""
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

TRACE_DOCS, TRACE_K, TRACE_ITERATIONS = 300, 10, 60
TINY_K, TINY_V, TINY_ALPHA, TINY_BETA, TINY_MARKS = 3, 12, 0.5, 0.1, (10, 20, 30)
TINY_DOCS = [[0, 0, 1, 2, 3, 0, 1, 4], [4, 5, 5, 6, 7, 5, 4], [8, 9, 10, 11, 8, 8, 9], [0, 1, 5, 6, 2, 0],
             [9, 10, 4, 5, 11, 10], [2, 3, 7, 8, 3, 2]]
OPT_CASES = (("A", True), ("A", False), ("B", True))
OPT_SEEDS = (0, 1)


def posterior_state(name):
    """(n_dk, n_kv, alpha, beta) of a hand-made state: tokens drawn from a sparse LDA, counted."""
    K, V, D, length, seed = {"A": (5, 30, 12, 25, 5), "B": (10, 2000, 300, 150, 6)}[name]
    rng = np.random.default_rng(seed)
    phi = rng.dirichlet(np.zeros(V) + 0.05, K)
    n_dk = np.zeros((D, K), dtype=np.int64)
    n_kv = np.zeros((K, V), dtype=np.int64)
    for d in range(D):
        theta = rng.dirichlet(np.zeros(K) + 0.3)
        for k in rng.choice(K, size=int(rng.integers(length // 2, 2 * length)), p=theta):
            n_dk[d, k] += 1
            n_kv[k, rng.choice(V, p=phi[k])] += 1
    alpha = rng.gamma(2.0, 0.2, K) + 0.01
    beta = rng.gamma(2.0, 0.02, V) + 0.001
    return n_dk, n_kv, alpha, beta


def load_monte_carlo():
    from _ref_loader import REFERENCE_ROOT, load_reference
    load_reference()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from lib2to3 import refactor
    fixers = [f for f in refactor.get_fixers_from_package("lib2to3.fixes") if not f.endswith("fix_import")]
    path = os.path.join(REFERENCE_ROOT, "monte_carlo.py")
    with open(path) as fh:
        tree = refactor.RefactoringTool(fixers).refactor_string(fh.read() + "\n", path)
    mod = types.ModuleType("monte_carlo")
    mod.__file__ = path
    sys.modules["monte_carlo"] = mod
    exec(compile(str(tree), path, "exec"), mod.__dict__)
    return mod


def _bare(mc, K, V, alpha, beta, symmetric=True):
    m = mc.MonteCarlo(10 ** 9, symmetric, symmetric)
    m._type_to_index = {str(v): v for v in range(V)}
    m._index_to_type = {v: str(v) for v in range(V)}
    m._number_of_types = V
    m._counter = 0
    m._number_of_topics = K
    m._alpha_alpha = np.zeros(K) + alpha
    m._alpha_beta = np.zeros(V) + beta
    return m


def _sampler(mc, K, V, alpha, beta, docs):
    """A reference model on `docs` (lists of term ids) with its own random initial assignment."""
    m = _bare(mc, K, V, alpha, beta)
    m._parsed_corpus = docs
    m._number_of_documents = len(docs)
    m._n_dk = np.zeros((len(docs), K))
    m._n_kv = np.zeros((K, V))
    m._n_k = np.zeros(K)
    m._k_dn = {}
    m.random_initialize()
    for d in m._k_dn:
        m._k_dn[d] = m._k_dn[d].astype(np.int64)
    return m


def make_posterior():
    mc = load_monte_carlo()
    out = {"opt_seeds": np.array(OPT_SEEDS)}
    for name in ("A", "B"):
        n_dk, n_kv, alpha, beta = posterior_state(name)
        K, V = n_kv.shape

        def model(symmetric=True):
            m = _bare(mc, K, V, alpha, beta, symmetric)
            m._number_of_documents = len(n_dk)
            m._n_dk, m._n_kv, m._n_k = n_dk.astype(np.float64), n_kv.astype(np.float64), n_kv.sum(1).astype(np.float64)
            return m
        out.update({name + "_n_dk": n_dk.astype(np.int32), name + "_n_kv": n_kv.astype(np.int32), name + "_alpha": alpha,
                    name + "_beta": beta, name + "_lp": np.float64(model().log_posterior(alpha, beta))})
        flat = model()
        out[name + "_lp_flat"] = np.float64(flat.log_posterior(np.zeros(K) + 1.0 / K, np.zeros(V) + 1.0 / V))
        for case, symmetric in OPT_CASES:
            if case != name:
                continue
            alphas, betas = [], []
            for seed in OPT_SEEDS:
                m = model(symmetric)
                np.random.seed(seed)
                m.optimize_hyperparameters()
                alphas.append(np.array(m._alpha_alpha))
                betas.append(np.array(m._alpha_beta))
            tag = "%s_opt_%s_" % (name, "sym" if symmetric else "vec")
            out[tag + "alpha"], out[tag + "beta"] = np.array(alphas), np.array(betas)
    np.savez_compressed(os.path.join(HERE, "gibbs_posterior.npz"), **out)


def make_sequential_part(first, count):
    mc = load_monte_carlo()
    rows = []
    for seed in range(first, first + count):
        np.random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            m = _sampler(mc, TINY_K, TINY_V, TINY_ALPHA, TINY_BETA, [list(d) for d in TINY_DOCS])
            row = []
            for it in range(1, TINY_MARKS[-1] + 1):
                m.learning()
                if it in TINY_MARKS:
                    row.append([m.log_posterior(m._alpha_alpha, m._alpha_beta)] + sorted(m._n_k) + [m._n_dk.max(axis=1).sum()])
        rows.append(row)
    np.savez_compressed(os.path.join(HERE, "gibbs_sequential_part_%d.npz" % first), stats=np.array(rows),
                        seeds=np.arange(first, first + count))


def merge_sequential(firsts):
    names = [os.path.join(HERE, "gibbs_sequential_part_%d.npz" % f) for f in firsts]
    parts = [np.load(n) for n in names]
    ptr = np.cumsum([0] + [len(d) for d in TINY_DOCS])
    np.savez_compressed(os.path.join(HERE, "gibbs_sequential_k3.npz"), seeds=np.concatenate([p["seeds"] for p in parts]),
                        stats=np.concatenate([p["stats"] for p in parts]).astype(np.float32), marks=np.array(TINY_MARKS),
                        stat_names=np.array(["log_posterior", "n_k_0", "n_k_1", "n_k_2", "sum_max_n_dk"]),
                        doc_ptr=ptr, tokens=np.concatenate(TINY_DOCS), K=np.int64(TINY_K), V=np.int64(TINY_V),
                        alpha=np.float64(TINY_ALPHA), beta=np.float64(TINY_BETA))
    for n in names:
        os.remove(n)


def make_trace_part(seed):
    mc = load_monte_carlo()
    g = np.load(os.path.join(HERE, "ap_train_k10.npz"))
    V = len(g["words"])
    ptr, ids, cts = g["doc_ptr"], g["term_id"], g["term_ct"]
    docs = [[int(t) for t, c in zip(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]]) for _ in range(int(c))]
            for d in range(TRACE_DOCS)]
    np.random.seed(seed)
    lps = []
    with contextlib.redirect_stdout(io.StringIO()):
        m = _sampler(mc, TRACE_K, V, 1.0 / TRACE_K, 1.0 / V, docs)
        for _ in range(TRACE_ITERATIONS):
            m.learning()
            lps.append(m.log_posterior(m._alpha_alpha, m._alpha_beta))
    np.savez_compressed(os.path.join(HERE, "gibbs_trace_part_%d.npz" % seed), log_posterior=np.array(lps))


def merge(seeds):
    names = [os.path.join(HERE, "gibbs_trace_part_%d.npz" % s) for s in seeds]
    np.savez_compressed(os.path.join(HERE, "gibbs_trace_k10.npz"), seeds=np.array(seeds),
                        log_posterior=np.stack([np.load(n)["log_posterior"] for n in names]),
                        documents=np.int64(TRACE_DOCS), iterations=np.int64(TRACE_ITERATIONS), K=np.int64(TRACE_K))
    for n in names:
        os.remove(n)


if __name__ == "__main__":
    if sys.argv[1] == "posterior":
        make_posterior()
    elif sys.argv[1] == "sequential":
        make_sequential_part(int(sys.argv[2]), int(sys.argv[3]))
    elif sys.argv[1] == "sequential-merge":
        merge_sequential([int(s) for s in sys.argv[2:]])
    elif sys.argv[1] == "trace":
        make_trace_part(int(sys.argv[2]))
    else:
        merge([int(s) for s in sys.argv[2:]])

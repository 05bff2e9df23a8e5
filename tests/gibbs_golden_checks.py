"""Comparisons against the goldens of the reference's monte_carlo.py (tests/golden/make_gibbs_golden.py), shared by the
CPU tests of the numpy restatement and the GPU tests of the kernels."""
import numpy as np

Z = 5.0
TRACE_FROM, TRACE_TO = 41, 60          # S = mean of the log posterior over these iterations (1-based, inclusive)


def grouped_csr(docs):
    """Token lists -> CSR with a term's copies merged, terms in first-occurrence order."""
    ptr, ids, cts = [0], [], []
    for tokens in docs:
        counts = {}
        for t in tokens:
            counts[int(t)] = counts.get(int(t), 0) + 1
        ids += list(counts.keys())
        cts += list(counts.values())
        ptr.append(len(ids))
    return np.array(ptr, dtype=np.int64), np.array(ids, dtype=np.int32), np.array(cts, dtype=np.int32)


def tiny_corpus(golden):
    ptr, tokens = golden["doc_ptr"], golden["tokens"]
    return grouped_csr([tokens[ptr[d]:ptr[d + 1]] for d in range(len(ptr) - 1)])


def first_documents(ap, n):
    """CSR of the first n documents of the associated-press training golden."""
    end = int(ap["doc_ptr"][n])
    return ap["doc_ptr"][:n + 1].astype(np.int64), ap["term_id"][:end].astype(np.int32), ap["term_ct"][:end].astype(np.int32)


def chain_statistics(chain, alpha, beta):
    """(replicas, 5): log posterior, the sorted n_k, sum_d max_k n_dk - none depends on the topics' names."""
    R = chain.R
    lp = np.array([chain.log_posterior(alpha, beta, r) for r in range(R)])
    n_k = np.sort(chain.n_k, axis=1)
    peak = chain.n_dk.reshape(R, chain.D1, chain.K).max(axis=2).sum(axis=1)
    return np.column_stack([lp, n_k, peak]).astype(np.float64)


def _variance_se(x):
    """Standard error of the sample variance from the sample's fourth central moment."""
    n = x.shape[0]
    c = x - x.mean(axis=0)
    var = (c ** 2).sum(axis=0) / (n - 1)
    m4 = (c ** 4).mean(axis=0)
    return np.sqrt(np.maximum(m4 - var ** 2 * (n - 3.0) / (n - 1.0), 0.0) / n)


def moment_failures(reference, mine, names, label=""):
    """Statistics (samples, n) of two samples: where the means differ by more than 5 sigma (sigma from both samples) or
    the variances by more than 5 standard errors (from the fourth moments of both samples)."""
    reference, mine = np.asarray(reference, dtype=np.float64), np.asarray(mine, dtype=np.float64)
    bad = []
    sigma = np.sqrt(reference.var(axis=0, ddof=1) / len(reference) + mine.var(axis=0, ddof=1) / len(mine))
    zm = np.abs(reference.mean(axis=0) - mine.mean(axis=0)) / sigma
    se = np.sqrt(_variance_se(reference) ** 2 + _variance_se(mine) ** 2)
    zv = np.abs(reference.var(axis=0, ddof=1) - mine.var(axis=0, ddof=1)) / se
    for i, name in enumerate(names):
        if not zm[i] <= Z:
            bad.append("%s mean of %s: %.4f vs %.4f (z=%.2f)" % (label, name, mine[:, i].mean(), reference[:, i].mean(), zm[i]))
        if not zv[i] <= Z:
            bad.append("%s variance of %s: %.4f vs %.4f (z=%.2f)" % (label, name, mine[:, i].var(ddof=1),
                                                                   reference[:, i].var(ddof=1), zv[i]))
    return bad


def trace_statistic(log_posterior):
    """S of a trace (.., iterations): the mean over iterations 41..60."""
    return np.asarray(log_posterior)[..., TRACE_FROM - 1:TRACE_TO].mean(axis=-1)


def trace_band(golden):
    """(lo, hi): the mean of the reference seeds' S +- 5 sample standard deviations, not less than half their range."""
    s = trace_statistic(golden["log_posterior"])
    half = max(Z * s.std(ddof=1), 0.5 * (s.max() - s.min()))
    return s.mean() - half, s.mean() + half

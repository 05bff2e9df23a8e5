"""What the left-to-right estimator is held to, on the host and on the device: the K = 3, V = 5 model
of foldin_fixture.py, whose p(w) can be enumerated, and the estimator written straight from the paper."""
import itertools

import numpy as np
import scipy.special

import foldin_fixture as fx

SEVEN = fx.WORDS                    # the seven-token document
TWO = [4, 4]                        # a two-token document - one term, two copies: resampling leaves z_0 in its stationary law
REPLICAS = 1600                     # standard error of mean exp(ll) at R = 1: 0.8 % of p(w) for either document


def corpus(words, replicas):
    """The document `replicas` times (global documents 0 .. replicas - 1: independent chains), grouped CSR."""
    ids, cts = np.unique(words, return_counts=True)
    ptr = np.arange(replicas + 1, dtype=np.int64) * len(ids)
    return ptr, np.tile(ids, replicas).astype(np.int32), np.tile(cts, replicas).astype(np.int32)


def exact_probability(words, P, alpha):
    """p(w) = sum over all K^N assignments z of prod_n P[w_n][z_n] * DirMult(z | alpha), theta integrated out."""
    alpha = np.asarray(alpha, dtype=np.float64)
    K, N = len(alpha), len(words)
    const = scipy.special.gammaln(alpha.sum()) - scipy.special.gammaln(alpha.sum() + N) - np.sum(scipy.special.gammaln(alpha))
    total = 0.0
    for z in itertools.product(range(K), repeat=N):
        n = np.bincount(z, minlength=K)
        total += np.exp(np.sum(np.log(P[words, z])) + np.sum(scipy.special.gammaln(n + alpha)) + const)
    return float(total)


def paper_algorithm_3(words, P, alpha, particles, replicas, rng):
    """Wallach et al. 2009, Algorithm 3, as printed, `replicas` independent runs side by side: for each position n, for each
    particle r, resample z_n' for n' < n from (count without n' + alpha_t) P[w_n'][t]; p_n += sum_t (count_t + alpha_t)
    P[w_n][t] / (n + alpha_sum); draw z_n; l += log(p_n / R).  numpy's own generator and sums, no lane layout."""
    alpha = np.asarray(alpha, dtype=np.float64)
    K, N, M = len(alpha), len(words), int(replicas)
    rows = np.arange(M)

    def categorical(weights):
        cdf = np.cumsum(weights, axis=1)
        return np.minimum((cdf < (rng.random(M) * cdf[:, -1])[:, np.newaxis]).sum(axis=1), K - 1)
    z = np.zeros((particles, M, N), dtype=np.int64)
    counts = np.zeros((particles, M, K))
    ll = np.zeros(M)
    for n in range(N):
        pn = np.zeros(M)
        for r in range(particles):
            for m in range(n):
                counts[r, rows, z[r, :, m]] -= 1
                z[r, :, m] = categorical((counts[r] + alpha) * P[words[m]])
                counts[r, rows, z[r, :, m]] += 1
            weights = (counts[r] + alpha) * P[words[n]]
            pn += weights.sum(axis=1) / (n + alpha.sum())
            z[r, :, n] = categorical(weights)
            counts[r, rows, z[r, :, n]] += 1
        ll += np.log(pn / particles)
    return ll


def z_score(values, exact):
    values = np.asarray(values, dtype=np.float64)
    return float((values.mean() - exact) / (values.std(ddof=1) / np.sqrt(len(values))))

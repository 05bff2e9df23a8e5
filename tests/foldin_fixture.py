"""The fixture the held-out fold-in is held to, on the host and on the device: a posterior small
enough to enumerate, and the test of a sampler's output against it."""
import itertools

import numpy as np
import scipy.special

import foldin_restatement as spec

# The enumeration fixture: K = 3, V = 5, one document of seven tokens.
N_KV = np.array([[40, 3, 0, 9, 1], [2, 30, 12, 0, 4], [5, 5, 5, 20, 0]])
BETA = np.array([.05, .1, .2, .05, .4])
ALPHA = np.array([.02, .4, 3.2])
WORDS = [0, 0, 0, 1, 3, 3, 4]
EXPECTED = np.array([0.3101, 0.7631, 5.9268])      # E[n_dk], to the four decimals given
REPLICAS, SWEEPS, BURN_IN = 4000, 100, 40


def table():
    return spec.predictive_table(N_KV, N_KV.sum(axis=1), BETA, float(np.sum(BETA)))


def corpus(replicas=REPLICAS):
    """The document `replicas` times (global documents 0 .. replicas - 1: independent chains), grouped CSR."""
    ids, cts = np.unique(WORDS, return_counts=True)
    ptr = np.arange(replicas + 1, dtype=np.int64) * len(ids)
    return ptr, np.tile(ids, replicas).astype(np.int32), np.tile(cts, replicas).astype(np.int32)


def exact_counts(alpha=ALPHA):
    """E[n_dk] under the posterior over the 3^7 assignments: prod_i P[w_i][z_i] * prod_k Gamma(n_k + alpha_k)."""
    P = table()
    K = len(alpha)
    weights, counts = [], []
    for z in itertools.product(range(K), repeat=len(WORDS)):
        n = np.bincount(z, minlength=K)
        weights.append(np.sum(np.log(P[WORDS, z])) + np.sum(scipy.special.gammaln(n + alpha)))
        counts.append(n)
    weights = np.exp(np.array(weights) - max(weights))
    return (weights[:, np.newaxis] * np.array(counts)).sum(axis=0) / weights.sum()


def z_scores(gamma, alpha=ALPHA):
    """Per topic: (mean over the replicas of gamma - alpha, minus the exact value) in standard errors across the replicas."""
    counts = gamma - alpha[np.newaxis, :]
    return (counts.mean(axis=0) - exact_counts()) / (counts.std(axis=0, ddof=1) / np.sqrt(len(counts)))

"""Writes tests/golden/logspace_mp.npz: the reference's E-step (variational_bayes.py:162-207, training and held-out) for a
handful of tiny documents in mpmath at 50 digits - what the log-space kernel (pylda_amd/csrc/estep_logspace.h) and the fp64
C oracle are measured against where the oracle's own accuracy is the question.  Pure host code.

    python tests/golden/make_logspace_mp.py

The inputs come from closed formulas (tests/safety_net_cases.py: MP_CASES, mp_inputs), so the file holds results only.  Per
case c and iteration cap m, keys "<c>_m<m>_...", every value the mpmath result rounded once to a double:
  gamma        (D, K)   :188 after the last inner iteration
  doc_ll       (D,)     :195-199 of the document
  words_ll     (D,)     :204 of the document (held-out mode; gamma and the iteration count are those of training mode)
  sstats       (K, V)   :207 summed over the documents
  iters        (D,)     inner iterations run
  stop_margin  (D,)     the smallest |mean |delta gamma| / tol - 1| over the iterations run: the stop test (:189) is nowhere
                        within 1e-6 of its threshold (asserted), so fp64 and mpmath must stop together

The cases: K = 65 and 257 (one topic beyond a wavefront's / a workgroup's stride) with documents of 1-5 terms and one count
of 10^6; K = 1024 at alpha = 1e-4 with documents of one, two and four tokens - psi(gamma) between -1e3 and -1e4, lnG(1e-4) -
where a dense kernel flags the document; K = 1."""
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import safety_net_cases as cases          # noqa: E402

DIGITS = 50
TOL = 1e-6


def logsumexp(xs):
    top = max(xs)
    return top + mpmath.log(mpmath.fsum(mpmath.exp(x - top) for x in xs))


def compute(name, max_iter, tol=TOL):
    mpmath.mp.dps = DIGITS
    mpf = mpmath.mpf
    alpha64, eta64, ptr, ids, cts = cases.mp_inputs(name)
    K, V = eta64.shape
    alpha = [mpf(float(a)) for a in alpha64]
    eta = [[mpf(float(x)) for x in row] for row in eta64]
    row_psi = [mpmath.digamma(mpmath.fsum(row)) for row in eta]
    elog = [[mpmath.digamma(eta[k][w]) - row_psi[k] for w in range(V)] for k in range(K)]              # :152
    elog_prob = [[elog[k][w] - lse for w in range(V)] for k, lse in ((k, logsumexp(elog[k])) for k in range(K))]   # :155
    D = len(ptr) - 1
    out = {"gamma": np.zeros((D, K)), "doc_ll": np.zeros(D), "words_ll": np.zeros(D), "sstats": np.zeros((K, V)),
           "iters": np.zeros(D, dtype=np.int32), "stop_margin": np.zeros(D)}
    sstats = [[mpf(0)] * V for _ in range(K)]
    alpha_term = mpmath.loggamma(mpmath.fsum(alpha)) - mpmath.fsum(mpmath.loggamma(a) for a in alpha)   # :195
    for d in range(D):
        w = [int(i) for i in ids[ptr[d]:ptr[d + 1]]]
        c = [mpf(int(x)) for x in cts[ptr[d]:ptr[d + 1]]]
        N = len(w)
        gamma = [a + mpmath.fsum(c) / K for a in alpha]                                                 # :165
        margin, log_phi, iters = mpf("inf"), None, 0
        for _ in range(max_iter):                                                                       # :174
            ps = [mpmath.digamma(g) for g in gamma]
            log_phi = [[elog[k][w[n]] + ps[k] for k in range(K)] for n in range(N)]                     # :177
            for n in range(N):
                lse = logsumexp(log_phi[n])
                log_phi[n] = [x - lse for x in log_phi[n]]                                              # :182
            new = [alpha[k] + mpmath.fsum(mpmath.exp(log_phi[n][k] + mpmath.log(c[n])) for n in range(N))
                   for k in range(K)]                                                                   # :185
            change = mpmath.fsum(abs(new[k] - gamma[k]) for k in range(K)) / K                          # :187
            gamma = new
            iters += 1
            if tol > 0:
                margin = min(margin, abs(change / mpf(tol) - 1))
            if change <= tol:                                                                           # :189
                break
        ll = alpha_term + mpmath.fsum(mpmath.loggamma(g) for g in gamma) - mpmath.loggamma(mpmath.fsum(gamma))   # :197
        ll -= mpmath.fsum(c[n] * mpmath.exp(log_phi[n][k]) * log_phi[n][k] for n in range(N) for k in range(K))  # :199
        wll = mpmath.fsum(mpmath.exp(log_phi[n][k]) * c[n] * elog_prob[k][w[n]] for n in range(N) for k in range(K))  # :204
        for n in range(N):
            for k in range(K):
                sstats[k][w[n]] += mpmath.exp(log_phi[n][k]) * c[n]                                     # :207
        assert margin > 1e-6, (name, max_iter, d, margin)
        out["gamma"][d] = [float(g) for g in gamma]
        out["doc_ll"][d], out["words_ll"][d], out["iters"][d] = float(ll), float(wll), iters
        out["stop_margin"][d] = float(min(margin, mpf(1e300)))
    out["sstats"][:] = [[float(x) for x in row] for row in sstats]
    return out


def main():
    store = {}
    for name, K, lengths, _, _ in cases.MP_CASES:
        for m in cases.MP_MAX_ITER:
            got = compute(name, m)
            print("%s max_iter %d: iterations %s, smallest stop margin %.3g" % (name, m, got["iters"].tolist(),
                                                                               got["stop_margin"].min()))
            for key, value in got.items():
                store["%s_m%d_%s" % (name, m, key)] = value
    np.savez_compressed(os.path.join(HERE, "logspace_mp.npz"), **store)


if __name__ == "__main__":
    main()

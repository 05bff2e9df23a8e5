"""Writes tests/golden/posterior_mp.npz: the collapsed Gibbs log posterior (monte_carlo.py:217-256 of the reference; on the
device estep_gibbs.h through pylda_test_gibbs_posterior_terms) term by term, from mpmath at 50 digits.  Pure host code.

    python tests/golden/make_posterior_mp.py

The states are NOT stored: tests/posterior_cases.py rebuilds them, and <case>_sha256 (32 bytes over K, V, D, n_dk, n_kv,
n_k, alpha and beta) ties the numbers below to the inputs they were computed from.  Per case of posterior_cases.NAMES,
every reference a (hi, lo) pair of doubles as in make_special_mp.py - hi the correctly rounded value, lo the correctly
rounded remainder:
  <case>_docs_hi / _lo     (D,)   sum_k lnG(n_dk[d][k] + alpha_k) - lnG(N_d + sum alpha)
  <case>_words_hi / _lo    (V,)   sum_k lnG(n_kv[k][v] + beta_v)
  <case>_sums_hi / _lo     (3,)   the three device sums: docs + words - sum_k lnG(n_k + sum beta); the documents' half;
                                  the words' and n_k's half
  <case>_totals_hi / _lo   (3,)   what the public entry points return: pylda_gibbs_log_posterior's total and the two
                                  parts of pylda_gibbs_log_posterior_parts - the sums plus (lnG(sum alpha) -
                                  sum_k lnG(alpha_k)) D and (lnG(sum beta) - sum_v lnG(beta_v)) K
All of it from the DOUBLES the device receives: the priors as float64, sum alpha and sum beta the exact sums of those
doubles, the counts exact integers.
"""
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_special_mp import pair          # noqa: E402  (the same (hi, lo) convention)
import posterior_cases as cases           # noqa: E402

DIGITS = 50


def exact_sum(values):
    f = sum((Fraction(float(v)) for v in values), Fraction(0))
    return mpmath.mpf(int(f.numerator)) / mpmath.mpf(int(f.denominator))


def references(c):
    """(docs, words, sums, totals) as lists of mpf"""
    seen = {}

    def lg(count, prior):
        """lnG(count + prior): the count an integer, the prior a double or an mpf"""
        key = (int(count), prior)
        if key not in seen:
            seen[key] = mpmath.loggamma(mpmath.mpf(int(count)) + (prior if isinstance(prior, mpmath.mpf) else mpmath.mpf(float(prior))))
        return seen[key]

    alpha, beta = [float(a) for a in c.alpha], [float(b) for b in c.beta]
    alpha_sum, beta_sum = exact_sum(alpha), exact_sum(beta)
    docs = [mpmath.fsum(lg(c.n_dk[d, k], alpha[k]) for k in range(c.K)) - lg(c.n_dk[d].sum(), alpha_sum) for d in range(c.D)]
    words = [mpmath.fsum(lg(c.n_kv[k, v], beta[v]) for k in range(c.K)) for v in range(c.V)]
    topics = mpmath.fsum(lg(c.n_k[k], beta_sum) for k in range(c.K))
    half_docs, half_words = mpmath.fsum(docs), mpmath.fsum(words) - topics
    sums = [half_docs + half_words, half_docs, half_words]
    scalar_alpha = (lg(0, alpha_sum) - mpmath.fsum(lg(0, a) for a in alpha)) * c.D
    scalar_beta = (lg(0, beta_sum) - mpmath.fsum(lg(0, b) for b in beta)) * c.K
    totals = [scalar_alpha + scalar_beta + sums[0], scalar_alpha + sums[1], scalar_beta + sums[2]]
    return docs, words, sums, totals


def main():
    mpmath.mp.dps = DIGITS
    out = {}
    terms = 0
    for name in cases.NAMES:
        c = cases.case(name)
        out[name + "_sha256"] = c.digest()
        for key, values in zip(("docs", "words", "sums", "totals"), references(c)):
            both = np.array([pair(v) for v in values], dtype=np.float64).reshape(-1, 2)
            out["%s_%s_hi" % (name, key)] = both[:, 0].copy()
            out["%s_%s_lo" % (name, key)] = both[:, 1].copy()
        terms += c.D + c.V
        print("%s: K = %d, V = %d, D = %d, log posterior %.17g" % (name, c.K, c.V, c.D, out[name + "_totals_hi"][0]))
    path = os.path.join(HERE, "posterior_mp.npz")
    np.savez_compressed(path, digits=DIGITS, **out)
    print("posterior_mp: %d cases, %d terms, %d bytes" % (len(cases.NAMES), terms, os.path.getsize(path)))


if __name__ == "__main__":
    main()

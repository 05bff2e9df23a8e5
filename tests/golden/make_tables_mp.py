"""Writes tests/golden/tables_mp.npz: high-precision references for the tables every E-step prepares from eta
(pylda_amd/csrc/prepare_kernels.h through pylda_test_tables) and for alpha_mortality_kernel's classification, from mpmath
at 60 digits.  Pure host code.

    python tests/golden/make_tables_mp.py

Per case c = "K<K>_V<V>" (tests/tables_reference.py: CASES), every reference a (hi, lo) pair of doubles as in
make_special_mp.py - hi the correctly rounded value, lo the correctly rounded remainder:
  <c>_eta               (K, V)   the input itself (no seed is stored: the file is the definition of the case)
  <c>_u_hi / _u_lo      (K, V)   u[k][w] = psi(eta[k][w]) - psi(sum_v eta[k][v]), UNSHIFTED; the row sum is the exact sum
  <c>_rowsum_hi / _lo   (K,)     psi(sum_v eta[k][v])
  <c>_lse_hi / _lo      (K,)     log sum_v exp(u[k][v])
Everything else (shift, e = u - shift, b = exp(e), b e) tests/tables_reference.py derives from the pairs in long double.

What an eta holds (rows are topics; each part only where the shape has room for it, asserted below on mpmath's values):
  all          entries log-uniform over 1e-5 .. 1e6: about a fifth of them have psi below -745, an exact 0 of exp(e)
  K >= 6       rows 0 and 1 identical (their e must agree bit for bit); row 2 with a sum near 1e9; row 3 with a sum
               below 1 (psi of the sum is negative); row 5 is row 4 with ONE entry moved by an ulp, the largest of its
               word: two topics tie for that word's maximum to within an ulp of u
               one word whose maximum is in topic K - 1, and at K > 64 one whose maximum is in topic 63 (a shift taken
               over too few columns shows there)
  K >= 17, V > 1   a word - two at K < 40 - whose e sweeps from about -700 to about -760 over the topics, beside one
               entry near the root of psi: exp(e) goes through the subnormals to an exact 0.  More than 10 subnormal and
               more than 10 zero reference values of exp(e) per case
  V == 1       (K = 300) the row sum IS the entry: u is identically 0, whatever eta holds - asserted as such

The alpha cases "alpha<i>" (several of K = 1, one each of K = 255, 256, 257, 1025):
  alpha<i>              (K,)     log-spaced over 0.003 .. 0.05 (K = 1: one value per case), with pairs at the threshold
                                 times (1 - 1e-6) and (1 + 1e-6) at the ends and in the middle of the vector
  alpha<i>_mortal       (K,)     exp(psi(a_k) - psi(sum a + kMortalTokens)) < kMortalT, exactly
  alpha<i>_margin       (K,)     t / kMortalT - 1 (a double): at least 1e-9 away from 0 for every alpha, asserted
"""
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np
import scipy.special

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_special_mp import pair          # noqa: E402  (the same (hi, lo) convention)

DIGITS = 60
CASES = [(1, 5), (10, 257), (16, 64), (17, 33), (33, 30), (64, 40), (65, 37), (128, 31), (257, 9), (300, 1), (1025, 5)]
ALPHA_K = (1, 1, 1, 1, 1, 1, 255, 256, 257, 1025)
MORTAL_T = 1e-33           # estep_common.h kMortalT
MORTAL_TOKENS = 8.0        # estep_common.h kMortalTokens
PSI_ROOT = 1.4616321449683623
EULER = 0.5772156649015329


def log_uniform(rng, lo, hi, size):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


def make_eta(rng, K, V):
    eta = log_uniform(rng, 1e-5, 1e6, (K, V))
    if K < 6:
        return eta, {}
    if V == 1:
        eta[1], eta[5] = eta[0], np.nextafter(eta[4], np.inf)
        return eta, {}
    words = list(rng.permutation(V))
    marks = {"tie": int(words.pop()), "last": int(words.pop())}
    if K > 64:
        marks["col63"] = int(words.pop())
    sweeps = [] if K < 17 else [(700.0, 760.0)] if K >= 40 else [(700.0, 760.0), (701.9, 758.1)]
    marks["sweep"] = [(int(words.pop()), lo, hi) for lo, hi in sweeps]
    # a word whose largest u belongs to one chosen topic: that topic's entry dominates its row, the others' are tiny
    for name, row in (("tie", 4), ("last", K - 1), ("col63", 63)):
        if name in marks:
            eta[:, marks[name]] = log_uniform(rng, 1e-5, 1e-3, K)
            eta[row, marks[name]] = rng.uniform(2e6, 4e6)
    # (a power of two and the double below it: 2^-53 apart relatively, which keeps the two u within an ulp of u)
    eta[4, marks["tie"]] = 2.0 ** 21
    # the rows of a large and of a small sum, over the words left
    eta[2, words] *= 1e9 / eta[2, words].sum()
    eta[3, words] = log_uniform(rng, 1e-5, 0.5 / V, len(words))
    # e[k] = psi(eta[k][w]) - psi(S_k) - (psi(root) - psi(S_j)) = -t_k, with psi(x) = -1 / x - gamma for small x
    j = 6
    rows = np.arange(K) != j
    for w, lo, hi in marks["sweep"]:
        eta[j, w] = PSI_ROOT + rng.uniform(-1e-3, 1e-3)
        eta[rows, w] = 1.0 / 730.0
    for _ in range(200):    # (the entries move the sum of a row whose sum is small)
        for w, lo, hi in marks["sweep"]:
            psi_s = scipy.special.digamma(eta.sum(axis=1))
            eta[rows, w] = 1.0 / (np.linspace(lo, hi, K)[rows] - psi_s[rows] + psi_s[j] - EULER)
    eta[1] = eta[0]
    eta[5] = eta[4]
    eta[5, marks["tie"]] = np.nextafter(eta[4, marks["tie"]], 0.0)
    return eta, marks


def references(eta):
    K, V = eta.shape
    sums = [mpmath.mpf(int(f.numerator)) / mpmath.mpf(int(f.denominator))
            for f in (sum((Fraction(float(v)) for v in row), Fraction(0)) for row in eta)]
    psi_sum = [mpmath.digamma(s) for s in sums]
    u = [[mpmath.digamma(mpmath.mpf(float(eta[k, w]))) - psi_sum[k] for w in range(V)] for k in range(K)]
    lse = [mpmath.log(mpmath.fsum(mpmath.exp(v) for v in row)) for row in u]
    return u, psi_sum, lse


def check_case(K, V, eta, marks, u):
    """The case holds what the docstring says it holds, by mpmath's values."""
    assert np.all(eta > 0.0) and np.all(np.isfinite(eta))
    if V == 1:
        assert all(row[0] == 0 for row in u)
        return ""
    assert all(v < 0 for row in u for v in row)
    shift = [max(u[k][w] for k in range(K)) for w in range(V)]
    b = [[mpmath.exp(u[k][w] - shift[w]) for w in range(V)] for k in range(K)]
    zeros = sum(1 for row in b for v in row if v < mpmath.mpf(2) ** -1075)
    subnormal = sum(1 for row in b for v in row if mpmath.mpf(2) ** -1075 <= v < mpmath.mpf(2) ** -1022)
    if K >= 17:
        assert zeros > 10 and subnormal > 10, (K, V, zeros, subnormal)
        for w, lo, hi in marks["sweep"]:
            e = sorted(float(u[k][w] - shift[w]) for k in range(K))
            assert abs(e[0] + hi) < 0.5 and abs(e[-2] + lo) < 0.5 and e[-1] == 0.0, (K, V, e[0], e[-2])
    if K >= 6:
        assert np.array_equal(eta[0], eta[1])
        assert 0.5e9 < eta[2].sum() < 2e9 and eta[3].sum() < 1.0
        w = marks["tie"]
        order = sorted(range(K), key=lambda k: u[k][w])
        assert set(order[-2:]) == {4, 5}
        gap = abs(u[4][w] - u[5][w])
        assert 0 < gap <= float(np.spacing(abs(float(u[4][w])))), (K, V, float(gap))
        for name, row in (("last", K - 1), ("col63", 63)):
            if name in marks:
                assert max(range(K), key=lambda k: u[k][marks[name]]) == row, (K, V, name)
    return "%d exact zeros and %d subnormals of exp(e)" % (zeros, subnormal)


def mortal_threshold(total):
    """The alpha at which exp(psi(a) - psi(total + kMortalTokens)) == kMortalT (bisection in doubles)."""
    target = mpmath.log(mpmath.mpf(MORTAL_T)) + mpmath.digamma(mpmath.mpf(total) + MORTAL_TOKENS)
    lo, hi = 0.003, 0.05
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if mpmath.digamma(mpmath.mpf(mid)) < target else (lo, mid)
    return lo


def make_alpha(index, K):
    if K == 1:
        thr = mortal_threshold(0.0132)
        for _ in range(3):
            thr = mortal_threshold(thr)
        return np.array([[0.003, 0.05, thr * (1 - 1e-6), thr * (1 + 1e-6), 0.012, 0.0145][index]])
    at = [0, 1, K // 2, K // 2 + 1, K - 2, K - 1]
    alpha = np.empty(K)
    rest = np.setdiff1d(np.arange(K), at)
    alpha[rest] = np.clip(np.exp(np.linspace(np.log(0.003), np.log(0.05), rest.size)), 0.003, 0.05)
    alpha[at] = 0.0132
    for _ in range(3):
        thr = mortal_threshold(float(alpha.sum()))
        alpha[at] = [thr * (1 - 1e-6), thr * (1 + 1e-6)] * 3
    return alpha


def classify(alpha):
    total = mpmath.fsum(mpmath.mpf(float(a)) for a in alpha)
    psi_shortest = mpmath.digamma(total + MORTAL_TOKENS)
    ratio = [mpmath.exp(mpmath.digamma(mpmath.mpf(float(a))) - psi_shortest) / mpmath.mpf(MORTAL_T) for a in alpha]
    margin = np.array([float(r - 1) for r in ratio])
    assert np.all(np.abs(margin) >= 1e-9), margin[np.abs(margin) < 1e-9]
    return np.array([r < 1 for r in ratio]), margin


def main():
    mpmath.mp.dps = DIGITS
    rng = np.random.default_rng(31)
    out = {}
    for K, V in CASES:
        eta, marks = make_eta(rng, K, V)
        u, psi_sum, lse = references(eta)
        note = check_case(K, V, eta, marks, u)
        name = "K%d_V%d" % (K, V)
        out[name + "_eta"] = eta
        for key, values, shape in (("u", [v for row in u for v in row], (K, V)), ("rowsum", psi_sum, (K,)), ("lse", lse, (K,))):
            both = np.array([pair(v) for v in values])
            out["%s_%s_hi" % (name, key)] = both[:, 0].reshape(shape).copy()
            out["%s_%s_lo" % (name, key)] = both[:, 1].reshape(shape).copy()
        print("%s: %s %s" % (name, note, {k: v for k, v in marks.items()}))
    for i, K in enumerate(ALPHA_K):
        alpha = make_alpha(i, K)
        mortal, margin = classify(alpha)
        out["alpha%d" % i], out["alpha%d_mortal" % i], out["alpha%d_margin" % i] = alpha, mortal, margin
        print("alpha%d: K = %d, %d of them mortal, closest t / kMortalT - 1 = %.2e" % (i, K, mortal.sum(), np.abs(margin).min()))
    path = os.path.join(HERE, "tables_mp.npz")
    np.savez_compressed(path, digits=DIGITS, **out)
    print("tables_mp: %d table entries, %d bytes" % (sum(K * V for K, V in CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()

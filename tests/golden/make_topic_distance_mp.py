"""Writes tests/golden/topic_distance_mp.npz: the exact Bhattacharyya coefficients and Jensen-Shannon divergences (nats)
between the rows of two tables (on the device topic_distance_kernels.h through
pylda_topic_distances), from mpmath at 50 digits.  Pure host code.

    python tests/golden/make_topic_distance_mp.py

The tables are NOT stored: tests/topic_distance_restatement.py rebuilds them from seeds (case(name)), and <case>_sha256
(32 bytes over the shapes and the doubles of both tables) ties the numbers below to the inputs they were computed from.
Per case of topic_distance_restatement.CASES, every reference a (hi, lo) pair of doubles as in make_special_mp.py - hi
the correctly rounded value, lo the correctly rounded remainder:
  <case>_bc_hi / _lo   (Ka, Kb)   sum_v sqrt(p_v q_v)
  <case>_js_hi / _lo   (Ka, Kb)   (sum_v p_v ln(p_v / m_v) + q_v ln(q_v / m_v)) / 2, m = (p + q) / 2, a term with p = 0 or
                                  q = 0 that side's 0: ln 2 for disjoint supports
All of it from the DOUBLES the device receives: p = t / sum(t) with the exact sum of the row's doubles.
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
import topic_distance_restatement as spec  # noqa: E402

DIGITS = 50


def distributions(table):
    """Per row the list of exact p_v as mpf."""
    out = []
    for row in table:
        total = sum((Fraction(float(t)) for t in row), Fraction(0))
        total = mpmath.mpf(int(total.numerator)) / mpmath.mpf(int(total.denominator))
        out.append([mpmath.mpf(float(t)) / total for t in row])
    return out


def references(a, b):
    """(bc, js) as (Ka, Kb) lists of mpf"""
    pa, pb = distributions(a), distributions(b)
    root = lambda rows: [[mpmath.sqrt(p) for p in row] for row in rows]
    plogp = lambda rows: [[p * mpmath.log(p) if p > 0 else mpmath.mpf(0) for p in row] for row in rows]
    ra, rb, ea, eb = root(pa), root(pb), plogp(pa), plogp(pb)
    bc, js = [], []
    for i in range(len(pa)):
        for j in range(len(pb)):
            bc.append(mpmath.fsum(x * y for x, y in zip(ra[i], rb[j])))
            js.append(mpmath.mpf(0.5) * mpmath.fsum(e + f - (p + q) * mpmath.log((p + q) / 2) if p + q > 0 else mpmath.mpf(0)
                                  for p, q, e, f in zip(pa[i], pb[j], ea[i], eb[j])))
    return bc, js


def main():
    mpmath.mp.dps = DIGITS
    out = {}
    pair_words = 0
    for name in spec.CASES:
        a, b = spec.case(name)
        out[name + "_sha256"] = spec.digest(a, b)
        for key, numbers in zip(("bc", "js"), references(a, b)):
            both = np.array([pair(v) for v in numbers], dtype=np.float64).reshape(len(a), len(b), 2)
            out["%s_%s_hi" % (name, key)] = both[:, :, 0].copy()
            out["%s_%s_lo" % (name, key)] = both[:, :, 1].copy()
        pair_words += len(a) * len(b) * a.shape[1]
        print("%s: Ka = %d, Kb = %d, V = %d, BC[0][0] %.17g, JS[0][0] %.17g"
              % (name, len(a), len(b), a.shape[1], out[name + "_bc_hi"][0, 0], out[name + "_js_hi"][0, 0]))
    path = os.path.join(HERE, "topic_distance_mp.npz")
    np.savez_compressed(path, digits=DIGITS, **out)
    print("topic_distance_mp: %d cases, %d pair-words, %d bytes" % (len(spec.CASES), pair_words, os.path.getsize(path)))


if __name__ == "__main__":
    main()

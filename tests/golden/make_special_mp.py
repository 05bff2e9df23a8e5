"""Writes tests/golden/special_mp.npz: high-precision references for the device special functions
(pylda_amd/csrc/special_device.h), from mpmath at 60 digits.

    python tests/golden/make_special_mp.py

Every reference is a PAIR of doubles (hi, lo): hi is the correctly rounded value (subnormals included), lo the
correctly rounded remainder value - hi, so hi + lo carries ~106 bits and the GPU test needs no mpmath:
it forms an error as (got - hi) - lo.  tests/test_special_golden.py recomputes a spread of the pairs.

Arrays (x: the points, *_hi / *_lo: the pairs)
  sp_x, psi_*, lgam_*       digamma and ln Gamma: log-uniform over 2.3e-308 .. 1e-6 .. 1e4 .. 1e15 and the branch set
  tg_x, tg_*                trigamma: log-uniform over 1e-150 .. 1e15 (below that the value overflows) and the branch set
  fx_x, fx_psi, fx_c, fx_hi, fx_lo   exp(psi(x) - c), c in fx_c (rows of fx_hi / fx_lo): 1e-4 .. 1e15, the branch set
                            without (0.9, 2.1), and 1e24 .. 1e30 (the level-ordered form clamps its shift at 1e25)
  uf_x, uf_psi, uf_c, uf_hi, uf_lo   the same on a dense sorted grid of [1.30e-3, 1.45e-3]: the result goes through
                            the subnormals to 0
  tiny_x                    arguments whose exp(psi(x) - c) is below half the smallest subnormal for every c >= 0: exactly 0
  ex_x, ex_*                exp: uniform over [-745, 700] and arguments within 4 ulp of (k + 1/2) ln 2, the rounding
                            boundary of the argument reduction
  rc_x, rc_*                1 / x: log-uniform over 1e-300 .. 1e300
The branch set: uniform over (0, 14); n - 2 ulp .. n + 2 ulp for n = 1 .. 13 (digamma branches at 10, lgamma_pos and
the trigamma loop at 12, the loop's trip count changes at every integer) and for the root of psi; 300 points of
(0.9, 2.1), where ln Gamma crosses zero twice.
"""
import os
from fractions import Fraction

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DIGITS = 60
PSI_ROOT = 1.4616321449683623
FUSED_C = (0.0, 3.5, -1.25, 9.0, 23.0)
UNDERFLOW_C = (0.0, 9.0)
TINY_X = (1e-300, 1e-250, 1e-170, 1e-100, 1e-60, 1e-40, 1e-20, 1e-10, 1e-5)


def exact(v):
    """The mpf as an exact fraction."""
    sign, man, exp, _ = v._mpf_
    f = Fraction(int(man)) * (Fraction(2) ** exp if exp >= -4000 else Fraction(0))
    return -f if sign else f


def pair(v):
    """(hi, lo) of an mpf: float(Fraction) rounds correctly, subnormals included."""
    f = exact(v)
    hi = float(f)
    return hi, float(f - Fraction(hi))


def pairs(fn, xs):
    out = np.array([pair(fn(mpmath.mpf(float(x)))) for x in xs])
    return out[:, 0].copy(), out[:, 1].copy()


def ulp_neighbours(v):
    out = [v]
    lo = hi = v
    for _ in range(2):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return sorted(out)


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def branch_set(rng, uniform, with_lgamma_zeros=True):
    pts = [rng.uniform(0.0, 14.0, uniform) + 1e-12]
    for n in range(1, 14):
        pts.append(ulp_neighbours(float(n)))
    pts.append(ulp_neighbours(PSI_ROOT))
    if with_lgamma_zeros:
        pts.append(rng.uniform(0.9, 2.1, 300))
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in pts])


def fused(x, c):
    return mpmath.exp(mpmath.digamma(x) - mpmath.mpf(c))


def main():
    mpmath.mp.dps = DIGITS
    rng = np.random.default_rng(20)
    out = {}

    sp_x = np.concatenate([log_uniform(rng, 2.3e-308, 1e-6, 400), log_uniform(rng, 1e-6, 1e4, 400),
                           log_uniform(rng, 1e4, 1e15, 400), branch_set(rng, 600)])
    out["sp_x"] = sp_x
    out["psi_hi"], out["psi_lo"] = pairs(mpmath.digamma, sp_x)
    out["lgam_hi"], out["lgam_lo"] = pairs(mpmath.loggamma, sp_x)

    tg_x = np.concatenate([log_uniform(rng, 1e-150, 1e15, 800), branch_set(rng, 600)])
    out["tg_x"] = tg_x
    out["tg_hi"], out["tg_lo"] = pairs(lambda v: mpmath.polygamma(1, v), tg_x)

    fx_x = np.concatenate([log_uniform(rng, 1e-4, 1e4, 400), log_uniform(rng, 1e4, 1e15, 200),
                           branch_set(rng, 300, with_lgamma_zeros=False), [1e24, 1e25, 1e26, 1e30]])
    uf_x = np.sort(rng.uniform(1.30e-3, 1.45e-3, 2000))
    for name, x, cs in (("fx", fx_x, FUSED_C), ("uf", uf_x, UNDERFLOW_C)):
        out[name + "_x"], out[name + "_c"] = x, np.array(cs)
        out[name + "_psi"] = np.array([float(mpmath.digamma(mpmath.mpf(float(v)))) for v in x])
        both = [pairs(lambda v: fused(v, c), x) for c in cs]
        out[name + "_hi"] = np.array([b[0] for b in both])
        out[name + "_lo"] = np.array([b[1] for b in both])
    # the grid starts at an exact 0 and ends among the normal numbers, for both c
    assert np.all(out["uf_hi"][:, 0] == 0.0) and np.all(out["uf_hi"][:, -1] > 2.0 ** -1022)
    for v in TINY_X:
        assert mpmath.digamma(mpmath.mpf(v)) < -1e5 and fused(mpmath.mpf(v), 0.0) < mpmath.mpf(2) ** -1076
    out["tiny_x"] = np.array(TINY_X)

    ln2 = mpmath.log(2)
    ks = rng.integers(-1021, 1009, 200)
    near = np.array([float((int(k) + mpmath.mpf(0.5)) * ln2) for k in ks])
    for _ in range(4):          # 0 .. 4 ulp to either side
        step = rng.integers(-1, 2, near.size)
        near = np.where(step < 0, np.nextafter(near, -np.inf), np.where(step > 0, np.nextafter(near, np.inf), near))
    ex_x = np.concatenate([rng.uniform(-745.0, 700.0, 1000), near])
    out["ex_x"] = ex_x
    out["ex_hi"], out["ex_lo"] = pairs(mpmath.exp, ex_x)

    rc_x = log_uniform(rng, 1e-300, 1e300, 1000)
    out["rc_x"] = rc_x
    out["rc_hi"], out["rc_lo"] = pairs(lambda v: 1 / v, rc_x)

    path = os.path.join(HERE, "special_mp.npz")
    np.savez_compressed(path, digits=DIGITS, **out)
    print("special_mp: %s, %d bytes" % (", ".join("%s %d" % (k, out[k].size) for k in ("sp_x", "tg_x", "fx_x", "uf_x", "ex_x", "rc_x")),
                                        os.path.getsize(path)))


if __name__ == "__main__":
    main()

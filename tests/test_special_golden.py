"""tests/golden/special_mp.npz is what tests/test_gpu_special.py measures the device special functions against: here
the file itself is checked (against mpmath, where that is installed), and the C oracle's digamma / trigamma / lgamma are
held to the bounds the device functions are held to, on the same points.  CPU only."""
import numpy as np
import pytest
import scipy.special

from conftest import load_golden
from oracle import c_oracle
from special_bounds import (DIGAMMA_SCALED, LGAMMA_SCALED, MIN_NORMAL, TRIGAMMA_OVER_SCIPY, pair_error, scaled_error,
                            relative_error)

# name of the points, of the pair, the function in mpmath's terms
FUNCTIONS = [("sp_x", "psi", "digamma"), ("sp_x", "lgam", "loggamma"), ("tg_x", "tg", "trigamma"), ("ex_x", "ex", "exp"),
             ("rc_x", "rc", "reciprocal")]


@pytest.fixture(scope="module")
def golden():
    return load_golden("special_mp.npz")


def test_pairs_are_normalised(golden):
    """hi is the rounded value and lo the remainder: |lo| <= ulp(hi) / 2; the points
    are normal positive doubles (exp's arguments apart)."""
    g = golden
    for xs, name in [(f[0], f[1]) for f in FUNCTIONS] + [("fx_x", "fx"), ("uf_x", "uf")]:
        hi, lo = g[name + "_hi"], g[name + "_lo"]
        assert hi.shape == lo.shape and hi.shape[-1] == g[xs].size
        assert np.all(np.isfinite(hi)) and np.all(np.isfinite(lo))
        assert np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi))), name
        if xs != "ex_x":
            assert np.all(g[xs] >= MIN_NORMAL), xs
    assert np.all(np.diff(g["uf_x"]) > 0.0)
    # the dense grid takes exp(psi(x) - c) from an exact 0 through the subnormals to the normal numbers
    for row in g["uf_hi"]:
        assert row[0] == 0.0 and row[-1] > MIN_NORMAL and np.all(np.diff(row) >= 0.0)
        assert np.sum((row > 0.0) & (row < MIN_NORMAL)) > 300


def test_pairs_against_mpmath(golden):
    """A spread of the stored pairs, recomputed: hi + lo within 1e-30 relative of mpmath's value at 50 digits, plus half a
    subnormal spacing (what lo itself is rounded to where the value is tiny)."""
    mpmath = pytest.importorskip("mpmath")
    g = golden
    mpmath.mp.dps = 50
    fns = {"digamma": mpmath.digamma, "loggamma": mpmath.loggamma, "trigamma": lambda v: mpmath.polygamma(1, v),
           "exp": mpmath.exp, "reciprocal": lambda v: 1 / v}
    checked = 0

    def check(x, hi, lo, fn):
        want = fn(mpmath.mpf(float(x)))
        got = mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))
        assert abs(got - want) <= mpmath.mpf("1e-30") * abs(want) + mpmath.mpf(2) ** -1075, (float(x), float(hi), float(lo))
        return 1

    for xs, name, fn in FUNCTIONS:
        x, hi, lo = g[xs], g[name + "_hi"], g[name + "_lo"]
        # every 11th of the samples and every one of the ulp neighbours (they differ from an integer by ~1e-16)
        near = np.nonzero((np.abs(x - np.rint(x)) < 1e-13) & (x > 0.5) & (x < 13.5))[0] if xs != "ex_x" and xs != "rc_x" else []
        for i in sorted(set(range(0, x.size, 11)) | set(int(j) for j in near)):
            checked += check(x[i], hi[i], lo[i], fns[fn])
    for name in ("fx", "uf"):
        x = g[name + "_x"]
        for row, c in enumerate(g[name + "_c"]):
            for i in range(row, x.size, 13):
                checked += check(x[i], g[name + "_hi"][row, i], g[name + "_lo"][row, i],
                                 lambda v: mpmath.exp(mpmath.digamma(v) - mpmath.mpf(float(c))))
        # (fx_psi / uf_psi only scale the fused forms' bound)
        for i in range(0, x.size, 50):
            assert abs(mpmath.mpf(float(g[name + "_psi"][i])) - mpmath.digamma(mpmath.mpf(float(x[i])))) <= 1e-15 * max(
                1.0, abs(float(g[name + "_psi"][i])))
    for v in g["tiny_x"]:
        assert mpmath.exp(mpmath.digamma(mpmath.mpf(float(v)))) < mpmath.mpf(2) ** -1076
    assert checked >= 500, checked


def test_c_oracle_special_functions_against_the_golden(golden):
    """The C oracle's digamma / trigamma / lgamma (what every E-step parity test compares with) on the golden's
    points, under the bounds tests/test_gpu_special.py holds the device functions to."""
    g = golden
    x = g["sp_x"]
    dg = scaled_error(c_oracle.digamma(x), g["psi_hi"], g["psi_lo"])
    lg = scaled_error(c_oracle.lgamma(x), g["lgam_hi"], g["lgam_lo"])
    tg = relative_error(c_oracle.trigamma(g["tg_x"]), g["tg_hi"], g["tg_lo"])
    scipy_tg = relative_error(scipy.special.polygamma(1, g["tg_x"]), g["tg_hi"], g["tg_lo"])
    print("C oracle against the golden: digamma %.2e at x = %r, lgamma %.2e at x = %r, trigamma %.2e at x = %r "
          "(scipy.special.polygamma %.2e)" % (dg.max(), x[dg.argmax()], lg.max(), x[lg.argmax()], tg.max(),
                                              g["tg_x"][tg.argmax()], scipy_tg.max()))
    assert dg.max() < DIGAMMA_SCALED
    assert lg.max() < LGAMMA_SCALED
    assert tg.max() < TRIGAMMA_OVER_SCIPY * scipy_tg.max()
    assert np.array_equal(pair_error(g["psi_hi"], g["psi_hi"], g["psi_lo"]), -g["psi_lo"])

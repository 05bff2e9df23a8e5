"""Bounds and error measures shared by tests/test_special_golden.py (the C oracle) and tests/test_gpu_special.py (the
device functions), both against the (hi, lo) pairs of tests/golden/special_mp.npz."""
import numpy as np

MIN_NORMAL = 2.0 ** -1022
SUBNORMAL_SPACING = 2.0 ** -1074

DIGAMMA_SCALED = 5e-15        # |error| / max(1, |psi|)
LGAMMA_SCALED = 5e-14         # |error| / max(1, |ln Gamma|): two values near 21 cancel around x = 1.45
TRIGAMMA_OVER_SCIPY = 8.0     # relative error, in units of scipy.special.polygamma(1, x)'s worst on the same points
EXP_SHALLOW_ULP = 4.0         # results >= MIN_NORMAL
RCP_NEWTON_ULP = 1.0


def fused_bound(psi, c):
    """Relative bound of exp(psi(x) - c): the exponent carries ~1 ulp of its own magnitude."""
    return 2e-15 * (4.0 + np.abs(psi - c))


def pair_error(got, hi, lo):
    """got - (hi + lo), formed so that the remainder counts: (got - hi) is exact for got near hi."""
    return (got - hi) - lo


def scaled_error(got, hi, lo):
    return np.abs(pair_error(got, hi, lo)) / np.maximum(1.0, np.abs(hi))


def relative_error(got, hi, lo):
    return np.abs(pair_error(got, hi, lo)) / np.abs(hi)


def ulp_error(got, hi, lo):
    """In units of the spacing of doubles at the reference."""
    return np.abs(pair_error(got, hi, lo)) / np.spacing(np.abs(hi))

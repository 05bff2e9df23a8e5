"""The M-step's two reductions (variational_bayes.py:222-233) in plain fp64 with exact sums: what the device M-step
(pylda_amd/csrc/mstep_kernels.h) is compared against in tests/test_gpu_mstep.py.

It shares no code with the kernels or with oracle/vb_numpy.py: scipy's psi / gammaln per element, and every sum - the row
sums of gamma and eta that feed psi(sum) and lnG(sum) included - through math.fsum, which rounds the exact sum once.

Each value comes with its SCALE, the sum over its terms of max(1, |term|): the denominator tests/test_gpu_estep.py::
test_device_special_functions holds the device's psi and lnG to, per element.  A comparison |device - reference| <=
tolerance * scale is therefore a statement about the worst term, not about a sum in which the terms may have cancelled.
The smallest |term| is returned too: a test whose smallest term is well above its tolerance cannot lose, double or
misplace a single element unnoticed.  tests/test_mstep_reference.py pins this module to mpmath at 40 digits.  Pure host code."""
import math

import numpy as np
from scipy.special import gammaln, psi

TOLERANCE = 1e-13       # of the scale; derived in tests/test_gpu_mstep.py


class Reduced(object):
    """value, scale = sum of max(1, |term|), smallest = min |term| (inf without terms); arrays for a vector of values."""

    def __init__(self, value, scale, smallest):
        self.value, self.scale, self.smallest = value, scale, smallest

    def error_of(self, got):
        """Largest |got - value| / scale."""
        err = np.abs(np.asarray(got, dtype=np.float64) - self.value) / self.scale
        return float(np.max(err)) if np.size(err) else 0.0

    def terms_stand_out(self, tolerance=TOLERANCE):
        """The condition on the inputs: every term is at least ten times what the comparison lets through."""
        return bool(np.all(self.smallest >= 10.0 * tolerance * self.scale))


def _reduce(terms):
    """One value from a flat sequence of terms."""
    mag = np.abs(terms)
    return math.fsum(terms), math.fsum(np.maximum(1.0, mag)), float(mag.min()) if len(terms) else math.inf


def alpha_statistics(gamma):
    """Sum over the documents of psi(gamma_dk) - psi(sum_k gamma_dk) (:232-233), one Reduced of K-vectors.
    The terms of topic k: psi(gamma_dk) and -psi(sum_k gamma_dk), over the documents."""
    gamma = np.asarray(gamma, dtype=np.float64)
    D, K = gamma.shape
    if D == 0:
        return Reduced(np.zeros(K), np.ones(K), np.full(K, math.inf))
    row_sum = np.array([math.fsum(row) for row in gamma])
    minus_psi_sum = -psi(row_sum)
    psi_gamma = psi(gamma)
    out = [_reduce(np.concatenate([psi_gamma[:, k], minus_psi_sum])) for k in range(K)]
    return Reduced(*(np.array(x) for x in zip(*out)))


def topic_log_likelihood(eta, beta):
    """K (lnG(sum beta) - sum_v lnG(beta_v)) + sum_k (sum_v lnG(eta_kv) - lnG(sum_v eta_kv)) (:222-224) of the eta the
    M-step finds in place.  The terms: every lnG(eta_kv), every -lnG(sum_v eta_kv), K lnG(sum beta), every -K lnG(beta_v)."""
    eta = np.asarray(eta, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    K = eta.shape[0]
    row_sum = np.array([math.fsum(row) for row in eta])
    terms = np.concatenate([gammaln(eta).ravel(), -gammaln(row_sum), [K * gammaln(math.fsum(beta))], -K * gammaln(beta)])
    return Reduced(*_reduce(terms))

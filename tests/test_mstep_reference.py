"""tests/mstep_reference.py, the yardstick of tests/test_gpu_mstep.py, against mpmath at 40 digits - two orders below
the tolerance the GPU tests hold the kernels to.  No GPU."""
import math

import numpy as np

import mstep_reference as ref


def log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(math.log(lo), math.log(hi), shape))


def test_alpha_statistics_against_mpmath():
    import mpmath
    mpmath.mp.dps = 40
    rng = np.random.default_rng(0)
    gamma = log_uniform(rng, 1e-3, 1e4, (3000, 3))
    got = ref.alpha_statistics(gamma)
    mp = [[mpmath.mpf(float(x)) for x in row] for row in gamma]
    psi_sum = [mpmath.digamma(mpmath.fsum(row)) for row in mp]
    for k in range(3):
        terms = [mpmath.digamma(row[k]) for row in mp] + [-p for p in psi_sum]
        want = mpmath.fsum(terms)
        scale = mpmath.fsum(max(mpmath.mpf(1), abs(t)) for t in terms)
        assert abs(mpmath.mpf(float(got.value[k])) - want) <= 1e-15 * scale, k
        assert abs(mpmath.mpf(float(got.scale[k])) - scale) <= 1e-12 * scale, k
        assert abs(mpmath.mpf(float(got.smallest[k])) - min(abs(t) for t in terms)) <= 1e-12, k
    assert got.terms_stand_out(1e-16) and not got.terms_stand_out(1e-3)


def test_topic_log_likelihood_against_mpmath():
    import mpmath
    mpmath.mp.dps = 40
    rng = np.random.default_rng(1)
    K, V = 5, 2049
    eta = log_uniform(rng, 1e-5, 1e6, (K, V))
    beta = rng.uniform(0.01, 0.5, V)
    got = ref.topic_log_likelihood(eta, beta)
    mp_beta = [mpmath.mpf(float(b)) for b in beta]
    terms = [K * mpmath.loggamma(mpmath.fsum(mp_beta))] + [-K * mpmath.loggamma(b) for b in mp_beta]
    for row in eta:
        mp_row = [mpmath.mpf(float(x)) for x in row]
        terms += [mpmath.loggamma(x) for x in mp_row] + [-mpmath.loggamma(mpmath.fsum(mp_row))]
    want = mpmath.fsum(terms)
    scale = mpmath.fsum(max(mpmath.mpf(1), abs(t)) for t in terms)
    assert len(terms) == K * V + K + 1 + V
    assert abs(mpmath.mpf(got.value) - want) <= 1e-15 * scale
    assert abs(mpmath.mpf(got.scale) - scale) <= 1e-12 * scale
    assert abs(mpmath.mpf(got.smallest) - min(abs(t) for t in terms)) <= 1e-12


def test_terms_scales_and_the_comparison_by_hand():
    # two documents, two topics: psi(1) = -gamma_E, psi(2) = 1 - gamma_E, psi(3) = 1.5 - gamma_E, psi(4) = 11/6 - gamma_E
    e = 0.5772156649015329
    got = ref.alpha_statistics(np.array([[1.0, 2.0], [2.0, 2.0]]))
    assert np.allclose(got.value, [(-e - (1.5 - e)) + ((1 - e) - (11 / 6 - e)), 2 * (1 - e) - (1.5 - e) - (11 / 6 - e)], rtol=0, atol=1e-15)
    assert np.allclose(got.scale, [4 + (11 / 6 - e - 1), 4 + (11 / 6 - e - 1)], rtol=0, atol=1e-15)      # only psi(4) exceeds 1
    assert np.allclose(got.smallest, [1 - e, 1 - e], rtol=0, atol=1e-15)
    assert abs(got.error_of(got.value + np.array([0.0, 1e-3])) - 1e-3 / got.scale[1]) < 1e-15
    # no documents: exact zeros, and a scale under which nothing but zero passes
    none = ref.alpha_statistics(np.zeros((0, 4)))
    assert np.array_equal(none.value, np.zeros(4)) and none.error_of(np.zeros(4)) == 0.0 and none.terms_stand_out()
    # lnG(1) = lnG(2) = 0, lnG(3) = ln 2, lnG(6) = ln 120: one topic, eta = (3, 3), beta = (1, 2)
    t = ref.topic_log_likelihood(np.array([[3.0, 3.0]]), np.array([1.0, 2.0]))
    assert abs(t.value - (2 * math.log(2) - math.log(120) + math.log(2))) < 1e-15
    assert t.smallest == 0.0 and not t.terms_stand_out()                      # lnG(beta) = 0: such inputs are refused
    assert abs(t.scale - (6 + math.log(120) - 1)) < 1e-14

"""The device M-step stage (pylda_amd/csrc/mstep_kernels.h, mstep_api.hip, the transposes of context.hip) at the shapes
where its kernels branch, against tests/mstep_reference.py.  Needs an MI355X.

What the shapes reach (launch arithmetic of mstep_api.hip: min(1024, ceil(D / 4)) workgroups of four wavefronts, a
wavefront takes documents d and d + stride per trip, stride = 4 * workgroups, trips 2 * stride apart):

    D <= 4096    no pair                              D = 8192    only pairs
    D = 4097     one pair, 4095 singles               D = 8193    one wavefront makes a second trip, with a single
    D = 12289    every wavefront makes two trips: 4097 pairs and 4095 singles
    K = 65, 130  two and three `k += 64` trips per lane; K = 2100: 67 200 bytes of dynamic LDS, above the 64 KiB default
    (K, V) of test_eta_update_and_transposes: table strides 16, 32, 64, 128, 256, 384 and 1088, tiles past a full
    32 x 32 tile in K and in V, V < 8 (empty chunks of the topic term), V no multiple of 8, chunks above 256 words

One tolerance for the alpha statistics and the topic log-likelihood, derived and not tuned: |device - reference| <=
1e-13 * scale, scale = the sum over the value's terms of max(1, |term|).  test_device_special_functions holds the
device's psi to 5e-15 and lnG to 5e-14 of max(1, |value|) per element, which bounds the sum of the terms' errors by
5e-14 * scale; the kernels' fixed-order sums add at most about 260 sequential fp64 additions to a value of the alpha
statistics (256 partial rows per column group in column_sum_kernel, the wave and workgroup levels) and about
V / 2048 + 18 + K to the topic term: for the shapes here below 4e-14 of the scale.  Every such test also asserts, from
the reference alone, that the smallest |term| of its inputs is at least ten times what the comparison lets through: one
dropped, doubled or misplaced element cannot hide.  What was observed is recorded in LABNOTES.md, not folded back into
the bound.  eta <- sstats + beta and the transposes are compared bit for bit: one fp64 addition has one correct result."""
import math

import numpy as np
import pytest

import mstep_reference as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = ref.TOLERANCE
V_CORPUS = 40


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    _capi.load()
    assert _capi.device_count() >= 1, "no HIP device visible"
    return _capi


def synthetic_corpus(D=12289, V=V_CORPUS, seed=0):
    """D documents of one to three distinct terms with counts of 1 ... 2000, log-uniform: gamma spans orders of magnitude."""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 4, D)
    drawn = rng.random((D, V)).argsort(axis=1)[:, :3]
    drawn[np.arange(3)[None, :] >= n[:, None]] = V           # unused slots sort to the end
    drawn.sort(axis=1)
    ids = drawn[drawn < V].astype(np.int32)                  # row-major: document after document, ids ascending
    ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    cts = np.minimum(2000, np.exp(rng.uniform(0.0, math.log(2001.0), ids.size))).astype(np.int32)
    assert ids.size == ptr[-1] and cts.min() >= 1 and cts.max() > 1000
    return ptr, ids, cts


@pytest.fixture(scope="module")
def corpus12289():
    return synthetic_corpus()


def prefix(csr, D):
    ptr, ids, cts = csr
    return ptr[:D + 1], ids[:ptr[D]], cts[:ptr[D]]


def model(K, V=V_CORPUS):
    """Mixed alpha in 0.01 ... 2, the reference's initial eta (variational_bayes.py:95), a beta with no two values alike."""
    rng = np.random.default_rng(1000 + K)
    return rng.uniform(0.01, 2.0, K), rng.gamma(100.0, 0.01, (K, V)), rng.uniform(0.3, 0.65, V)


def eta_off_the_zeros(rng, shape, lo, hi):
    """Log-uniform over lo ... hi without (0.8, 2.2): lnG vanishes at 1 and 2, and a term that is nearly zero could be
    lost without a trace."""
    eta = np.exp(rng.uniform(math.log(lo), math.log(hi), shape))
    inside = (eta > 0.8) & (eta < 2.2)
    eta[inside] *= 3.0                                        # 2.4 ... 6.6
    return eta


def check(name, reduced, got):
    """|got - reference| <= TOL * scale, after the condition on the inputs; the figure is printed for LABNOTES.md."""
    assert reduced.terms_stand_out(TOL), "%s: a term of these inputs is too small for the comparison to see it" % name
    err = reduced.error_of(got)
    print("%s: |device - reference| / scale = %.2e" % (name, err))
    assert err <= TOL, (name, err)


# ---- 1. alpha sufficient statistics at the branch points of mstep_alpha_ss_kernel ----
@pytest.mark.parametrize("K,D", [(3, D) for D in (0, 1, 3, 4, 5, 4096, 4097, 8192, 8193, 12289)] + [(65, 8193), (130, 8193)])
def test_alpha_statistics_at_the_branch_points(capi, corpus12289, K, D):
    alpha, eta, beta = model(K)
    ctx = capi.Context(K, V_CORPUS)
    ctx.set_alpha(alpha)
    ctx.set_eta(eta)
    corpus = ctx.corpus(*prefix(corpus12289, D))
    ctx.estep(corpus)
    gamma = np.array(ctx.get_gamma(corpus))
    _, stats = ctx.mstep(corpus, beta)
    _, again = ctx.mstep(corpus, beta)          # (eta has moved on; gamma, all these statistics read, has not)
    corpus.close()
    ctx.close()
    assert gamma.shape == (D, K) and np.all(np.isfinite(gamma)) and np.all(gamma > 0)
    assert np.array_equal(stats, again)         # fixed document -> workgroup assignment, fixed order of summation
    if D == 0:
        assert np.array_equal(stats, np.zeros(K))
        return
    if D >= 4096:
        assert gamma.max() / gamma.min() > 1e3
    check("alpha statistics K=%d D=%d" % (K, D), ref.alpha_statistics(gamma), stats)


# ---- 2. eta <- sstats + beta and the two transposes, bit for bit; the topic term of the pre-update eta ----
SHAPES = [(1, 1), (1, 9), (7, 8), (31, 33), (32, 32), (33, 31), (65, 95), (129, 70), (257, 40), (1030, 37), (5, 2049), (3, 4097)]


def table_inputs(K, V):
    rng = np.random.default_rng(K * 10007 + V)
    sstats = rng.gamma(0.5, 20.0, (K, V))
    eta = eta_off_the_zeros(rng, (K, V), 1e-5, 1e6 if K * V < 1000 else 1e4)
    beta = rng.uniform(0.3, 0.65, V)
    assert np.unique(sstats).size == K * V and np.unique(beta).size == V and np.all(sstats > 0)
    return sstats, eta, beta


@pytest.mark.parametrize("K,V", SHAPES)
def test_eta_update_and_transposes(capi, K, V):
    sstats, eta, beta = table_inputs(K, V)
    ctx = capi.Context(K, V)
    stride = ctx.sstats_elements() // V
    assert stride == {1: 16, 7: 16, 31: 32, 32: 32, 33: 64, 65: 128, 129: 256, 257: 384, 1030: 1088, 5: 16, 3: 16}[K]
    ctx.set_sstats(sstats)
    assert np.array_equal(ctx.get_sstats(), sstats)           # (K, V) -> (V, stride) -> (K, V)
    ctx.set_eta(eta)
    topic_ll, _ = ctx.mstep(None, beta, want_alpha_ss=False)
    updated = np.array(ctx.get_eta())
    # (the export's staging buffer still holds what set_sstats was handed: halve the table in place - exact - so that
    #  an export that moved nothing, or not all of it, cannot return the right answer)
    ctx.hybrid_scale_sstats(2.0)
    halved = np.array(ctx.get_sstats())
    ctx.close()
    assert np.array_equal(updated, sstats + beta)
    assert np.array_equal(halved, sstats / 2)
    check("topic term K=%d V=%d" % (K, V), ref.topic_log_likelihood(eta, beta), topic_ll)


# ---- 3. K above 2048: the alpha statistics kernel asks for more than 64 KiB of dynamic LDS ----
def test_m_step_above_2048_topics(capi):
    K, V = 2100, 64
    rng = np.random.default_rng(2100)
    alpha = rng.uniform(0.01, 2.0, K)
    eta = eta_off_the_zeros(rng, (K, V), 0.05, 50.0)
    beta = rng.uniform(0.3, 0.65, V)
    ptr = np.array([0, 1, 3, 6, 7, 9, 12], np.int64)
    ids = np.array([5, 0, 63, 1, 2, 40, 17, 8, 9, 30, 31, 62], np.int32)
    cts = np.array([1, 3, 700, 2, 2, 2, 1999, 10, 1, 4, 50, 6], np.int32)
    assert 4 * K * 8 > 64 * 1024
    ctx = capi.Context(K, V)
    ctx.set_alpha(alpha)
    ctx.set_eta(eta)
    corpus = ctx.corpus(ptr, ids, cts)
    ctx.estep(corpus)
    gamma = np.array(ctx.get_gamma(corpus))
    sstats = np.array(ctx.get_sstats())
    topic_ll, stats = ctx.mstep(corpus, beta)
    updated = np.array(ctx.get_eta())
    corpus.close()
    ctx.close()
    assert np.all(np.isfinite(gamma)) and np.all(gamma > 0) and abs(sstats.sum() - cts.sum()) < 1e-8
    check("alpha statistics K=2100", ref.alpha_statistics(gamma), stats)
    check("topic term K=2100", ref.topic_log_likelihood(eta, beta), topic_ll)
    assert np.array_equal(updated, sstats + beta)


# ---- 4. the beta cache of enqueue_mstep, and mstep_enqueue + outer_fetch against mstep ----
def test_beta_cache_follows_the_values_it_is_handed(capi):
    K, V = 33, 70
    rng = np.random.default_rng(4)
    # sstats below 0.05 or above 3: sstats + beta stays off the zeros of lnG for both betas
    sstats = np.where(rng.random((K, V)) < 0.5, np.exp(rng.uniform(math.log(1e-3), math.log(0.05), (K, V))),
                      np.exp(rng.uniform(math.log(3.0), math.log(1e4), (K, V))))
    eta = eta_off_the_zeros(rng, (K, V), 1e-3, 1e4)
    beta_a = rng.uniform(0.3, 0.65, V)
    beta_b = beta_a.copy()
    beta_b[41] += 0.03125                                     # one element apart
    ctx = capi.Context(K, V)
    ctx.set_sstats(sstats)
    ctx.set_eta(eta)
    in_place = eta
    for call, beta in enumerate((beta_a, beta_b, beta_a)):
        topic_ll, _ = ctx.mstep(None, beta, want_alpha_ss=False)
        check("topic term, call %d of the beta sequence" % call, ref.topic_log_likelihood(in_place, beta), topic_ll)
        in_place = np.array(ctx.get_eta())
        assert np.array_equal(in_place, sstats + beta), call
    ctx.close()


def test_enqueued_m_step_returns_what_the_waited_one_does(capi, corpus12289):
    K, D = 3, 4097
    alpha, eta, beta = model(K)
    got = []
    for enqueued in (False, True):
        ctx = capi.Context(K, V_CORPUS)
        ctx.set_alpha(alpha)
        ctx.set_eta(eta)
        corpus = ctx.corpus(*prefix(corpus12289, D))
        ctx.estep(corpus)
        if enqueued:
            ctx.mstep_enqueue(corpus, beta, hyper_parameter_iteration=0)
            _, docs, _, topic_ll, stats, alpha_back = ctx.outer_fetch()
            assert docs == D and np.array_equal(alpha_back, alpha)
        else:
            topic_ll, stats = ctx.mstep(corpus, beta)
        got.append((topic_ll, stats, np.array(ctx.get_eta())))
        corpus.close()
        ctx.close()
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])
    assert np.all(got[0][1] < 0)


# ---- 6. whole outer iterations at a document count that takes the paired branch ----
def test_outer_iterations_beyond_4096_documents(corpus12289):
    """E-step, pack, Newton update and the next iteration's alpha meet here at D = 8200; the tolerances are those
    test_hundred_iteration_trace_and_heldout holds for the associated-press trace."""
    from oracle import c_oracle, vb_numpy
    from pylda_amd.variational_bayes import VariationalBayes
    D, K, V = 8200, 5, V_CORPUS
    ptr, ids, cts = prefix(corpus12289, D)
    eta = np.random.default_rng(6).gamma(100.0, 0.01, (K, V))
    m = VariationalBayes()
    m._verbose = False
    m._initialize_parsed(ptr, ids, cts, V, K, 1.0 / K, 1.0 / V, eta=eta.copy())
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    for it in range(3):
        e = c_oracle.e_step(alpha, eta, ptr, ids, cts)
        topic_ll, stats, eta = vb_numpy.m_step(eta, beta, e["sstats"], e["gamma"])
        alpha = vb_numpy.optimize_hyperparameters(alpha, stats, D)
        want = e["document_log_likelihood"] + topic_ll
        joint = m.learning()
        print("iteration %d: joint log-likelihood relative difference %.2e" % (it, abs(joint - want) / abs(want)))
        assert abs(joint - want) < 1e-7 * abs(want), (it, joint, want)
    print("alpha %.2e, eta %.2e" % (rel_err(m._alpha_alpha, alpha), rel_err(m._eta, eta)))
    assert rel_err(m._alpha_alpha, alpha) < 1e-6
    assert rel_err(m._eta, eta) < 1e-10

"""The collapsed Gibbs engine's log posterior on the GPU (estep_gibbs.h: gibbs_doc_posterior_kernel,
gibbs_word_posterior_kernel, gibbs_posterior_sum_kernel; gibbs_exchange.h: gibbs_posterior_parts_kernel) term by term
against mpmath (tests/golden/posterior_mp.npz) on the grid of tests/posterior_cases.py, each term within the bound derived
there; and gibbs_recount_kernel behind gibbs_set_state against the counts it was given."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import gibbs_restatement as spec
import posterior_cases as cases
from conftest import load_golden
from special_bounds import pair_error

pytestmark = pytest.mark.gpu

_worst = {}        # kernel -> (error / bound, case), over the cases run so far


@pytest.fixture(scope="module")
def golden():
    return load_golden("posterior_mp.npz")


class _State(object):
    """A case's state on the device."""

    def __init__(self, c):
        from pylda_amd import _capi
        self.ctx = _capi.Context(c.K, c.V)
        try:
            csr, topics = c.corpus()
            self.corpus = self.ctx.corpus(*csr)
            self.ctx.gibbs_set_state(self.corpus, c.n_kv, c.n_k, topics)
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self.ctx, self.corpus

    def __exit__(self, *exc):
        self.corpus.close()
        self.ctx.close()


def _ratios(got, bounds, g, key):
    return cases.bound_ratio(pair_error(np.atleast_1d(got), g[key + "_hi"], g[key + "_lo"]), bounds)


def _host_scalars(c):
    """The host's two scalar terms exactly as launch_gibbs.hip forms them: the sums in order, libm's lgamma."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.lgamma.restype, libm.lgamma.argtypes = ctypes.c_double, [ctypes.c_double]
    out = []
    for prior, times in ((c.alpha, c.D), (c.beta, c.K)):
        total, lg = 0.0, 0.0
        for x in prior:
            total += float(x)
            lg += libm.lgamma(float(x))
        out.append((libm.lgamma(total) - lg) * float(times))
    return out


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_term_is_within_its_bound_of_mpmath(name, golden):
    """After gibbs_set_state: n_dk is the case's, exactly (the recount kernel); through the test hook every document
    term, every word term and the three device sums are within their bounds of the references; so are the two public
    entry points, which repeat their bits and use the sums the hook shows.

    D = 0 (sum_D0_V257): the C ABI admits a corpus without documents; its documents' half is an exact 0."""
    c = cases.case(name)
    assert np.array_equal(golden[name + "_sha256"], c.digest())
    e = cases.evaluate(c)
    with _State(c) as (ctx, corpus):
        assert np.array_equal(np.array(ctx.get_gamma(corpus)).reshape(c.D, c.K), c.n_dk.astype(np.float64)), "n_dk after gibbs_set_state"
        docs, words, sums = ctx.test_gibbs_posterior_terms(corpus, c.alpha, c.beta)
        whole = ctx.gibbs_log_posterior(corpus, c.alpha, c.beta)
        parts = ctx.gibbs_log_posterior_parts(corpus, c.alpha, c.beta)
        again = (ctx.gibbs_log_posterior(corpus, c.alpha, c.beta), ctx.gibbs_log_posterior_parts(corpus, c.alpha, c.beta),
                 ctx.test_gibbs_posterior_terms(corpus, c.alpha, c.beta))
        counts = ctx.gibbs_get_counts(corpus)
    found = {"documents": _ratios(docs, e.doc_bounds, golden, name + "_docs"),
             "words": _ratios(words, e.word_bounds, golden, name + "_words"),
             "sums": _ratios(sums, e.sum_bounds, golden, name + "_sums"),
             "totals": _ratios([whole, parts[0], parts[1]], e.total_bounds, golden, name + "_totals")}
    both = parts[0] + parts[1]
    found["parts' sum"] = cases.bound_ratio(pair_error(both, golden[name + "_totals_hi"][0], golden[name + "_totals_lo"][0]),
                                            e.total_bounds[1] + e.total_bounds[2] + cases.U * abs(both))
    report = []
    for key, r in found.items():
        worst = float(r.max()) if r.size else 0.0
        report.append("%s %.3g" % (key, worst))
        if worst >= _worst.get(key, (-1.0, ""))[0]:
            _worst[key] = (worst, name)
    print("%s: worst error / bound: %s" % (name, ", ".join(report)))
    for key, r in found.items():
        assert np.all(np.isfinite(r)) and np.all(r < 1.0), \
            "%s: %s off by %.3g bounds at index %d (%s)" % (name, key, np.nanmax(r), int(np.nanargmax(r)), ", ".join(report))
    # the same bits again; the state untouched
    assert again[0] == whole and again[1] == parts
    assert all(np.array_equal(a, b) for a, b in zip(again[2], (docs, words, sums)))
    assert np.array_equal(counts[0], c.n_kv) and np.array_equal(counts[1], c.n_k)
    # the hook's sums are what the public calls used
    scalar_alpha, scalar_beta = _host_scalars(c)
    assert whole == scalar_alpha + scalar_beta + sums[0]
    assert parts == (scalar_alpha + sums[1], scalar_beta + sums[2])


def test_worst_ratios_over_the_grid():
    """(prints what the cases above found; DESIGN.md section 11 quotes it)"""
    print("log posterior against mpmath, worst error / bound over the grid: "
          + ", ".join("%s %.3g (%s)" % (k, v[0], v[1]) for k, v in _worst.items()))
    assert all(v[0] < 1.0 for v in _worst.values())


def test_hook_returns_codes_and_leaves_the_state_alone():
    from pylda_amd import _capi
    c = cases.case("doc_K65_D5")
    csr, topics = c.corpus()
    ctx = _capi.Context(c.K, c.V)
    try:
        corpus = ctx.corpus(*csr)
        docs, words, sums = np.zeros(c.D), np.zeros(c.V), np.zeros(3)
        dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        call = lambda handle, a, b, d, w, s: ctx._lib.pylda_test_gibbs_posterior_terms(ctx._h, handle, dp(a), dp(b), dp(d), dp(w), dp(s))
        assert call(corpus._h, c.alpha, c.beta, docs, words, sums) == -4                          # PYLDA_ERR_STATE: no state yet
        assert b"gibbs_init" in ctx._lib.pylda_last_error(ctx._h)
        with pytest.raises(_capi.PyldaError) as err:
            ctx.test_gibbs_posterior_terms(corpus, c.alpha, c.beta)
        assert err.value.status == -4
        ctx.gibbs_set_state(corpus, c.n_kv, c.n_k, topics)
        want = ctx.test_gibbs_posterior_terms(corpus, c.alpha, c.beta)
        for args in ((None, c.beta, docs, words, sums), (c.alpha, None, docs, words, sums), (c.alpha, c.beta, None, words, sums),
                     (c.alpha, c.beta, docs, None, sums), (c.alpha, c.beta, docs, words, None)):
            assert call(corpus._h, *args) == -1                                                   # PYLDA_ERR_INVALID
        assert ctx._lib.pylda_test_gibbs_posterior_terms(None, corpus._h, dp(c.alpha), dp(c.beta), dp(docs), dp(words), dp(sums)) == -1
        other = ctx.corpus(*csr)
        other.close()
        assert other._h is None and call(None, c.alpha, c.beta, docs, words, sums) == -1          # a closed corpus
        with pytest.raises(_capi.PyldaError) as err:
            ctx.test_gibbs_posterior_terms(other, c.alpha, c.beta)
        assert err.value.status == -1
        assert not docs.any() and not words.any() and not sums.any()                              # nothing was written
        got = ctx.test_gibbs_posterior_terms(corpus, c.alpha, c.beta)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        n_kv, n_k, state = ctx.gibbs_get_counts(corpus)
        assert np.array_equal(n_kv, c.n_kv) and np.array_equal(n_k, c.n_k) and np.array_equal(state, topics)
        assert np.array_equal(np.array(ctx.get_gamma(corpus)).reshape(c.D, c.K), c.n_dk.astype(np.float64))
        corpus.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("name", cases.SLICE_CASES)
def test_hyper_parameter_step_on_the_device_equals_the_restatements(name, symmetric):
    """slice_sample_hyperparameters on the device's log posterior and on the restatement's, from the same numpy state, end
    on the same bits (K = 65 and K = 300; the seeds are the ones tests/test_gibbs_posterior_host.py shows to leave every
    decision more than 100 bounds from its threshold).  Every log posterior the step asks for is moreover within two
    bounds of the restatement's - each is within one of the truth: with the switches off no proposal is accepted, and
    this is then what the comparison rests on."""
    from pylda_amd.monte_carlo import slice_sample_hyperparameters
    c = cases.case(name)
    seed = cases.SLICE_SEEDS[(name, symmetric)]
    asked = []
    with _State(c) as (ctx, corpus):
        def device(alpha, beta):
            asked.append((alpha.copy(), beta.copy(), ctx.gibbs_log_posterior(corpus, alpha, beta)))
            return asked[-1][2]
        np.random.seed(seed)
        got = slice_sample_hyperparameters(device, c.alpha, c.beta, symmetric, symmetric)
    np.random.seed(seed)
    want = slice_sample_hyperparameters(lambda a, b: spec.log_posterior(c.n_dk, c.n_kv, a, b), c.alpha, c.beta, symmetric, symmetric)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], c.alpha) != symmetric
    worst = 0.0
    for alpha, beta, lp in asked[::7]:
        worst = max(worst, abs(lp - spec.log_posterior(c.n_dk, c.n_kv, alpha, beta)) / cases.evaluate(c, alpha, beta).total_bounds[0])
    print("%s, symmetric %s: %d log posteriors, every 7th against the restatement: at most %.3g bounds apart" % (name, symmetric, len(asked), worst))
    assert worst < 2.0

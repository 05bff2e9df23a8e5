"""Host-side checks of the log posterior's grid (tests/posterior_cases.py) and its mpmath references
(tests/golden/posterior_mp.npz): the bound admits a correct fp64 implementation, the stored numbers belong to the states
the builders build today, and the seeds of the GPU's hyper-parameter test leave every accept decision a wide margin.
No GPU."""
import numpy as np
import pytest

import gibbs_restatement as spec
import posterior_cases as cases
from conftest import load_golden
from special_bounds import pair_error


@pytest.fixture(scope="module")
def golden():
    return load_golden("posterior_mp.npz")


def _ratios(got, bounds, g, key):
    return cases.bound_ratio(pair_error(np.atleast_1d(got), g[key + "_hi"], g[key + "_lo"]), bounds)


def test_stored_hashes_are_the_builders(golden):
    for name in cases.NAMES:
        assert np.array_equal(golden[name + "_sha256"], cases.case(name).digest()), \
            "%s: posterior_mp.npz was made from other inputs - run tests/golden/make_posterior_mp.py" % name
    stored = sorted(k[:-len("_sha256")] for k in golden if k.endswith("_sha256"))
    assert stored == sorted(cases.NAMES)


def test_the_grid_holds_what_it_promises():
    from fractions import Fraction
    for name in cases.NAMES:
        c = cases.case(name)
        assert np.array_equal(c.n_k, c.n_kv.sum(axis=1)) and c.D * c.K <= 100000, name
        (ptr, ids, cts), topics = c.corpus()
        assert len(ptr) == c.D + 1 and int(cts.sum()) == int(c.n_dk.sum()) == topics.size, name
    for K in cases.DOC_K:
        c = cases.case("doc_K%d_D9" % K)
        tokens = c.n_dk.sum(axis=1)
        assert 0 in tokens and {63, 64, 65} <= set(tokens.tolist()), K
        assert any(np.count_nonzero(r) == 1 and r[K - 1] > 0 for r in c.n_dk)
        assert K <= 64 or any(np.count_nonzero(r) == 1 and r[64] > 0 for r in c.n_dk)
    for K in cases.WORD_K:
        c = cases.case("word_K%d" % K)
        assert not c.n_kv[:, 0].any() and c.n_kv[:, 2].all() and c.n_kv[K - 1, 1] > 0
        assert np.count_nonzero(c.n_kv[:, 1]) == (2 if K > 257 else 1)          # (K = 257: one cell is both)
        assert K <= 256 or c.n_kv[256, 1] > 0
    for K in cases.PRIOR_K:
        for side, below in (("below", True), ("above", False)):
            c = cases.case("prior_sum12_%s_K%d" % (side, K))
            for prior in (c.alpha, c.beta):
                exact = sum((Fraction(float(x)) for x in prior), Fraction(0))
                in_order = 0.0
                for x in prior:
                    in_order += float(x)
                assert (exact < 12) == below and (in_order < 12.0) == below and abs(in_order - 12.0) < 1e-10, (name, in_order)
            assert 0 in c.n_dk.sum(axis=1) and 0 in c.n_k
        c = cases.case("prior_near12_K%d" % K)
        for x in (c.n_dk + c.alpha[np.newaxis, :], c.n_kv + c.beta[np.newaxis, :]):
            assert np.any((x < 12.0) & (x > 12.0 - 1e-9)) and np.any((x > 12.0) & (x < 12.0 + 1e-9))
        c = cases.case("heavy_K%d" % K)
        assert c.n_dk.max() == 10 ** 6 and c.n_k.max() == cases.INT32_MAX
        assert {1, 2, 10 ** 3, 10 ** 6, cases.INT32_MAX} <= set(c.n_kv.ravel().tolist())
        for kind in cases.PRIOR_KINDS:
            c = cases.case("prior_a%s_b%s_K%d" % (kind, kind, K))
            lo, hi = {"tiny": (1e-6, 1e-6), "huge": (1e3, 1e3), "spread": (1e-6, 1e3)}[kind]
            assert c.alpha.min() >= lo and c.alpha.max() <= hi and c.beta.min() >= lo and c.beta.max() <= hi
            assert kind != "spread" or (c.alpha.min() < 1e-4 and c.alpha.max() > 10.0)


def test_fp64_evaluations_stay_within_the_bound(golden):
    """scipy's gammaln summed by numpy, term by term, and gibbs_restatement.log_posterior: a correct fp64 implementation
    passes the bound the device is held to, with room."""
    worst = {"docs": (0.0, ""), "words": (0.0, ""), "sums": (0.0, ""), "totals": (0.0, ""), "restatement": (0.0, "")}
    for name in cases.NAMES:
        c = cases.case(name)
        e = cases.evaluate(c)
        found = {"docs": _ratios(e.docs, e.doc_bounds, golden, name + "_docs"),
                 "words": _ratios(e.words, e.word_bounds, golden, name + "_words"),
                 "sums": _ratios(e.sums, e.sum_bounds, golden, name + "_sums"),
                 "totals": _ratios(e.totals, e.total_bounds, golden, name + "_totals")}
        whole = spec.log_posterior(c.n_dk, c.n_kv, c.alpha, c.beta)
        found["restatement"] = cases.bound_ratio(pair_error(whole, golden[name + "_totals_hi"][0], golden[name + "_totals_lo"][0]),
                                                 e.total_bounds[0])
        assert np.all(e.doc_bounds > 0) and np.all(e.word_bounds > 0)
        for bounds in (e.sum_bounds, e.total_bounds):           # (without documents their half is an exact 0)
            assert np.all(bounds[[0, 2]] > 0) and (bounds[1] > 0) == (c.D > 0)
        for key, r in found.items():
            if r.size and r.max() > worst[key][0]:
                worst[key] = (float(r.max()), name)
    print("worst error / bound of the fp64 evaluation: " + ", ".join("%s %.2e (%s)" % (k, v[0], v[1]) for k, v in worst.items()))
    for key, (ratio, name) in worst.items():
        assert ratio < 1.0, "%s of %s: %.3g bounds" % (key, name, ratio)


def test_an_ordinary_bound_is_tight():
    """the bound of a document's term at K = 700 with ordinary priors is near 1e-11, not near the 1e-10 of a total of 4e5
    (4e-5) the older test allows"""
    rng = np.random.default_rng(5)
    n_dk = np.zeros((1, 700), dtype=np.int64)
    n_dk[0, rng.choice(700, 40, replace=False)] = rng.integers(1, 9, 40)
    e = cases.Evaluation(n_dk, np.ones((700, 1), dtype=np.int64), np.ones(700, dtype=np.int64), rng.uniform(0.02, 0.5, 700), np.array([0.1]))
    assert 1e-12 < e.doc_bounds[0] < 1e-9


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("name", cases.SLICE_CASES)
def test_slice_sampler_seeds_leave_every_decision_a_margin(name, symmetric):
    """The GPU test asserts bit-equal alpha and beta after a hyper-parameter step on the device's log posterior and on the
    restatement's: every accept decision |log posterior(proposal) - threshold| must be far from a coin toss - more than
    100 bounds of the total at that proposal - under the seed it uses."""
    from pylda_amd.monte_carlo import slice_sample_hyperparameters
    c = cases.case(name)
    lp = lambda a, b: spec.log_posterior(c.n_dk, c.n_kv, a, b)
    seed = cases.SLICE_SEEDS[(name, symmetric)]
    np.random.seed(seed)
    alpha, beta, decisions = cases.slice_sample_with_margins(lp, c.alpha, c.beta, symmetric, symmetric)
    np.random.seed(seed)
    want = slice_sample_hyperparameters(lp, c.alpha, c.beta, symmetric, symmetric)
    assert np.array_equal(alpha, want[0]) and np.array_equal(beta, want[1])
    accepted = sum(1 for d in decisions if d[2] > 0)
    # with the switches off every coordinate of the first proposal jumps on its own and none is ever accepted - then the
    # reference's kept quirk repeats that proposal; with them on, both kinds of decision occur
    assert len(decisions) > accepted and (accepted >= 3) == symmetric
    assert np.array_equal(alpha, c.alpha) != symmetric and np.array_equal(beta, c.beta) != symmetric
    closest = min(abs(m) / cases.evaluate(c, a, b).total_bounds[0] for a, b, m in decisions)
    print("%s, symmetric %s, seed %d: %d decisions, %d accepted, the closest %.3g bounds from its threshold"
          % (name, symmetric, seed, len(decisions), accepted, closest))
    assert closest > 100.0

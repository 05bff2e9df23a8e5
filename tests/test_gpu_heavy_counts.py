"""Term counts up to 10^6 through every family of E-step kernels.  Counts are int32, so a real corpus can push gamma_k to
10^6 and beyond; no other test takes gamma past a few thousand.  Here the fused exp(psi(gamma) - c) forms run at such
arguments inside the kernels, together with the counts' conversion to double in every kernel family and in the
statistics gather, training and held-out, at the default threshold (every document runs to the cap of 50 inner
iterations) and at a threshold of 1000 (the stops range from 1 to 50) - against the C oracle.  Needs an MI355X.

Counts towards 2^31 are left out on purpose: there the per-document log-likelihood cancels values near 1e11 and the two
CPU restatements (oracle/c_oracle.py, oracle/vb_numpy.py) themselves differ by 4e-8.  The samplers expand
counts into tokens and are no part of this.
"""
import numpy as np
import pytest

from conftest import rel_err
from test_gpu_estep import GAMMA_RTOL, LL_ATOL, LL_RTOL

pytestmark = pytest.mark.gpu

V = 3000
LENGTHS = (1, 2, 17, 64, 130, 215, 330, 600)        # distinct terms per document
HEAVY = 10 ** 6
CASES = [(10, None), (128, None), (256, None), (256, 0.01), (700, None), (1500, None)]      # K, alpha (None: U(0.05, 1.5))
THRESHOLDS = (1e-6, 1000.0)     # the default (the C oracle runs every document to the cap of 50) and one with stops from 1 to 50
FAMILIES = {"slab": {"slab"}, "quad": {"quad"}, "fused streaming": {"qgroup", "qfuse", "qfusek"},
            "generic": {"generic64", "generic256", "generic512", "generic_global", "generic_huge"}}


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    _capi.load()
    assert _capi.device_count() >= 1, "no HIP device visible"
    return _capi


def heavy_corpus(K, alpha0, copies=1):
    """Documents of LENGTHS distinct terms; counts exp(U(0, ln 10^6)) truncated to integers, one per document exactly 10^6."""
    rng = np.random.default_rng(K)
    ptr, ids, cts = [0], [], []
    for n in LENGTHS * copies:
        ids.append(np.sort(rng.choice(V, size=n, replace=False)))
        c = np.exp(rng.uniform(0.0, np.log(float(HEAVY)), n)).astype(np.int64)
        c[rng.integers(n)] = HEAVY
        cts.append(c)
        ptr.append(ptr[-1] + n)
    eta = rng.gamma(100.0, 0.01, (K, V))
    alpha = rng.uniform(0.05, 1.5, K) if alpha0 is None else np.full(K, alpha0)
    return np.array(ptr, np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(cts).astype(np.int32), eta, alpha


@pytest.mark.parametrize("heldout", [False, True])
@pytest.mark.parametrize("K,alpha0", CASES)
def test_heavy_counts_against_c_oracle(capi, K, alpha0, heldout):
    from oracle import c_oracle
    ptr, ids, cts, eta, alpha = heavy_corpus(K, alpha0)
    assert cts.min() >= 1 and cts.max() == HEAVY and np.all(np.maximum.reduceat(cts, ptr[:-1]) == HEAVY)
    tokens_of_word = np.bincount(ids, weights=cts.astype(np.float64), minlength=V)
    total = float(cts.astype(np.int64).sum())

    ctx = capi.Context(K, V)
    corpus = ctx.corpus(ptr, ids, cts)
    kernels = sorted({c["kernel"] for c in corpus.plan() if c["documents"] > 0})
    ctx.set_profiling(True)
    handed = 0
    for tol in THRESHOLDS:
        ref = c_oracle.e_step(alpha, eta, ptr, ids, cts, 50, tol, heldout=heldout)
        ctx.work_counters()
        out = ctx.estep_host(corpus, alpha, eta, 50, tol, heldout)
        ctx.work_counters()
        handed += ctx.executed_work()[1]
        key = "doc_words_ll" if heldout else "doc_ll"
        where = "K = %d, alpha %s, %s, threshold %g" % (K, alpha0 or "uniform", "held-out" if heldout else "training", tol)
        print("%s: kernels %s, iterations %d..%d (oracle %d..%d), gamma up to %.3g, worst gamma %.2e, log-likelihood %.2e"
              % (where, kernels, out["iters"].min(), out["iters"].max(), ref["iters"].min(),
                 ref["iters"].max(), out["gamma"].max(), rel_err(out["gamma"], ref["gamma"]),
                 np.max(np.abs(out[key] - ref[key]) / np.abs(ref[key]))))
        assert np.array_equal(out["iters"], ref["iters"]), where
        assert rel_err(out["gamma"], ref["gamma"]) < GAMMA_RTOL, where
        assert np.all(np.abs(out[key] - ref[key]) <= LL_RTOL * np.abs(ref[key]) + LL_ATOL), where
        if not heldout:
            err = np.abs(out["sstats"] - ref["sstats"]).max(axis=0)
            print("    statistics: worst error / (1e-9 tokens of the word + 1e-8) %.3f, sum off by %.2e of %g tokens"
                  % (np.max(err / (1e-9 * tokens_of_word + 1e-8)), abs(out["sstats"].sum() - total) / total, total))
            assert np.all(err <= 1e-9 * tokens_of_word + 1e-8), where
            assert abs(out["sstats"].sum() - total) <= 1e-9 * total, where
    print("K = %d, alpha %s: %d documents handed to the live-topic kernel over the two runs" % (K, alpha0 or "uniform", handed))
    if alpha0 is not None:
        assert handed > 0, "the live-topic hand-over took no document"
    corpus.close()
    ctx.close()


def test_heavy_counts_reach_every_kernel_family(capi):
    """The plans of the cases above, taken together, hold a slab, a quad, a fused streaming and a generic kernel."""
    plans = {}
    for K, alpha0 in CASES:
        ptr, ids, cts, _, _ = heavy_corpus(K, alpha0)
        ctx = capi.Context(K, V)
        corpus = ctx.corpus(ptr, ids, cts)
        plans[(K, alpha0)] = sorted({c["kernel"] for c in corpus.plan() if c["documents"] > 0})
        corpus.close()
        ctx.close()
    print("plans: %s" % plans)
    seen = set().union(*plans.values())
    for family, kernels in FAMILIES.items():
        assert seen & kernels, "no %s kernel in any plan: %s" % (family, plans)

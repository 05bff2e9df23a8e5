"""The M-step's alpha statistics with digamma only where gamma_dk moved away from alpha_k (mstep_alpha_ss_moved_kernel,
option alpha_ss_moved = 1, the default) against the kernel that evaluates all D x K entries (option 0): bit for bit,
on injected rows of gamma through pylda_test_alpha_statistics - the very launch pylda_mstep makes.  Needs an MI355X.

Natural inputs cannot produce a document with no moved topic, or with exactly 64 or 65 of them, so the rows are built
on the host from a mixed alpha (0.01 .. 2); per row the number of entries that differ from alpha is one of

    0, 1, 63, 64, 65, K     spread over all 64-topic stripes
    63, 64                  all inside ONE stripe (where K has a whole one)

(clipped to K), the moved entries log-uniform over 1e-3 .. 1e4, and in every row with two or more of them one is
nextafter(alpha_k, inf) and one nextafter(alpha_k, 0): one ulp off counts as moved.  64 moved entries and the row sum
are 65 list entries - the first count that no longer fits one call.  K = 3 ... 2049: below a stripe, a whole one, one
topic into the second, three stripes with a tail, the benchmark's four, 33 stripes with 100 KiB of dynamic LDS.
D = 0 ... 8193: the two-documents-per-trip tail and both sides of the 1024-workgroup stride (test_gpu_mstep.py).

Both options are also held to tests/mstep_reference.py at its TOLERANCE, as tests/test_gpu_mstep.py holds the M-step."""
import numpy as np
import pytest

import live_exit_cases
import mstep_reference as ref

pytestmark = pytest.mark.gpu

KS = (3, 64, 65, 130, 256, 2049)
DS = (0, 1, 3, 4, 5, 4097, 8193)
SPREAD = (0, 1, 63, 64, 65, None)       # None: all K
ONE_STRIPE = (63, 64)
PATTERNS = len(SPREAD) + len(ONE_STRIPE)


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    _capi.load()
    assert _capi.device_count() >= 1, "no HIP device visible"
    return _capi


def mixed_alpha(K):
    return np.random.default_rng(4200 + K).uniform(0.01, 2.0, K)


def injected_gamma(K, D):
    """(gamma, moved per row): row r takes pattern (r + D) mod 8, so that the few rows of a small D differ between the D."""
    rng = np.random.default_rng(77 * K + D)
    alpha = mixed_alpha(K)
    gamma = np.tile(alpha, (D, 1))
    want = np.zeros(D, dtype=np.int64)
    for r in range(D):
        p = (r + D) % PATTERNS
        if p < len(SPREAD):
            n = K if SPREAD[p] is None else min(SPREAD[p], K)
            at = rng.choice(K, size=n, replace=False)
        else:
            n = min(ONE_STRIPE[p - len(SPREAD)], K)
            stripe = int(rng.integers(0, max(1, K // 64)))                  # a whole stripe where there is one
            at = 64 * stripe + rng.choice(min(64, K), size=n, replace=False)
        gamma[r, at] = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n))
        if n >= 2:
            gamma[r, at[0]] = np.nextafter(alpha[at[0]], np.inf)
            gamma[r, at[1]] = np.nextafter(alpha[at[1]], 0.0)
        elif n == 1 and r % 2:
            gamma[r, at[0]] = np.nextafter(alpha[at[0]], np.inf if r % 4 == 1 else 0.0)
        want[r] = n
    assert np.array_equal((gamma.view(np.uint64) != alpha.view(np.uint64)[None, :]).sum(axis=1), want)
    return alpha, gamma, want


def test_the_rows_hold_every_pattern():
    """The inputs, from the host alone: every count of moved entries occurs at every K once D reaches the patterns, and a
    row with all of them in one stripe exists wherever K has more than one stripe."""
    for K in KS:
        _, gamma, want = injected_gamma(K, 4097)
        assert set(want) == {min(n, K) for n in (0, 1, 63, 64, 65, K)}
        if K >= 128:
            alpha = mixed_alpha(K)
            moved = gamma != alpha[None, :]
            in_one = [r for r in range(64) if moved[r].sum() in ONE_STRIPE and len(set(np.nonzero(moved[r])[0] // 64)) == 1]
            assert in_one, K


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("K", KS)
def test_moved_equals_all_on_injected_rows(capi, K, D):
    alpha, gamma, _ = injected_gamma(K, D)
    ctx = capi.Context(K, 8)
    ctx.set_alpha(alpha)
    got = {}
    for option in (1, 0, 1):
        ctx.set_option("alpha_ss_moved", option)
        stats = ctx.test_alpha_statistics(gamma)
        assert option not in got or np.array_equal(got[option], stats)          # repeats itself
        got[option] = stats
    ctx.close()
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    assert np.array_equal(got[1], got[0]), (K, D, float(np.max(np.abs(got[1] - got[0]))))
    if D == 0:
        assert np.array_equal(got[1], np.zeros(K))
        return
    reduced = ref.alpha_statistics(gamma)
    assert reduced.terms_stand_out(ref.TOLERANCE), "a term of these inputs is too small for the comparison to see it"
    for option in (0, 1):
        err = reduced.error_of(got[option])
        print("alpha statistics K=%d D=%d option %d: |device - reference| / scale = %.2e" % (K, D, option, err))
        assert err <= ref.TOLERANCE, (K, D, option, err)


def test_moved_equals_all_after_a_live_topic_estep(capi):
    """The natural case: the peaked K = 256 model of tests/live_exit_cases.py (two topics per document, 96 documents; the
    C oracle leaves 96 % of its gamma at alpha bitwise), E-step, then the M-step under both options."""
    ptr, ids, cts, eta, alpha = live_exit_cases.inputs("K256")
    K, V = live_exit_cases.MODELS["K256"], live_exit_cases.V
    beta = np.random.default_rng(5).uniform(0.3, 0.65, V)
    ctx = capi.Context(K, V)
    ctx.set_alpha(alpha)
    ctx.set_eta(eta)
    corpus = ctx.corpus(ptr, ids, cts)
    ctx.estep(corpus)
    gamma = np.array(ctx.get_gamma(corpus))
    stats = {}
    for option in (1, 0):
        ctx.set_option("alpha_ss_moved", option)
        stats[option] = ctx.mstep(corpus, beta)[1]
    through_the_hook = ctx.test_alpha_statistics(gamma)
    corpus.close()
    ctx.close()
    at_alpha = float(np.mean(gamma.view(np.uint64) == alpha.view(np.uint64)[None, :]))
    print("gamma == alpha bitwise: %.1f %% of %d x %d" % (100 * at_alpha, gamma.shape[0], K))
    assert at_alpha >= 0.8                      # the test reaches the table
    assert np.array_equal(stats[1], stats[0])
    assert np.array_equal(through_the_hook, stats[0])
    reduced = ref.alpha_statistics(gamma)
    assert reduced.error_of(stats[1]) <= ref.TOLERANCE

"""The E-step's table preparation (pylda_amd/csrc/prepare_kernels.h: eta_rowsum_psi_kernel, elog_rows_small_kernel,
elog_transpose_kernel + row_shift_exp_kernel, topic_lse_kernel) and alpha_mortality_kernel, read back through
pylda_test_tables, against tests/golden/tables_mp.npz: mpmath references of the unshifted tables as (hi, lo) pairs, at the
shapes where the kernels branch - every table stride from 16 to 1088, K = 1, a full wavefront, partial 32 x 32 tiles in
both directions, one word, V % 4 == 1 and a second strided trip of the row sums - and on etas that hold what flat test
etas do not: entries from 1e-5 to 1e6, row sums from below 1 to 1e9, identical topics, a tie of two topics to within an
ulp, and words whose exp(e) goes through the subnormals to an exact 0.  The bounds and the exact (bit for bit) properties
are those of tests/tables_reference.py, which tests/test_tables_golden.py shows a plain fp64 restatement to fit and six
injected defects to miss.  Needs an MI355X.

The two paths of enqueue_prepare (option prepare_path) must agree bit for bit in all six outputs: checked on every
K <= 64 case and on a 64 x 32769 eta (8193 workgroups, V % 4 == 1, V % 32 == 1), just past the K V = 2^21 boundary.

Measured on an MI355X (worst error / bound over the eleven cases; every test prints its own per table and case):
  psi_rowsum 0.151 (K = 1025 V = 5), shift 0.047 (K = 1025 V = 5), elog 0.124 (K = 1025 V = 5), expElog 0.250
  (K = 65 V = 37, topic 19 of word 25), expElog_elog 0.139 (K = 1025 V = 5), topic_lse 0.093 (K = 1025 V = 5); the plain
  fp64 restatement of test_tables_golden.py reaches 0.25 on the same cases.  The two paths: the same bits everywhere.
  With row_shift_exp_kernel's maximum taken over k < K - 1 (tried, not kept) 11 of these tests fail while all 113 of
  test_gpu_estep.py pass: the shift cancels in everything an E-step returns.
"""
import numpy as np
import pytest

import tables_reference as tr
from conftest import load_golden

pytestmark = pytest.mark.gpu

OUTPUTS = tr.TABLES


@pytest.fixture(scope="module")
def golden():
    return load_golden("tables_mp.npz")


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    _capi.load()
    assert _capi.device_count() >= 1, "no HIP device visible"
    return _capi


def assert_same_bits(a, b, what):
    for name in OUTPUTS:
        differ = np.nonzero(tr.bits(a[name]).ravel() != tr.bits(b[name]).ravel())[0]
        assert differ.size == 0, "%s: %s differs in %d values, first at flat index %d: %r against %r" % (
            what, name, differ.size, differ[0], a[name].ravel()[differ[0]], b[name].ravel()[differ[0]])


@pytest.mark.parametrize("K,V,path", tr.CASES)
def test_tables_against_the_golden(capi, golden, K, V, path):
    ref = tr.Reference(golden, K, V)
    ctx = capi.Context(K, V)
    try:
        ctx.set_eta(ref.eta)
        out = ctx.test_tables()
        assert out["path"] == path and out["elog"].shape == (V, ref.ldk)
        faults, worst = tr.compare(out, ref)
        tr.report("K = %d V = %d path %d" % (K, V, path), worst)
        assert not faults, faults
        assert_same_bits(out, ctx.test_tables(), "K = %d V = %d, a second run" % (K, V))
        # the forced paths: the same bits as each other and as the automatic choice
        forced = {}
        for choice in ((1, 2) if K <= 64 else (2,)):
            ctx.set_option("prepare_path", choice)
            forced[choice] = ctx.test_tables()
            assert forced[choice]["path"] == choice
            other_faults, other_worst = tr.compare(forced[choice], ref)
            if choice != path:
                tr.report("K = %d V = %d path %d (forced)" % (K, V, choice), other_worst)
            assert not other_faults, (choice, other_faults)
            assert_same_bits(out, forced[choice], "K = %d V = %d, prepare_path = %d against 0" % (K, V, choice))
        ctx.set_option("prepare_path", 0)
        assert ctx.test_tables(tables=False)["path"] == path
        if K >= 6:          # topics 0 and 1 are one row of eta twice
            for name in ("elog", "expElog", "expElog_elog"):
                assert tr.same_bits(out[name][:, 0], out[name][:, 1]), name
            assert tr.bits(out["psi_rowsum"])[0] == tr.bits(out["psi_rowsum"])[1]
            assert tr.bits(out["topic_lse"])[0] == tr.bits(out["topic_lse"])[1]
        if K == 1 or V == 1:          # e == +0.0 and b == 1 bit for bit; at V == 1 the row sum is the entry: u is 0
            assert not np.any(tr.bits(out["elog"])) and np.all(out["expElog"][:, :K] == 1.0)
            assert not np.any(tr.bits(out["expElog_elog"]))
        if V == 1:
            assert not np.any(tr.bits(out["shift"])) and not np.any(tr.bits(out["topic_lse"]))
    finally:
        ctx.close()


def drawn_eta(K, V, seed):
    """The suite's usual draw times a log-uniform factor over 1e-4 .. 1e4."""
    rng = np.random.default_rng(seed)
    return rng.gamma(100.0, 0.01, (K, V)) * np.exp(rng.uniform(np.log(1e-4), np.log(1e4), (K, V)))


@pytest.mark.parametrize("K,V,path", [(64, 32768, 1), (64, 32769, 2), (16, 131072, 1), (16, 131073, 2), (65, 8, 2)])
def test_path_boundary(capi, K, V, path):
    """K <= 64 and K V <= 2^21 is the one-kernel path; at 64 x 32769 the forced paths agree on the whole tables."""
    ctx = capi.Context(K, V)
    try:
        ctx.set_eta(drawn_eta(K, V, K + V))
        assert ctx.test_tables(tables=False)["path"] == path
        if (K, V) != (64, 32769):
            return
        out = {}
        for choice in (1, 2):
            ctx.set_option("prepare_path", choice)
            out[choice] = ctx.test_tables()
            assert out[choice]["path"] == choice
            faults = tr.structure_faults(out[choice], K, V)
            assert not faults, (choice, faults)
        assert_same_bits(out[1], out[2], "K = 64 V = 32769, prepare_path = 1 against 2")
    finally:
        ctx.close()


@pytest.mark.parametrize("case", range(tr.ALPHA_CASES))
def test_alpha_sgn(capi, golden, case):
    """alpha_sgn is alpha bit for bit but for the sign, which is set exactly where exp(psi(alpha_k) - psi(sum alpha + 8))
    is NOT below 1e-33 - the topics that may never count as dead.  Every alpha of the golden is at least 1e-9 (relative in
    t / kMortalT) from the threshold; the fused form's own bound there is about 1.6e-13."""
    alpha, mortal = golden["alpha%d" % case], golden["alpha%d_mortal" % case]
    K = alpha.size
    ctx = capi.Context(K, 3)
    try:
        ctx.set_eta(np.ones((K, 3)))
        ctx.set_alpha(alpha)
        got = ctx.test_tables(alpha_sgn=True, tables=False)["alpha_sgn"]
        assert tr.same_bits(np.abs(got), alpha)
        wrong = np.nonzero(np.signbit(got) == mortal)[0]
        print("K = %d: %d of %d topics may count as dead, closest t / kMortalT - 1 = %.2e" % (
            K, mortal.sum(), K, np.abs(golden["alpha%d_margin" % case]).min()))
        assert wrong.size == 0, "topics %s (alpha %s): sign bit %s, the golden says mortal = %s" % (
            wrong[:5], alpha[wrong[:5]], np.signbit(got[wrong[:5]]), mortal[wrong[:5]])
        assert tr.same_bits(got, ctx.test_tables(alpha_sgn=True, tables=False)["alpha_sgn"])
    finally:
        ctx.close()


def test_refusals(capi):
    ctx = capi.Context(65, 4)
    small = capi.Context(64, 4)
    try:
        for context, value in ((ctx, 1), (ctx, 3), (ctx, -1), (small, 3)):
            with pytest.raises(capi.PyldaError) as e:
                context.set_option("prepare_path", value)
            assert e.value.status == -1 and "prepare_path" in str(e.value)
        for value in (0, 2):
            ctx.set_option("prepare_path", value)
        for value in (2, 1, 0):
            small.set_option("prepare_path", value)
        with pytest.raises(capi.PyldaError) as e:
            ctx.test_tables()
        assert e.value.status == -4 and "set_eta" in str(e.value)
        ctx.set_eta(np.ones((65, 4)))
        with pytest.raises(capi.PyldaError) as e:
            ctx.test_tables(alpha_sgn=True)
        assert e.value.status == -4 and "set_alpha" in str(e.value)
        # every pointer NULL: the kernels run, nothing is copied
        assert ctx._lib.pylda_test_tables(ctx._h, None, None, None, None, None, None, None, None) == 0
        assert ctx.test_tables()["path"] == 2
    finally:
        ctx.close()
        small.close()

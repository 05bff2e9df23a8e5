"""Every call form of the device special functions (pylda_amd/csrc/special_device.h, reached through
pylda_test_special_forms) against tests/golden/special_mp.npz: mpmath references stored as (hi, lo) pairs of doubles, at
the points where the functions branch - the thresholds 10 and 12, every trip count of the trigamma loop, the root of psi,
the zeros of ln Gamma, arguments from 2.3e-308 to 1e15 (1e30 for the fused forms) and the zone where exp(psi(x) - c)
passes through the subnormals to 0.  Needs an MI355X.

Each set of points is fed shuffled (the lanes of a wavefront then take different branches and loop counts) and once more
sorted: a value must not depend on its neighbours in the wavefront, so the two runs agree bit for bit.

Measured on an MI355X (maxima over the golden's points; every test prints its own):
  digamma 1.3e-15 scaled (x = 1.751), lgamma_pos 8.8e-15 scaled (x = 1.501), trigamma 5.1e-16 relative (scipy's polygamma
  6.2e-16 on the same points), exp_shallow 1.80 ulp, rcp_newton 0.4995 ulp, exp_digamma_minus 0.24 of its bound, the
  level-ordered forms 0.27 of it; on the dense grid both reach 0 exactly where the reference does (549 / 758 zeros).
"""
import numpy as np
import pytest
import scipy.special

from conftest import load_golden
from special_bounds import (DIGAMMA_SCALED, EXP_SHALLOW_ULP, LGAMMA_SCALED, MIN_NORMAL, RCP_NEWTON_ULP, SUBNORMAL_SPACING,
                            TRIGAMMA_OVER_SCIPY, fused_bound, pair_error, relative_error, scaled_error, ulp_error)

pytestmark = pytest.mark.gpu

DIGAMMA, LGAMMA, TRIGAMMA, EXP_SHALLOW, RCP_NEWTON, FUSED_LITERALS, FUSED_LEVELS, FUSED_LEVELS_A, FUSED_LEVELS_AB = range(9)
FUSED = (FUSED_LITERALS, FUSED_LEVELS, FUSED_LEVELS_A, FUSED_LEVELS_AB)
NAMES = ["digamma", "lgamma_pos", "trigamma", "exp_shallow", "rcp_newton", "exp_digamma_minus", "exp_digamma_minus_levels(x, c)",
         "exp_digamma_minus_levels(x, c, A)", "exp_digamma_minus_levels<true>(x, c, A, &B)"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("special_mp.npz")


@pytest.fixture(scope="module")
def ctx():
    from pylda_amd import _capi
    _capi.load()
    assert _capi.device_count() >= 1, "no HIP device visible"
    context = _capi.Context(2, 2)
    yield context
    context.close()


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def evaluate(ctx, form, x, c=0.0):
    """The form at every x, in x's order: fed shuffled, and sorted once more - bit-identical per point."""
    shuffled = np.random.default_rng(form + 1).permutation(x.size)
    ordered = np.argsort(x, kind="stable")
    got = np.empty_like(x)
    got[shuffled] = ctx.test_special_forms(x[shuffled], form, c)
    again = np.empty_like(x)
    again[ordered] = ctx.test_special_forms(x[ordered], form, c)
    differ = np.nonzero(got.view(np.int64) != again.view(np.int64))[0]
    assert differ.size == 0, "%s: %d values depend on the order of the points, first at x = %r: %r shuffled, %r sorted" % (
        NAMES[form], differ.size, x[differ[0]], got[differ[0]], again[differ[0]])
    return got


def report(form, what, err, x):
    i = int(np.argmax(err))
    print("%s: worst %s %.3e at x = %r" % (NAMES[form], what, err[i], x[i]))


def test_digamma(ctx, golden):
    g = golden
    got = evaluate(ctx, DIGAMMA, g["sp_x"])
    assert np.all(np.isfinite(got))
    err = scaled_error(got, g["psi_hi"], g["psi_lo"])
    report(DIGAMMA, "error / max(1, |psi|)", err, g["sp_x"])
    assert err.max() < DIGAMMA_SCALED


def test_lgamma_pos(ctx, golden):
    g = golden
    got = evaluate(ctx, LGAMMA, g["sp_x"])
    assert np.all(np.isfinite(got))
    err = scaled_error(got, g["lgam_hi"], g["lgam_lo"])
    report(LGAMMA, "error / max(1, |ln Gamma|)", err, g["sp_x"])
    assert err.max() < LGAMMA_SCALED


def test_trigamma(ctx, golden):
    """The alpha update's Newton step divides by it: as accurate as scipy.special.polygamma(1, x), which the reference
    calls - within 8 times scipy's own worst relative error against the same golden on the same points."""
    g = golden
    got = evaluate(ctx, TRIGAMMA, g["tg_x"])
    assert np.all(np.isfinite(got))
    err = relative_error(got, g["tg_hi"], g["tg_lo"])
    scipy_err = relative_error(scipy.special.polygamma(1, g["tg_x"]), g["tg_hi"], g["tg_lo"])
    report(TRIGAMMA, "relative error", err, g["tg_x"])
    print("scipy.special.polygamma(1, x): worst relative error %.3e at x = %r" % (scipy_err.max(), g["tg_x"][scipy_err.argmax()]))
    assert err.max() < TRIGAMMA_OVER_SCIPY * scipy_err.max()


def test_exp_shallow(ctx, golden):
    """Uniform arguments over [-745, 700] and the rounding boundaries (k + 1/2) ln 2 of its argument reduction."""
    g = golden
    got = evaluate(ctx, EXP_SHALLOW, g["ex_x"])
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
    normal = g["ex_hi"] >= MIN_NORMAL
    err = ulp_error(got[normal], g["ex_hi"][normal], g["ex_lo"][normal])
    report(EXP_SHALLOW, "error in ulp", err, g["ex_x"][normal])
    assert err.max() < EXP_SHALLOW_ULP
    # below the normal numbers the result is rounded twice (the polynomial, then the scaling): half a spacing more
    tiny = np.abs(pair_error(got[~normal], g["ex_hi"][~normal], g["ex_lo"][~normal])) / SUBNORMAL_SPACING
    print("exp_shallow below 2^-1022: worst error %.2f subnormal spacings or %.2e relative" % (
        tiny.max(), np.max(np.abs(got[~normal] - g["ex_hi"][~normal]) / g["ex_hi"][~normal])))


def test_rcp_newton(ctx, golden):
    g = golden
    got = evaluate(ctx, RCP_NEWTON, g["rc_x"])
    assert np.all(np.isfinite(got))
    err = ulp_error(got, g["rc_hi"], g["rc_lo"])
    report(RCP_NEWTON, "error in ulp", err, g["rc_x"])
    assert err.max() < RCP_NEWTON_ULP


def fused_forms(ctx, x, c):
    """The four fused forms at every x; the three level-ordered ones are one instruction sequence with its tables
    fetched at different times and agree bit for bit."""
    got = {form: evaluate(ctx, form, x, c) for form in FUSED}
    for form in (FUSED_LEVELS_A, FUSED_LEVELS_AB):
        differ = np.nonzero(got[form].view(np.int64) != got[FUSED_LEVELS].view(np.int64))[0]
        assert differ.size == 0, "c = %g: %s differs from %s on %d points, first at x = %r: %r against %r" % (
            c, NAMES[form], NAMES[FUSED_LEVELS], differ.size, x[differ[0]], got[form][differ[0]], got[FUSED_LEVELS][differ[0]])
    return got


@pytest.mark.parametrize("row", range(5))
def test_fused_exp_digamma_forms(ctx, golden, row):
    """exp(psi(x) - c) for x from 1e-4 to 1e30 and c in {0, 3.5, -1.25, 9, 23}."""
    g = golden
    x, c, hi, lo = g["fx_x"], float(g["fx_c"][row]), g["fx_hi"][row], g["fx_lo"][row]
    normal = hi >= MIN_NORMAL          # (x near 1e-4 gives exp(-1e4): there, as on the dense grid below, 4 subnormal spacings)
    assert normal.sum() > 0.8 * x.size
    for form, got in fused_forms(ctx, x, c).items():
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
        err = relative_error(got[normal], hi[normal], lo[normal]) / fused_bound(g["fx_psi"][normal], c)
        report(form, "relative error / (2e-15 (4 + |psi - c|)) at c = %g" % c, err, x[normal])
        assert err.max() < 1.0, (NAMES[form], c)
        assert np.all(np.abs(pair_error(got[~normal], hi[~normal], lo[~normal])) <= 4.0 * SUBNORMAL_SPACING), (NAMES[form], c)


@pytest.mark.parametrize("row", range(2))
def test_fused_forms_through_the_subnormals(ctx, golden, row):
    """2 000 sorted x in [1.30e-3, 1.45e-3]: exp(psi(x) - c) falls from 1e-300 through the subnormals to an exact 0 -
    where a topic dies, which the live-topic hand-over counts on.  Finite, not negative, never decreasing in x, within
    the relative bound or 4 subnormal spacings of the reference."""
    g = golden
    x, c, hi, lo = g["uf_x"], float(g["uf_c"][row]), g["uf_hi"][row], g["uf_lo"][row]
    allowed = np.maximum(fused_bound(g["uf_psi"], c) * hi, 4.0 * SUBNORMAL_SPACING)
    subnormal = hi < MIN_NORMAL
    for form, got in fused_forms(ctx, x, c).items():
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
        err = np.abs(pair_error(got, hi, lo))
        print("%s at c = %g: %d exact zeros (reference %d), worst error below 2^-1022 %.2f subnormal spacings, worst error / "
              "allowed %.3f" % (NAMES[form], c, int((got == 0.0).sum()), int((hi == 0.0).sum()),
                                (err[subnormal] / SUBNORMAL_SPACING).max(), (err / allowed).max()))
        falls = np.nonzero(np.diff(got) < 0.0)[0]
        assert falls.size == 0, "%s at c = %g decreases from x = %r to %r" % (NAMES[form], c, x[falls[0]], x[falls[0] + 1])
        worst = int(np.argmax(err / allowed))
        assert err[worst] <= allowed[worst], "%s at c = %g, x = %r: %r, reference %r" % (NAMES[form], c, x[worst], got[worst], hi[worst])


def test_fused_forms_give_zero_for_tiny_arguments(ctx, golden):
    """x from 1e-300 to 1e-5 (an alpha_k that small: pylda_set_alpha accepts any positive value): exp(-1 / x - ...) is a clean
    0 in every form, never inf or NaN."""
    x = golden["tiny_x"]
    for c in (0.0, 4.0, 23.0):
        for form, got in fused_forms(ctx, x, c).items():
            assert same_bits(got, np.zeros_like(x)), (NAMES[form], c, got)


def test_unknown_form_is_refused(ctx):
    from pylda_amd import _capi
    for form in (-1, 9, 100):
        with pytest.raises(_capi.PyldaError) as e:
            ctx.test_special_forms(np.ones(3), form)
        assert e.value.status == -1 and "form" in str(e.value)
    assert ctx.test_special_forms(np.zeros(0), 0).size == 0

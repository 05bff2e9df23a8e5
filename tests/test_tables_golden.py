"""tests/golden/tables_mp.npz is what tests/test_gpu_tables.py measures the E-step's table preparation against.  Here, on
the CPU: the file itself is checked (against mpmath, where that is installed), a plain fp64 restatement of the tables
(the C oracle's digamma and numpy) is shown to fit inside the bounds of tests/tables_reference.py on every case - a correct
fp64 implementation passes - and the same restatement with one defect at a time is shown to be rejected by the same
comparison - a wrong one does not."""
import numpy as np
import pytest
import scipy.special

import tables_reference as tr
from conftest import load_golden
from oracle import c_oracle
from special_bounds import MIN_NORMAL

MORTAL_T, MORTAL_TOKENS = 1e-33, 8.0          # estep_common.h kMortalT, kMortalTokens
SHAPES = [(K, V) for K, V, _ in tr.CASES]


@pytest.fixture(scope="module")
def golden():
    return load_golden("tables_mp.npz")


@pytest.fixture(scope="module")
def references(golden):
    return {(K, V): tr.Reference(golden, K, V) for K, V in SHAPES}


_PSI_ETA = {}


def restatement(eta, defect=None):
    """The tables in plain fp64, laid out as Context.test_tables returns them; `defect` breaks one thing."""
    K, V = eta.shape
    ldk = tr.table_stride(K)
    with np.errstate(all="ignore"):
        S = (eta[:, :-1] if defect == "row sum without its last element" else eta).sum(axis=1)
        psi_rowsum = c_oracle.digamma(S)
        if (K, V) not in _PSI_ETA:
            _PSI_ETA[(K, V)] = c_oracle.digamma(eta)
        u = _PSI_ETA[(K, V)] - psi_rowsum[:, None]
        if defect == "one u off by 1e-12 relative":         # (an entry of everyday size: the one nearest -20)
            at = np.unravel_index(np.argmin(np.abs(u + 20.0)), u.shape)
            u[at] *= 1.0 + 1e-12
        over = u[:min(K, 64) - 1] if defect == "shift over the first min(K, 64) - 1 topics" else u
        shift = over.max(axis=0, initial=-np.inf)
        e = u - shift[None, :]
        b = np.exp(e)
        be = np.where(b > 0.0, b * e, 0.0)
        if defect == "expElog_elog -0.0 where expElog underflows":
            be = b * e
        if defect == "expElog_elog NaN where expElog underflows":
            be = np.where(b > 0.0, b * e, np.nan)
        # the held-out normaliser from the shifted table, as the tables are all an E-step keeps
        back = e + shift[None, :]
        top = back.max(axis=1)
        topic_lse = top + np.log(np.exp(back - top[:, None]).sum(axis=1))
    out = {"psi_rowsum": psi_rowsum, "shift": shift, "topic_lse": topic_lse}
    for name, table in (("elog", e), ("expElog", b), ("expElog_elog", be)):
        out[name] = np.zeros((V, ldk))
        out[name][:, :K] = table.T
    if defect == "words w and w + 1 swapped":
        for name in ("elog", "expElog", "expElog_elog", "shift"):
            out[name][:2] = out[name][:2][::-1].copy()
    if defect == "a padding column holds 1e-300":
        out["expElog"][V // 2, ldk - 1] = 1e-300
    return out


# defect -> the cases on which it changes nothing, and why
DEFECTS = {
    "row sum without its last element": [],
    "shift over the first min(K, 64) - 1 topics": [(300, 1)],        # u is identically 0 at V = 1: every topic is the maximum
    "one u off by 1e-12 relative": [(300, 1)],                       # ... and 0 (1 + 1e-12) is 0
    "words w and w + 1 swapped": [(300, 1)],                         # one word
    "a padding column holds 1e-300": [(16, 64), (128, 31)],          # ldk == K: no padding
    "expElog_elog -0.0 where expElog underflows": [(1, 5), (300, 1)],    # expElog is 1 everywhere
    "expElog_elog NaN where expElog underflows": [(1, 5), (300, 1)],
}


def test_pairs_are_normalised_and_the_cases_hold_what_they_are_for(golden, references):
    g = golden
    for K, V in SHAPES:
        name = "K%d_V%d" % (K, V)
        for key in ("u", "rowsum", "lse"):
            hi, lo = g["%s_%s_hi" % (name, key)], g["%s_%s_lo" % (name, key)]
            assert hi.shape == lo.shape == ((K, V) if key == "u" else (K,))
            assert np.all(np.isfinite(hi)) and np.all(np.isfinite(lo))
            assert np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi))), (name, key)
        r = references[(K, V)]
        assert np.all(r.eta > 0.0) and np.all(np.isfinite(r.eta)) and r.ldk == tr.table_stride(K)
        if V == 1:
            assert np.all(r.u == 0.0) and np.all(r.topic_lse == 0.0)
            continue
        assert np.all(r.u < 0.0)
        subnormal = (r.b >= tr.LD(2.0) ** -1075) & (r.b < tr.LD(MIN_NORMAL))
        if K >= 17:
            assert subnormal.sum() > 10 and r.must_be_zero.sum() > 10, (name, subnormal.sum(), r.must_be_zero.sum())
        if K >= 6:
            assert np.array_equal(r.eta[0], r.eta[1]) and tr.same_bits(g[name + "_u_hi"][0], g[name + "_u_hi"][1])
            assert 0.5e9 < r.eta[2].sum() < 2e9 and r.eta[3].sum() < 1.0 and r.psi_rowsum[3] < 0.0
            top2 = np.sort(r.u, axis=0)[-2:]                # a word whose two largest u are an ulp apart at most
            gap = (top2[1] - top2[0]).astype(np.float64)
            assert np.any((gap > 0.0) & (gap <= np.spacing(np.abs(top2[1]).astype(np.float64))))
            # the maximum of some word is in the last topic, and in topic 63 where there are more than 64
            assert K - 1 in r.u.argmax(axis=0) and (K <= 64 or 63 in r.u.argmax(axis=0))
    assert sum(K * V for K, V in SHAPES) == 21821


def test_pairs_and_derived_tables_against_mpmath(golden, references):
    """A spread of the stored pairs recomputed: hi + lo within 1e-30 relative of mpmath's value at 50 digits.  What
    tables_reference.py derives from them in long double - shift, e, exp(e), exp(e) e - on a sample of whole words, to what
    64 bits of mantissa give: 2^-60 of the magnitudes that went into each."""
    mpmath = pytest.importorskip("mpmath")
    from fractions import Fraction
    mpmath.mp.dps = 50
    mp = lambda v: mpmath.mpf(float(v))
    both = lambda hi, lo: mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))

    def long(v):            # a long double, exactly (its exponent range is wider than a double's)
        m, ex = np.frexp(v)
        return mpmath.mpf(int(np.ldexp(m, 64))) * mpmath.mpf(2) ** (int(ex) - 64)

    close = lambda got, want: abs(got - want) <= mpmath.mpf("1e-30") * abs(want)
    checked = derived = 0
    for K, V in SHAPES:
        name, r = "K%d_V%d" % (K, V), references[(K, V)]
        g = {key: golden["%s_%s" % (name, key)] for key in ("u_hi", "u_lo", "rowsum_hi", "rowsum_lo", "lse_hi", "lse_lo")}
        row_psi = {}

        def u_of(k, w):
            if k not in row_psi:
                s = sum((Fraction(float(v)) for v in r.eta[k]), Fraction(0))
                row_psi[k] = mpmath.digamma(mpmath.mpf(s.numerator) / mpmath.mpf(s.denominator))
            return mpmath.digamma(mp(r.eta[k, w])) - row_psi[k]

        for flat in range(K * V % 37, K * V, 37):
            k, w = divmod(flat, V)
            assert close(both(g["u_hi"][k, w], g["u_lo"][k, w]), u_of(k, w)), (name, k, w)
            checked += 1
        for k in range(0, K, 5):
            u_of(k, 0)
            assert close(both(g["rowsum_hi"][k], g["rowsum_lo"][k]), row_psi[k]), (name, k)
            want = mpmath.log(mpmath.fsum(mpmath.exp(u_of(k, w)) for w in range(V)))
            assert close(both(g["lse_hi"][k], g["lse_lo"][k]), want) or (V == 1 and want == 0), (name, k)
            checked += 2
        for w in range(0, V, 16):
            u = [u_of(k, w) for k in range(K)]
            shift = max(u)
            assert abs(long(r.shift[w]) - shift) <= mpmath.mpf(2) ** -60 * max(1, abs(shift))
            for k in range(K):
                e = u[k] - shift
                mag = 1 + abs(u[k]) + abs(shift)
                assert abs(long(r.e[k, w]) - e) <= mpmath.mpf(2) ** -60 * mag, (name, k, w)
                if e > -11000:          # (below that exp(e) leaves the long doubles' normal range: next to nothing there)
                    b = mpmath.exp(e)
                    assert abs(long(r.b[k, w]) - b) <= mpmath.mpf(2) ** -60 * mag * b, (name, k, w)
                    assert abs(long(r.be[k, w]) - b * e) <= mpmath.mpf(2) ** -59 * mag * b * max(1, abs(e)), (name, k, w)
                else:
                    assert 0 <= r.b[k, w] < tr.LD(2.0) ** -15000 and abs(r.be[k, w]) < tr.LD(2.0) ** -14000
                assert bool(r.must_be_zero[k, w]) == (mpmath.exp(e) < mpmath.mpf(2) ** -1075)
                derived += 1
    assert checked >= 500 and derived >= 2000, (checked, derived)


def test_alpha_cases_against_mpmath_and_plain_fp64(golden):
    """Every alpha at least 1e-9 (relative, in t / kMortalT) away from the threshold; the stored classification recomputed
    with mpmath on a sample, and by plain fp64 on all of it - which the margin makes safe."""
    g = golden
    sizes = []
    for i in range(tr.ALPHA_CASES):
        alpha, mortal, margin = g["alpha%d" % i], g["alpha%d_mortal" % i], g["alpha%d_margin" % i]
        sizes.append(alpha.size)
        assert mortal.dtype == np.bool_ and alpha.shape == mortal.shape == margin.shape
        assert np.all(alpha >= 0.003) and np.all(alpha <= 0.05) and np.all(np.abs(margin) >= 1e-9)
        assert np.array_equal(mortal, margin < 0.0)
        if alpha.size > 1:
            assert 0 < mortal.sum() < alpha.size and np.sum(np.abs(margin) < 1e-4) == 6      # the pairs at (1 +- 1e-6)
        t = np.exp(scipy.special.digamma(alpha) - scipy.special.digamma(alpha.sum() + MORTAL_TOKENS))
        assert np.array_equal(t < MORTAL_T, mortal), i
    assert sorted(set(sizes)) == [1, 255, 256, 257, 1025]
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    for i in range(tr.ALPHA_CASES):
        alpha = g["alpha%d" % i]
        psi_shortest = mpmath.digamma(mpmath.fsum(mpmath.mpf(float(a)) for a in alpha) + MORTAL_TOKENS)
        for k in sorted(set(range(0, alpha.size, 9)) | {1, alpha.size // 2, alpha.size - 1} & set(range(alpha.size))):
            ratio = mpmath.exp(mpmath.digamma(mpmath.mpf(float(alpha[k]))) - psi_shortest) / mpmath.mpf(MORTAL_T)
            assert (ratio < 1) == bool(g["alpha%d_mortal" % i][k])
            assert abs(float(ratio - 1) - g["alpha%d_margin" % i][k]) <= 1e-12 * abs(float(ratio - 1)) + 1e-20


@pytest.mark.parametrize("K,V", SHAPES)
def test_plain_fp64_restatement_is_within_the_bounds(references, K, V):
    """The proof that a correct fp64 implementation fits: the C oracle's digamma, numpy's sum, exp and log."""
    r = references[(K, V)]
    faults, worst = tr.compare(restatement(r.eta), r)
    tr.report("fp64 restatement K = %d V = %d" % (K, V), worst)
    assert not faults, faults


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_the_comparison_rejects_an_injected_defect(references, defect):
    """One defect at a time in the same restatement: rejected on every case it can show on."""
    for K, V in SHAPES:
        if (K, V) in DEFECTS[defect]:
            continue
        r = references[(K, V)]
        faults, _ = tr.compare(restatement(r.eta, defect), r)
        assert faults, "%s goes unnoticed at K = %d V = %d" % (defect, K, V)
        print("K = %d V = %d, %s: %s" % (K, V, defect, faults[0]))

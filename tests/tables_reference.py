"""The tables an E-step prepares from eta, derived from the mpmath pairs of tests/golden/tables_mp.npz in long double, and the
comparison tests/test_tables_golden.py (a plain fp64 restatement, on the CPU) and tests/test_gpu_tables.py (the kernels
of pylda_amd/csrc/prepare_kernels.h, through pylda_test_tables) both go through.  Shares no code with the kernels or
with oracle/.

The golden stores, per case, eta, the UNSHIFTED u[k][w] = psi(eta_kw) - psi(S_k) (S_k = sum_v eta_kv), psi(S_k) and
topic_lse[k] = log sum_v exp(u[k][v]) as (hi, lo) pairs; from hi + lo in np.longdouble (64 bits of mantissa, an exponent
range that holds exp(-1e5)):
    shift[w] = max_k u[k][w]      e = u - shift      b = exp(e)      b e

The bounds (absolute unless said otherwise; D = special_bounds.DIGAMMA_SCALED, the bound the device digamma is held to by
tests/test_gpu_special.py; n = ceil(V / 256) + 10 roundings of a tree sum of V terms: V / 256 serial additions per thread,
8 levels of the tree, two to spare):
  tol_u[k,w]   = D (max(1, |psi(eta_kw)|) + max(1, |psi(S_k)|)) + trigamma(S_k) S_k n 2^-53
                 two digammas; the second one's ARGUMENT is the device's sum of V positive terms, relative error n 2^-53,
                 which psi turns into trigamma(S) S n 2^-53.  (The rounding of the subtraction itself, 2^-53 |u|, is part
                 of tol_e below and small against D here.)
  tol_rowsum[k]= D max(1, |psi(S_k)|) + trigamma(S_k) S_k n 2^-53          (the second half of tol_u)
  tol_shift[w] = max tol_u[k,w] over the topics k that CAN be the word's maximum: those with u_k + tol_u_k >= max_j (u_j -
                 tol_u_j).  A maximum moves by no more than the arguments that can reach it do.  Never more than the
                 max_k tol_u[k,w] over all topics, and much less for nearly every word: a topic with eta = 1e-5 has
                 |psi| = 1e5 and tol_u = 5e-10, never is the maximum, and would otherwise hide an error of 1e-11 in
                 every entry of its word
  tol_e        = tol_u + tol_shift + 2^-53 (|u| + |e|)                     the two rounded subtractions
  expElog      relative tol_e + 2 * 2^-52: exp turns the absolute error of e into a relative one, one ulp for the
                 library exp, one for rounding.  Where the reference is below MIN_NORMAL the allowance is at least
                 4 SUBNORMAL_SPACING, as tests/test_gpu_special.py allows exp(psi(x) - c) in the same zone
                 (max(relative bound * reference, 4 spacings)): down there a result is a multiple of the spacing, and the
                 relative bound alone would ask for less than one.  The relative part stays: just below MIN_NORMAL tol_e
                 is worth thousands of spacings (2^-53 |e| alone, the rounding of e at |e| = 708, is 350).
  expElog_elog the product rule: |e| tol_b + b tol_e + tol_b tol_e, tol_b the absolute allowance of expElog
  topic_lse[k] = log sum_v p_v exp(t_v) + n 2^-52, p_v = exp(u_kv - topic_lse_k), t_v = tol_u[k,v] + 2^-53 (|u| + |e|)
                 logsumexp is monotone, so this is exactly how far arguments off by up to t_v move it: their weighted
                 mean to first order, never more than max_v t_v, for the reason given for tol_shift.  The kernel forms
                 its arguments as e + shift, which gives u back to the two roundings in t_v.  n 2^-52: the sum and the log
Structure, bit for bit, wherever it is exact: columns K .. ldk-1 of the three tables +0.0; expElog in [0, 1] and exactly 1
at a row's maximum; expElog_elog +0.0 where expElog is 0 and never NaN; expElog an exact 0 where the reference is below
2^-1075; shift the maximum of the table's own unshifted values (elog <= 0 with an exact 0 in every row); everything finite.
"""
import math

import numpy as np
import scipy.special

from special_bounds import DIGAMMA_SCALED, MIN_NORMAL, SUBNORMAL_SPACING

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not the 80-bit extended type: no headroom over fp64 here"

LD = np.longdouble
# (K, V) -> the path pylda_test_tables reports with prepare_path = 0
CASES = [(1, 5, 1), (10, 257, 1), (16, 64, 1), (17, 33, 1), (33, 30, 1), (64, 40, 1),
         (65, 37, 2), (128, 31, 2), (257, 9, 2), (300, 1, 2), (1025, 5, 2)]
ALPHA_CASES = 10
TABLES = ("psi_rowsum", "shift", "elog", "expElog", "expElog_elog", "topic_lse")
EPS = 2.0 ** -53


def table_stride(K):
    """The row stride of the word-major tables (pylda_table_stride): 16 .. 256 in powers of two, multiples of 128 up to
    1024, multiples of 64 above."""
    for ldk in (16, 32, 64, 128, 256):
        if K <= ldk:
            return ldk
    return (K + 127) // 128 * 128 if K <= 1024 else (K + 63) // 64 * 64


class Reference(object):
    """One case of the golden: eta, the long-double tables (K x V, topic-major as eta) and their bounds."""

    def __init__(self, golden, K, V):
        name = "K%d_V%d" % (K, V)
        self.K, self.V, self.ldk = K, V, table_stride(K)
        self.eta = golden[name + "_eta"]
        assert self.eta.shape == (K, V)
        pair = lambda key: golden["%s_%s_hi" % (name, key)].astype(LD) + golden["%s_%s_lo" % (name, key)].astype(LD)
        self.u, self.psi_rowsum, self.topic_lse = pair("u"), pair("rowsum"), pair("lse")
        self.shift = self.u.max(axis=0)
        self.e = self.u - self.shift[None, :]
        self.b = np.exp(self.e)
        self.be = self.b * self.e
        # bounds, in doubles
        n = math.ceil(V / 256.0) + 10
        S = self.eta.astype(LD).sum(axis=1).astype(np.float64)
        sum_term = scipy.special.polygamma(1, S) * S * n * EPS
        psi_S = np.abs(self.psi_rowsum.astype(np.float64))
        psi_eta = np.abs((self.u + self.psi_rowsum[:, None]).astype(np.float64))
        self.tol_rowsum = DIGAMMA_SCALED * np.maximum(1.0, psi_S) + sum_term
        self.tol_u = DIGAMMA_SCALED * (np.maximum(1.0, psi_eta) + np.maximum(1.0, psi_S)[:, None]) + sum_term[:, None]
        reach = (self.u + self.tol_u) >= (self.u - self.tol_u).max(axis=0)[None, :]
        self.tol_shift = np.where(reach, self.tol_u, 0.0).max(axis=0)
        abs_u, abs_e = np.abs(self.u).astype(np.float64), np.abs(self.e).astype(np.float64)
        self.tol_e = self.tol_u + self.tol_shift[None, :] + EPS * (abs_u + abs_e)
        b = self.b.astype(np.float64)       # (only scales a bound; an exact 0 below the subnormals)
        self.tol_b = (self.tol_e + 2.0 * 2.0 ** -52) * b
        below = self.b < LD(MIN_NORMAL)
        self.tol_b[below] = np.maximum(self.tol_b[below], 4.0 * SUBNORMAL_SPACING)
        self.tol_be = abs_e * self.tol_b + b * self.tol_e + self.tol_b * self.tol_e
        t = (self.tol_u + EPS * (abs_u + abs_e)).astype(LD)
        weight = np.exp(self.u - self.topic_lse[:, None])
        self.tol_lse = np.log1p((weight * np.expm1(t)).sum(axis=1)).astype(np.float64) + n * 2.0 ** -52
        self.must_be_zero = self.b < LD(2.0) ** -1075

    def pairs(self):
        """(name, reference, bound) of the six outputs, the tables topic-major."""
        return [("psi_rowsum", self.psi_rowsum, self.tol_rowsum), ("shift", self.shift, self.tol_shift),
                ("elog", self.e, self.tol_e), ("expElog", self.b, self.tol_b), ("expElog_elog", self.be, self.tol_be),
                ("topic_lse", self.topic_lse, self.tol_lse)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def structure_faults(out, K, V):
    """What is exact about the tables of ANY eta, checked bit for bit on `out` (the dict Context.test_tables returns:
    V x ldk tables, padding included).  A list of complaints, empty when there are none."""
    faults = []
    ldk = out["elog"].shape[1]
    for name in TABLES:
        if not np.all(np.isfinite(out[name])):
            faults.append("%s is not finite everywhere" % name)
    for name in ("elog", "expElog", "expElog_elog"):
        if out[name].shape != (V, ldk):
            faults.append("%s has shape %s" % (name, out[name].shape))
        if np.any(bits(out[name][:, K:]) != 0):
            faults.append("%s: padding columns %d..%d are not +0.0 bit for bit" % (name, K, ldk - 1))
    e, b, be = out["elog"][:, :K], out["expElog"][:, :K], out["expElog_elog"][:, :K]
    if np.any(b < 0.0) or np.any(b > 1.0) or np.any(b.max(axis=1) != 1.0):
        faults.append("expElog leaves [0, 1] or the largest of a row is not exactly 1")
    # shift[w] is the largest of the table's own unshifted values exactly when no e = fl(raw - shift) is positive and one
    # of them is 0 (fl(a - b) <= 0 where a <= b, and 0 only where a == b): the unshifted values themselves are not kept
    if np.any(e > 0.0) or np.any(e.max(axis=1) != 0.0):
        faults.append("shift is not the maximum of the row's own unshifted values: elog is positive, or none of a row is 0")
    if np.any(np.isnan(be)):
        faults.append("expElog_elog holds a NaN")
    if np.any(bits(be)[b == 0.0] != 0):
        faults.append("expElog_elog is not +0.0 where expElog is 0")
    if np.any(be > 0.0):
        faults.append("expElog_elog is positive")
    return faults


def compare(out, ref):
    """`out` (V x ldk tables) against the reference: (complaints, {table: (worst error / bound, where)})."""
    K, V = ref.K, ref.V
    faults = structure_faults(out, K, V)
    if out["elog"].shape[1] != ref.ldk:
        faults.append("table stride %d, expected %d" % (out["elog"].shape[1], ref.ldk))
    worst = {}
    for name, want, tol in ref.pairs():
        got = out[name] if out[name].ndim == 1 else out[name][:, :K].T
        with np.errstate(all="ignore"):
            ratio = np.abs(got.astype(LD) - want).astype(np.float64) / tol
        ratio[np.isnan(got)] = np.inf
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        worst[name] = (float(ratio[at]), tuple(int(i) for i in at))
        if ratio[at] > 1.0:
            faults.append("%s: error / bound %.3g at %s (got %r, reference %r)" % (name, ratio[at], worst[name][1],
                                                                                   float(got[at]), float(want[at])))
    zero = out["expElog"][:, :K].T[ref.must_be_zero]
    if np.any(bits(zero) != 0):
        faults.append("expElog is not an exact 0 at %d entries whose reference is below 2^-1075" % int(np.sum(bits(zero) != 0)))
    return faults, worst


def report(label, worst):
    for name in TABLES:
        print("%s %s: worst error / bound %.3f at %s" % (label, name, worst[name][0], worst[name][1]))

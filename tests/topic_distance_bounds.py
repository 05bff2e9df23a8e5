"""Error bounds of the topic distances against their exact values: derived from the operations the
device performs, not tuned to what it returns.  u = 2^-53 is the unit roundoff of a correctly rounded fp64 operation.

The transform.  s is a sum of non-negative entries: an entry passes through at most n_s = ceil(V / 64) + 6 additions
(its lane's, then the tree's), so s_hat = s (1 + theta), |theta| <= n_s u.  p_hat = t / s_hat rounded once:
p_hat = p (1 + e), |e| <= E_P = (n_s + 1) u.

Hellinger.  sa_hat = sqrt(p_hat) rounded once = sqrt(p) (1 + e / 2) (1 + d): relative error E_P / 2 + u a side.  The
product adds u, and a term passes through at most n = min(V, SEGMENT) + segments additions, each (1 + d):
|BC_hat - BC| <= (E_P + 2 u + u + n u) sum_v sqrt(p_v q_v).

Jensen-Shannon.  The device sums f(p, q) = p ln p + q ln q - (p + q) ln m, m = (p + q) / 2, and halves the finished sum,
which is exact: the bound of the sum, below, is halved with it.  With A = sum_v (p |lp| + q |lq| + (p + q) |lm|)
and T = sum_v (|p (lp - lm)| + |q (lq - lm)|):
  the logs        LOG_ULP 2^-53 A: lp, lq and lm are each LOG_ULP off at most, weighted by p, q and p + q.  LOG_ULP = 3 is
                  the accuracy the OpenCL C specification asks of an fp64 log, which the device math library implements
  the inputs      df/dp = ln(p / m): p_hat and q_hat in place of p and q move the sum by at most E_P T
  the operations  p + q (moves lm by u, weighted p + q: at most 2 u over all words, as sum p = sum q = 1), lp - lm, the
                  product, twice, and the add of the two products: at most 3 u T + 2 u
  the additions   (n + 1) u T
Second-order terms are covered by the factor 1.01.
"""
import numpy as np

import topic_distance_restatement as spec

U = 2.0 ** -53
LOG_ULP = 3
SLACK = 1.01


def _depths(V):
    n_s = -(-V // spec.WAVE) + 6
    n = min(V, spec.SEGMENT) + -(-V // spec.SEGMENT)
    return n_s, n


def hellinger_bound(a, b=None):
    """(Ka, Kb): |BC of the device's arithmetic - the exact BC| is at most this."""
    a = np.asarray(a, dtype=np.float64)
    n_s, n = _depths(a.shape[1])
    sa = spec.transform(a, "hellinger")
    sb = sa if b is None else spec.transform(b, "hellinger")
    weight = sa @ sb.T
    return SLACK * U * ((n_s + 1) + 3 + n) * weight


def jensen_shannon_weights(a, b=None):
    """(A, T), both (Ka, Kb)."""
    a = np.asarray(a, dtype=np.float64)
    p_all, lp_all = spec.transform(a, "jensen_shannon")
    q_all, lq_all = (p_all, lp_all) if b is None else spec.transform(b, "jensen_shannon")
    A = np.zeros((p_all.shape[0], q_all.shape[0]))
    T = np.zeros_like(A)
    for v in range(a.shape[1]):
        p, lp = p_all[:, v, np.newaxis], lp_all[:, v, np.newaxis]
        q, lq = q_all[np.newaxis, :, v], lq_all[np.newaxis, :, v]
        m = 0.5 * (p + q)
        with np.errstate(divide="ignore"):
            lm = np.where(m == 0.0, 0.0, np.log(m))
        A += p * np.abs(lp) + q * np.abs(lq) + (p + q) * np.abs(lm)
        T += np.abs(p * (lp - lm)) + np.abs(q * (lq - lm))
    return A, T


def jensen_shannon_bound(a, b=None):
    """(Ka, Kb): |JS of the device's arithmetic - the exact JS| is at most this."""
    n_s, n = _depths(np.asarray(a).shape[1])
    A, T = jensen_shannon_weights(a, b)
    return 0.5 * SLACK * U * (LOG_ULP * A + (n_s + 1) * T + 3 * T + 2 + (n + 1) * T)


def bound(a, b, metric):
    return hellinger_bound(a, b) if metric == "hellinger" else jensen_shannon_bound(a, b)

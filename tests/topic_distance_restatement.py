"""Topic distances between two models, restated in numpy: the row transform, both metrics, the order
of the sum over the words - and the cases of the mpmath golden (tests/golden/make_topic_distance_mp.py), rebuilt from seeds.

  row sum      lane l of 64 adds the entries t_v with v = l (mod 64) in ascending v, from +0.0; the 64 partials go through
               the tree x_l = x_l + x_(l xor m), m = 32, 16, 8, 4, 2, 1; s is lane 0's
  transform    p_v = t_v / s; hellinger keeps sqrt(p_v); jensen_shannon keeps p_v and lp_v = log(p_v), 0 where p_v is 0
  pair sum     V in segments of SEGMENT words; a segment's sum starts at +0.0 and adds its terms in ascending v; the
               segments' sums are added in ascending order from +0.0; every operation rounded once
  hellinger    term = sa_v * sb_v: the Bhattacharyya coefficient
  jensen_shannon  m = 0.5 * (p + q), lm = log(m), term = p * (lp - lm) + q * (lq - lm), exactly 0 where m == 0; the terms
               sum to KL(p || m) + KL(q || m), and the divergence (nats) is the finished sum times 0.5 - exact

The device's Hellinger numbers equal these bit for bit.  Its Jensen-Shannon numbers differ by its log against numpy's:
tests/topic_distance_bounds.py bounds that.
"""
import hashlib

import numpy as np

WAVE = 64
TILE = 32           # rows of either table of a workgroup (kTdTile)
CHUNK = 32          # words of a chunk through LDS (kTdChunk)
SEGMENT = 1024      # words of a segment (kTdSegment)
METRICS = {"hellinger": 0, "jensen_shannon": 1}


def row_sums(table):
    table = np.asarray(table, dtype=np.float64)
    rows, V = table.shape
    lanes = np.zeros((rows, WAVE))
    for v0 in range(0, V, WAVE):
        width = min(WAVE, V - v0)
        lanes[:, :width] = lanes[:, :width] + table[:, v0:v0 + width]
    for m in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, np.arange(WAVE) ^ m]
    return lanes[:, 0].copy()


def transform(table, metric):
    """hellinger: sqrt(p); jensen_shannon: (p, lp)."""
    table = np.asarray(table, dtype=np.float64)
    p = table / row_sums(table)[:, np.newaxis]
    if metric == "hellinger":
        return np.sqrt(p)
    with np.errstate(divide="ignore"):
        lp = np.where(p == 0.0, 0.0, np.log(p))
    return p, lp


def _terms(ta, tb, metric, v):
    if metric == "hellinger":
        return ta[:, v, np.newaxis] * tb[np.newaxis, :, v]
    (p_all, lp_all), (q_all, lq_all) = ta, tb
    p, lp = p_all[:, v, np.newaxis], lp_all[:, v, np.newaxis]
    q, lq = q_all[np.newaxis, :, v], lq_all[np.newaxis, :, v]
    m = 0.5 * (p + q)
    with np.errstate(divide="ignore", invalid="ignore"):
        lm = np.log(m)
        term = p * (lp - lm) + q * (lq - lm)
    return np.where(m == 0.0, 0.0, term)


def values(a, b=None, metric="jensen_shannon", segment=SEGMENT, segment_order=None):
    """(Ka, Kb): the Bhattacharyya coefficients or the Jensen-Shannon divergences of the rows of a against those of b
    (None: a).  segment / segment_order exist for the tests that show the order matters."""
    a = np.asarray(a, dtype=np.float64)
    ta = transform(a, metric)
    tb = ta if b is None else transform(b, metric)
    Ka, V = a.shape
    Kb = Ka if b is None else np.asarray(b).shape[0]
    starts = list(range(0, V, segment))
    total = np.zeros((Ka, Kb))
    for v_begin in (starts if segment_order is None else [starts[i] for i in segment_order]):
        acc = np.zeros((Ka, Kb))
        for v in range(v_begin, min(V, v_begin + segment)):
            acc = acc + _terms(ta, tb, metric, v)
        total = total + acc
    return 0.5 * total if metric == "jensen_shannon" else total


def distance(numbers, metric):
    numbers = np.asarray(numbers, dtype=np.float64)
    return np.sqrt(np.maximum(0.0, 1.0 - numbers if metric == "hellinger" else numbers))


# ---- the cases of the mpmath golden: rebuilt from seeds (numpy's frozen RandomState streams), tied to it by a hash ----
CASES = ("one", "two_words", "odd", "segment_edge", "zeros", "disjoint", "identical", "scaled", "peaked")


def case(name):
    """(a (Ka, V), b (Kb, V)) of a golden case."""
    rng = np.random.RandomState(20000 + CASES.index(name))
    rows = lambda K, V: rng.gamma(0.4, size=(K, V)) + 2.0 ** -40
    if name == "one":
        return np.array([[3.0]]), np.array([[0.5]])
    if name == "two_words":
        return rows(3, 2), rows(3, 2)
    if name == "odd":
        return rows(5, 17), rows(4, 17)
    if name == "segment_edge":
        return rows(65, SEGMENT + 1), rows(2, SEGMENT + 1)
    if name == "zeros":
        a, b = rows(4, 40), rows(4, 40)
        a[rng.random_sample(a.shape) < 0.5] = 0.0
        b[rng.random_sample(b.shape) < 0.5] = 0.0
        a[:, 0], b[:, 1] = 1.0, 1.0                     # (no row without an entry)
        return a, b
    if name == "disjoint":
        a, b = rows(2, 10), rows(2, 10)
        a[:, 5:], b[:, :5] = 0.0, 0.0
        return a, b
    if name == "identical":
        a = rows(3, 33)
        return a, a.copy()
    if name == "scaled":
        a = rows(3, 50)
        return a, a * np.array([1e-12, 1e6, 1.0])[:, np.newaxis]
    if name == "peaked":
        a, b = rows(2, 70), rows(3, 70)
        for table in (a, b):
            table[:] = table / row_sums(table)[:, np.newaxis] * 1e-12
            table[:, 7] = 1.0 - 1e-12
        b[2, 7], b[2, 8] = b[2, 8], b[2, 7]             # (one row peaked at another word)
        return a, b
    raise KeyError(name)


def digest(a, b):
    h = hashlib.sha256()
    for table in (a, b):
        table = np.ascontiguousarray(table, dtype=np.float64)
        h.update(np.array(table.shape, dtype=np.int64).tobytes())
        h.update(table.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()

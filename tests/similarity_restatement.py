"""The arithmetic of the nearest-documents pass restated in numpy, for tests that hold the device to
equality.  Rows are K doubles.

  transform(rows, t)          0: the rows as given; 1: theta_k = g_k / s with s = (((+0.0 + g_0) + g_1) + ...) in k order,
                              one s per row; 2: sqrt(theta_k).  numpy's divide and sqrt of doubles are correctly rounded.
  scores(a, b)                s[q][d] = (((+0.0 + a_0 b_0) + a_1 b_1) + ...): the k loop, one rounded multiply and one
                              rounded add per step, elementwise over the (Q, D) array
  top(scores, N, self_ids)    per query the first N documents by "larger score first, among equal scores the smaller index
                              first" (lexsort on (id, -score)), leaving out document self_ids[q] (-1: none); fewer than N
                              candidates: trailing ids -1, scores -inf
  brute_*                     the same per pair in plain Python, for cross-checking the above
"""
import math

import numpy as np


def row_sums(rows):
    rows = np.asarray(rows, dtype=np.float64)
    s = np.zeros(len(rows))
    for k in range(rows.shape[1]):
        s = s + rows[:, k]
    return s


def transform(rows, t):
    rows = np.asarray(rows, dtype=np.float64)
    if t == 0:
        return rows.copy()
    theta = rows / row_sums(rows)[:, None]
    return theta if t == 1 else np.sqrt(theta)


def scores(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    acc = np.zeros((len(a), len(b)))
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * b[None, :, k]
    return acc


def top(score, N, self_ids=None):
    score = np.asarray(score, dtype=np.float64)
    Q, D = score.shape
    ids = np.full((Q, N), -1, dtype=np.int32)
    values = np.full((Q, N), -np.inf)
    for q in range(Q):
        order = np.lexsort((np.arange(D), -score[q]))
        if self_ids is not None and self_ids[q] >= 0:
            order = order[order != self_ids[q]]
        order = order[:N]
        ids[q, :len(order)] = order
        values[q, :len(order)] = score[q, order]
    return ids, values


def nearest(base, base_transform, queries, query_transform, N, self_ids=None):
    """What pylda_similarity_set_base + pylda_similar_documents return."""
    return top(scores(transform(queries, query_transform), transform(base, base_transform)), N, self_ids)


def hellinger(affinity, ids):
    affinity = np.asarray(affinity, dtype=np.float64)
    out = np.full(affinity.shape, np.inf)
    for at in np.ndindex(*affinity.shape):
        if ids[at] >= 0:
            out[at] = math.sqrt(max(0.0, 1.0 - float(affinity[at])))
    return out


# ---- per pair, in plain Python (floats are IEEE doubles; every operation below is rounded once) ----
def brute_transform(rows, t):
    out = []
    for g in rows:
        g = [float(x) for x in g]
        if t == 0:
            out.append(g)
            continue
        s = 0.0
        for x in g:
            s = s + x
        out.append([x / s if t == 1 else math.sqrt(x / s) for x in g])
    return out


def brute_scores(a, b):
    out = []
    for x in a:
        row = []
        for y in b:
            acc = 0.0
            for k in range(len(x)):
                acc = acc + float(x[k]) * float(y[k])
            row.append(acc)
        out.append(row)
    return out


def brute_top(score, N, self_ids=None):
    """[(id, score)] per query, padded with (-1, -inf): selection by repeated search for the first entry of the order."""
    out = []
    for q, row in enumerate(score):
        left = [d for d in range(len(row)) if self_ids is None or d != self_ids[q]]
        picked = []
        while left and len(picked) < N:
            best = left[0]
            for d in left[1:]:
                if row[d] > row[best] or (row[d] == row[best] and d < best):
                    best = d
            left.remove(best)
            picked.append((best, row[best]))
        out.append(picked + [(-1, -math.inf)] * (N - len(picked)))
    return out

"""Reference of the sufficient-statistics pass (pylda_amd/csrc/sstats_kernels.h, sstats_sweep.h, sstats_live.h) and the
synthetic cases tests/test_gpu_sstats.py runs it on.  No GPU, no native code: numpy integers.

The pass computes sstats[w][k] = B[w][k] * sum_d r_dw t'_d[k], where t'_d is the document's dense row of t or - for a
document that left a list of live topics - the scatter of that list (its dense row is then never read).  With integer
inputs, 1 <= t < 2^12 and 1 <= r < 2^8, and D <= 1024 documents every partial sum is an integer below 2^30, far inside
2^53: the sum is exact in fp64 in ANY order, so the device's sums must equal reference_sums() bit for bit and the
statistics one fp64 multiply of them.

The corpus (build_corpus) aims at the edges the kernels have:
  * D = 643 documents: no multiple of 8, 24 or 40; at 40 document blocks (17 documents each) the last two hold none;
  * every light term v has a posting in document v % D - except EMPTY_RUN (31 terms across the multiples 48 and 64 of
    16), term 0 and term V - 1, which have none; those with v % 3 == 1 have a second one, so that the persistent sweep's
    dealing by posting count puts terms of more than one posting into slots beyond the first of a wavefront;
  * heavy terms with HEAVY_COUNTS postings - 2 .. 70 (the 4 x 64 / LR unrolls and their tails, the pair loop's odd tail,
    chunks of 63 / 64 / 65 postings, n % 4 of every kind), 127 .. 129, 191 .. 193, 255 .. 258 (the plain cut at 256),
    511 .. 513, and 643, one in every document (81 postings per block at 8 blocks: a second segment of the sweep's cut at
    64 within a block) - each three times: in consecutive documents from document 0, in consecutive documents up to the
    last, and spread evenly over the documents.
Document 0 is never empty: the bulk, sweep and live kernels read row 0 with factor 0 for the lanes past a chunk.
"""
import math

import numpy as np

D_DEFAULT = 643
HEAVY_COUNTS = tuple(range(2, 71)) + (127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 511, 512, 513, 643)
EMPTY_RUN = tuple(range(40, 71))                # 31 terms, across the multiples 48 and 64 of 16
LIST_LENGTHS = (1, 11, 12, 13, 24, 25, 59, 60)  # one entry, around one and two 128-byte lines of twelve, the last line
LIST_STRIDE = 60
T_LIMIT, R_LIMIT, D_LIMIT, SUM_LIMIT = 1 << 12, 1 << 8, 1024, 1 << 30
MIXES = ("all", "none", "third")                # every document listed, none, every third one (d % 3 == 2) without a list


def table_stride(K):
    """host_plan.h table_stride_for"""
    for s in (16, 32, 64, 128, 256):
        if K <= s:
            return s
    return (K + 127) // 128 * 128 if K <= 1024 else (K + 63) // 64 * 64


def empty_terms(V):
    return (0,) + EMPTY_RUN + (V - 1,)


class Corpus(object):
    """CSR of the synthetic corpus (term ids ascending within a document, every count 1) and what the tests ask about it."""

    def __init__(self, V, D, doc_ptr, term_id, heavy):
        self.V, self.D = V, D
        self.doc_ptr, self.term_id = doc_ptr, term_id
        self.term_ct = np.ones(term_id.size, dtype=np.int32)
        self.nnz = int(term_id.size)
        self.heavy = heavy                      # (postings, placement) -> term
        self.doc_of = np.repeat(np.arange(D, dtype=np.int64), np.diff(doc_ptr))     # document of every CSR position
        self.by_term = np.argsort(term_id, kind="stable")                            # CSR positions in postings order
        self.postings = np.bincount(term_id, minlength=V).astype(np.int64)           # per term

    def segments(self, blocks=1, cap=256):
        """Segments of every term's postings: cut at the boundaries of `blocks` document blocks and at `cap` postings
        (host_plan.cpp cut_segments_plain / cut_segments_blocked)."""
        per_block = (self.D + blocks - 1) // blocks
        pairs = self.term_id[self.by_term].astype(np.int64) * blocks + self.doc_of[self.by_term] // per_block
        in_block = np.bincount(pairs, minlength=self.V * blocks).reshape(self.V, blocks)
        return ((in_block + cap - 1) // cap).sum(axis=1)


def build_corpus(V, D=D_DEFAULT):
    empty = set(empty_terms(V))
    free = [v for v in range(V) if v not in empty]
    assert len(empty) == 33 and V - 1 > EMPTY_RUN[-1] and len(free) >= 3 * len(HEAVY_COUNTS), V
    # heavy terms spread over the vocabulary (the rounds of the gather and the pieces of the segment cut all get some)
    step = len(free) // (3 * len(HEAVY_COUNTS))
    pairs, heavy = [], {}
    for i, (count, place) in enumerate((c, p) for c in HEAVY_COUNTS for p in ("head", "tail", "spread")):
        term = free[i * step]
        heavy[(count, place)] = term
        if place == "head":
            docs = np.arange(count)
        elif place == "tail":
            docs = np.arange(D - count, D)
        else:
            docs = np.arange(count) * D // count
        assert np.unique(docs).size == count and docs.min() >= 0 and docs.max() < D
        pairs.append(docs.astype(np.int64) * V + term)
    light = set(free) - set(heavy.values())             # (a heavy term has exactly its count of postings)
    terms = np.array(sorted(light), dtype=np.int64)
    pairs.append((terms % D) * V + terms)
    second = terms[terms % 3 == 1]
    pairs.append(((second // 3 * 5 + 3) % D) * V + second)
    keys = np.unique(np.concatenate(pairs))             # (document, term) pairs, sorted by document, then term
    docs, term_id = keys // V, (keys % V).astype(np.int32)
    doc_ptr = np.zeros(D + 1, dtype=np.int64)
    np.cumsum(np.bincount(docs, minlength=D), out=doc_ptr[1:])
    corpus = Corpus(V, D, doc_ptr, term_id, heavy)
    assert doc_ptr[1] > 0, "document 0 is empty"
    assert all(corpus.postings[v] == 0 for v in empty) and np.count_nonzero(corpus.postings == 0) == 33
    for (count, place), term in heavy.items():
        assert corpus.postings[term] == count
    return corpus


def _lists(rng, D, K, mix, draw_t):
    """The documents' lists: lengths cycle through LIST_LENGTHS (capped by K), distinct topics, topics 0 and K - 1 both
    present wherever the list has room for two."""
    live_n = np.full(D, -1, dtype=np.int32)
    live_topic = np.zeros((D, LIST_STRIDE), dtype=np.uint16)
    live_t = np.zeros((D, LIST_STRIDE), dtype=np.float64)
    for d in range(D):
        if mix == "none" or (mix == "third" and d % 3 == 2):
            continue
        n = min(LIST_LENGTHS[d % len(LIST_LENGTHS)], K)
        topics = rng.permutation(K)[:n]
        if n >= 2 and K >= 2:
            topics = np.concatenate(([0, K - 1], [k for k in topics if k not in (0, K - 1)]))[:n]
            topics = rng.permutation(topics)
        live_n[d] = n
        live_topic[d, :n] = topics
        live_t[d, :n] = draw_t(n)
    return live_n, live_topic, live_t


def integer_inputs(corpus, K, seed=0, mix=None):
    """t (D, stride) and r (nnz) as integers in fp64 - padding columns of t included - and, with a mix, the lists.  The
    dense rows of listed documents are NaN: the pass must not read them."""
    assert corpus.D <= D_LIMIT and corpus.D * (T_LIMIT - 1) * (R_LIMIT - 1) < SUM_LIMIT
    rng = np.random.default_rng(seed)
    ldk = table_stride(K)
    case = {"K": K, "ldk": ldk,
            "t": rng.integers(1, T_LIMIT, size=(corpus.D, ldk)).astype(np.float64),
            "r": rng.integers(1, R_LIMIT, size=corpus.nnz).astype(np.float64),
            "live_n": None, "live_topic": None, "live_t": None}
    if mix is not None:
        case["live_n"], case["live_topic"], case["live_t"] = _lists(
            rng, corpus.D, K, mix, lambda n: rng.integers(1, T_LIMIT, size=n).astype(np.float64))
        case["t"][case["live_n"] >= 0] = np.nan
    check_integer_case(corpus, case)
    return case


def check_integer_case(corpus, case):
    """Every input an integer, 1 <= t < 2^12 and 1 <= r < 2^8 (NaN only in the dense rows of listed documents)."""
    t, r, live_n = case["t"], case["r"], case["live_n"]
    dense = np.ones(corpus.D, dtype=bool) if live_n is None else live_n < 0
    values = [t[dense].ravel()]
    if live_n is not None:
        assert np.all(np.isnan(t[~dense]))
        values.append(np.concatenate([case["live_t"][d, :n] for d, n in enumerate(live_n) if n > 0] or [np.ones(1)]))
    for v in values:
        assert np.all(v == np.floor(v)) and np.all(v >= 1) and np.all(v < T_LIMIT)
    assert np.all(r == np.floor(r)) and np.all(r >= 1) and np.all(r < R_LIMIT)
    assert t.shape == (corpus.D, case["ldk"]) and r.shape == (corpus.nnz,)


def real_inputs(corpus, K, seed=0, mix=None):
    """t uniform in (0, 1), r uniform in (0, 4): every addend of every sum is positive."""
    rng = np.random.default_rng(seed)
    ldk = table_stride(K)
    draw = lambda size: np.maximum(rng.random(size), 2.0 ** -30)
    case = {"K": K, "ldk": ldk, "t": draw((corpus.D, ldk)), "r": 4.0 * draw(corpus.nnz),
            "live_n": None, "live_topic": None, "live_t": None}
    if mix is not None:
        case["live_n"], case["live_topic"], case["live_t"] = _lists(rng, corpus.D, K, mix, draw)
        case["t"][case["live_n"] >= 0] = np.nan
    return case


def effective_rows(case, dtype):
    """t' (D, stride): the dense row, or the scatter of the document's list."""
    t, live_n = case["t"], case["live_n"]
    if live_n is None:
        return t.astype(dtype)
    rows = np.zeros(t.shape, dtype=dtype)
    rows[live_n < 0] = t[live_n < 0].astype(dtype)
    for d in np.nonzero(live_n > 0)[0]:
        n = live_n[d]
        np.add.at(rows[d], case["live_topic"][d, :n].astype(np.int64), case["live_t"][d, :n].astype(dtype))
    return rows


def reference_sums(corpus, case, columns=256):
    """s[w][k] = sum_d r_dw t'_d[k] as int64, (V, stride)."""
    rows = effective_rows(case, np.int64)
    order = corpus.by_term
    docs, r = corpus.doc_of[order], case["r"][order].astype(np.int64)
    assert np.array_equal(r, case["r"][order])
    s = np.zeros((corpus.V, case["ldk"]), dtype=np.int64)
    have = np.nonzero(corpus.postings)[0]
    first = np.concatenate(([0], np.cumsum(corpus.postings)))[have]
    for c0 in range(0, case["ldk"], columns):
        s[have, c0:c0 + columns] = np.add.reduceat(r[:, None] * rows[docs, c0:c0 + columns], first, axis=0)
    assert s.max(initial=0) < SUM_LIMIT
    return s


def brute_force_sums(V, doc_ptr, term_id, case):
    """The same by the definition, one posting and one topic at a time (small cases)."""
    ldk, live_n = case["ldk"], case["live_n"]
    s = [[0] * ldk for _ in range(V)]
    for d in range(len(doc_ptr) - 1):
        if live_n is None or live_n[d] < 0:
            row = [int(x) for x in case["t"][d]]
        else:
            row = [0] * ldk
            for j in range(live_n[d]):
                row[int(case["live_topic"][d, j])] += int(case["live_t"][d, j])
        for i in range(int(doc_ptr[d]), int(doc_ptr[d + 1])):
            for k in range(ldk):
                s[int(term_id[i])][k] += int(case["r"][i]) * row[k]
    return np.array(s, dtype=np.int64).reshape(V, ldk)


def _split(a):
    """Veltkamp: a = hi + lo, both of at most 26 significant bits, so that products of parts are exact."""
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def real_reference(corpus, case):
    """sum_d r_dw t'_d[k] correctly rounded: math.fsum over the EXACT products (four products of 26-bit parts each),
    (V, stride) float64, columns K .. stride-1 left 0."""
    rows = effective_rows(case, np.float64)
    K = case["K"]
    out = np.zeros((corpus.V, case["ldk"]), dtype=np.float64)
    start = np.concatenate(([0], np.cumsum(corpus.postings)))
    for w in np.nonzero(corpus.postings)[0]:
        at = corpus.by_term[start[w]:start[w + 1]]
        rh, rl = _split(case["r"][at][:, None])
        th, tl = _split(rows[corpus.doc_of[at], :K])
        parts = np.concatenate((rh * th, rh * tl, rl * th, rl * tl), axis=0)
        out[w, :K] = [math.fsum(column) for column in parts.T.tolist()]
    return out

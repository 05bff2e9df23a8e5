"""tests/sstats_reference.py against the definition - a brute-force loop over postings and topics - and against a case
worked by hand, and its case builder against what tests/test_gpu_sstats.py relies on: integer inputs whose every partial
sum stays below 2^30, and a corpus with the posting counts and the empty terms the kernels' edges need.  No GPU."""
import numpy as np
import pytest

import sstats_reference as sr


def small_corpus(V=90, D=17, seed=3):
    rng = np.random.default_rng(seed)
    present = rng.random((D, V)) < 0.2
    present[:, [0, V - 1]] = False
    present[0, 5] = True
    docs, terms = np.nonzero(present)
    doc_ptr = np.zeros(D + 1, dtype=np.int64)
    np.cumsum(np.bincount(docs, minlength=D), out=doc_ptr[1:])
    return sr.Corpus(V, D, doc_ptr, terms.astype(np.int32), {})


@pytest.mark.parametrize("K,mix", [(5, None), (20, None), (20, "all"), (20, "third"), (70, "third"), (3, "all"), (20, "none")])
def test_reference_is_the_brute_force_sum(K, mix):
    corpus = small_corpus()
    case = sr.integer_inputs(corpus, K, seed=K, mix=mix)
    got = sr.reference_sums(corpus, case, columns=16)
    assert got.dtype == np.int64 and got.shape == (corpus.V, sr.table_stride(K))
    assert np.array_equal(got, sr.brute_force_sums(corpus.V, corpus.doc_ptr, corpus.term_id, case))
    assert not got[0].any() and not got[corpus.V - 1].any() and got[5].any()
    if mix == "all":        # nothing beyond the listed topics, in particular not the padding columns
        assert not got[:, K:].any()


def test_reference_on_a_case_worked_by_hand():
    # three documents over four terms; document 1 left the list {topic 2: 7, topic 0: 3} and its dense row is NaN
    doc_ptr = np.array([0, 2, 4, 5], dtype=np.int64)
    term_id = np.array([0, 2, 0, 3, 2], dtype=np.int32)
    corpus = sr.Corpus(4, 3, doc_ptr, term_id, {})
    t = np.zeros((3, 16))
    t[0, :3], t[1], t[2, :3] = [1, 2, 3], np.nan, [10, 20, 30]
    live_topic, live_t = np.zeros((3, 60), dtype=np.uint16), np.zeros((3, 60))
    live_topic[1, :2], live_t[1, :2] = [2, 0], [7, 3]
    case = {"K": 3, "ldk": 16, "t": t, "r": np.array([2.0, 3.0, 5.0, 4.0, 6.0]),
            "live_n": np.array([-1, 2, -1], dtype=np.int32), "live_topic": live_topic, "live_t": live_t}
    want = np.zeros((4, 16), dtype=np.int64)
    want[0, :3] = [2 * 1 + 5 * 3, 2 * 2, 2 * 3 + 5 * 7]            # documents 0 (r = 2) and 1 (r = 5, the list)
    want[2, :3] = [3 * 1 + 6 * 10, 3 * 2 + 6 * 20, 3 * 3 + 6 * 30]  # documents 0 (r = 3) and 2 (r = 6)
    want[3, :3] = [4 * 3, 0, 4 * 7]                                  # document 1 (r = 4, the list)
    assert np.array_equal(sr.reference_sums(corpus, case), want)
    assert np.array_equal(sr.brute_force_sums(4, doc_ptr, term_id, case), want)
    # without the lists document 1's dense row counts: make it a row of ones
    dense = dict(case, t=np.where(np.isnan(t), 1.0, t), live_n=None)
    assert sr.reference_sums(corpus, dense)[3, :3].tolist() == [4, 4, 4]
    # the real-valued reference agrees on integers, where every sum is exact
    assert np.array_equal(sr.real_reference(corpus, case), want.astype(np.float64))


def test_real_reference_is_the_exact_sum():
    from fractions import Fraction
    corpus = small_corpus(V=30, D=9)
    case = sr.real_inputs(corpus, 4, seed=1, mix="third")
    got = sr.real_reference(corpus, case)
    rows = sr.effective_rows(case, np.float64)
    for w in (5, 11, 28):
        for k in range(4):
            exact = sum((Fraction(float(case["r"][i])) * Fraction(float(rows[corpus.doc_of[i], k]))
                         for i in np.nonzero(corpus.term_id == w)[0]), Fraction(0))
            assert got[w, k] == float(exact), (w, k)        # (float(Fraction) rounds correctly)
    assert np.all(case["r"] > 0) and np.all(case["r"] < 4) and np.all(rows >= 0) and np.all(rows < 1)


@pytest.mark.parametrize("V", [300, 700, 20000])
def test_corpus_has_the_edges(V):
    corpus = sr.build_corpus(V)
    D = corpus.D
    assert D == 643 and all(D % n for n in (8, 24, 40)) and 38 * ((D + 39) // 40) >= D
    assert corpus.doc_ptr[1] > 0                                   # document 0 is not empty
    for d in range(D):                                             # term ids ascending and distinct within a document
        ids = corpus.term_id[corpus.doc_ptr[d]:corpus.doc_ptr[d + 1]]
        assert np.all(np.diff(ids) > 0)
    empty = np.nonzero(corpus.postings == 0)[0]
    assert empty.tolist() == sorted(sr.empty_terms(V)) and empty.size == 33
    assert any(v % 16 == 0 for v in sr.EMPTY_RUN) and len(sr.EMPTY_RUN) == 31
    assert len(corpus.heavy) == 3 * len(sr.HEAVY_COUNTS)
    for (count, place), term in corpus.heavy.items():
        docs = corpus.doc_of[corpus.by_term][np.searchsorted(corpus.term_id[corpus.by_term], term, "left"):
                                             np.searchsorted(corpus.term_id[corpus.by_term], term, "right")]
        assert docs.size == count and np.all(np.diff(docs) > 0)   # postings in document order
        if place == "head":
            assert docs[0] == 0 and docs[-1] == count - 1
        elif place == "tail":
            assert docs[0] == D - count and docs[-1] == D - 1
        else:
            assert docs[0] == 0 and np.max(np.diff(docs, prepend=0)) <= D // count + 1
    light = np.setdiff1d(np.nonzero(corpus.postings)[0], list(corpus.heavy.values()))
    first_doc = corpus.doc_of[corpus.by_term][np.concatenate(([0], np.cumsum(corpus.postings)))[light]]
    assert np.all(corpus.postings[light] <= 2) and np.count_nonzero(corpus.postings[light] == 2) > len(light) // 4
    has = np.zeros((V, D), dtype=bool)
    has[corpus.term_id, corpus.doc_of] = True
    assert np.all(has[light, light % D]) and first_doc.size == light.size
    # segments: the plain cut at 256, the sweep's cut at 64 inside 8 blocks of 81 documents
    everywhere = corpus.heavy[(643, "head")]
    assert corpus.segments()[everywhere] == 3 and corpus.segments(8, 64)[everywhere] == 16
    assert corpus.segments()[corpus.heavy[(256, "tail")]] == 1 and corpus.segments()[corpus.heavy[(257, "tail")]] == 2
    assert corpus.segments(40, 256)[everywhere] == 38


@pytest.mark.parametrize("mix", [None] + list(sr.MIXES))
def test_builder_keeps_every_sum_exact(mix):
    corpus = sr.build_corpus(300)
    for K in (10, 130):
        case = sr.integer_inputs(corpus, K, seed=1, mix=mix)
        sr.check_integer_case(corpus, case)
        dense = np.ones(corpus.D, bool) if case["live_n"] is None else case["live_n"] < 0
        assert np.all(np.isfinite(case["t"][dense])) and np.all(case["t"][dense][:, K:] >= 1)     # padding columns too
        assert corpus.D * (sr.T_LIMIT - 1) * (sr.R_LIMIT - 1) < 2 ** 30 < 2 ** 53
        assert sr.reference_sums(corpus, case).max() < 2 ** 30
        if mix in ("all", "third"):
            n = case["live_n"]
            assert set(n[n >= 0].tolist()) == set(min(x, K) for x in sr.LIST_LENGTHS)
            assert (n < 0).sum() == (0 if mix == "all" else len(range(2, corpus.D, 3)))
            for d in np.nonzero(n >= 2)[0]:
                topics = case["live_topic"][d, :n[d]]
                assert np.unique(topics).size == n[d] and 0 in topics and K - 1 in topics and topics.max() < K
        elif mix == "none":
            assert np.all(case["live_n"] == -1)
    bad = sr.integer_inputs(corpus, 10, seed=1)
    bad["t"][3, 2] = 0.5
    with pytest.raises(AssertionError):
        sr.check_integer_case(corpus, bad)
    bad["t"][3, 2], bad["r"][7] = 1.0, float(sr.R_LIMIT)
    with pytest.raises(AssertionError):
        sr.check_integer_case(corpus, bad)

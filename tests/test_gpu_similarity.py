"""Nearest documents on the GPU (pylda_similarity_set_base / pylda_similar_documents, similarity_kernels.h) against the numpy
restatement (tests/similarity_restatement.py), and the engines' similar_documents() / top_documents() and
launch_test --similar_documents built on them.  Ids and scores are exact: every comparison is
array_equal, scores by their bits.  The shapes are the small ones at which tiles (64 queries x 128 documents), chunks
(16 k), lists (64 entries) and slices have their edges."""
import ctypes
import os
import pickle

import numpy as np
import pytest

import similarity_restatement as spec

pytestmark = pytest.mark.gpu

V = 5       # (the context wants a vocabulary; nothing here reads it)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _assert_equal(got, want, what=None):
    ids, scores = got
    assert ids.dtype == np.int32 and scores.dtype == np.float64 and ids.shape == scores.shape == want[0].shape, what
    assert np.array_equal(ids, want[0]), (what, int(np.argmax(np.any(ids != want[0], axis=1))))
    assert np.array_equal(_bits(scores), _bits(want[1])), what


@pytest.fixture(scope="module")
def sliced_case():
    """(64, 1000, 130, 10): base, queries and the restatement's answer, computed once."""
    rng = np.random.default_rng(64 + 1000 + 130 + 10)
    base, queries = rng.standard_normal((1000, 130)), rng.standard_normal((64, 130))
    return base, queries, spec.nearest(base, 0, queries, 0, 10)


@pytest.mark.parametrize("Q,D,K,N", [(1, 1, 1, 1), (3, 63, 3, 1), (65, 65, 10, 64), (64, 1000, 130, 10), (130, 257, 128, 64), (2, 5000, 17, 33)])
def test_transform_0_equals_the_restatement(Q, D, K, N, sliced_case):
    from pylda_amd import _capi
    if (Q, D, K, N) == (64, 1000, 130, 10):
        base, queries, want = sliced_case
    else:
        rng = np.random.default_rng(Q + D + K + N)
        base, queries = rng.standard_normal((D, K)), rng.standard_normal((Q, K))
        want = spec.nearest(base, 0, queries, 0, N)
    ctx = _capi.Context(K, V)
    try:
        ctx.similarity_set_base(base, 0)
        got = ctx.similar_documents(queries, N, 0)
        _assert_equal(got, want)
        again = ctx.similar_documents(queries, N, 0)
        assert np.array_equal(again[0], got[0]) and np.array_equal(_bits(again[1]), _bits(got[1]))
    finally:
        ctx.close()


def test_ties_come_in_ascending_id():
    from pylda_amd import _capi
    rng = np.random.default_rng(5)
    K, D, N = 7, 300, 64
    distinct = rng.standard_normal((5, K))
    base = distinct[rng.integers(0, 5, size=D)]
    ctx = _capi.Context(K, V)
    try:
        ctx.similarity_set_base(base, 0)
        ids, scores = ctx.similar_documents(distinct, N, 0)
        _assert_equal((ids, scores), spec.nearest(base, 0, distinct, 0, N))
        for q in range(5):
            for value in np.unique(scores[q]):
                run = ids[q][scores[q] == value]
                assert np.all(np.diff(run) > 0), (q, value)
        assert any(len(np.unique(scores[q])) < N for q in range(5))       # (there were ties to order)
        ctx.similarity_set_base(np.zeros((D, K)), 0)
        ids, scores = ctx.similar_documents(distinct, N, 0)
        assert np.array_equal(ids, np.tile(np.arange(N, dtype=np.int32), (5, 1)))
        _assert_equal((ids, scores), spec.nearest(np.zeros((D, K)), 0, distinct, 0, N))
    finally:
        ctx.close()


def test_same_result_whatever_the_slices(sliced_case):
    from pylda_amd import _capi
    base, queries, want = sliced_case
    ctx = _capi.Context(base.shape[1], V)
    try:
        ctx.similarity_set_base(base, 0)
        for slices in (1, 2, 7, 1000, 0):                                 # (1000: clamped to the 8 tiles of 128 documents)
            ctx.set_option("similarity_doc_slices", slices)
            _assert_equal(ctx.similar_documents(queries, 10, 0), want, slices)
        for bad in (-1, 1025):
            with pytest.raises(_capi.PyldaError) as e:
                ctx.set_option("similarity_doc_slices", bad)
            assert e.value.status == -1
        _assert_equal(ctx.similar_documents(queries, 10, 0), want, "after the refused options")
    finally:
        ctx.close()


def test_self_and_padding():
    from pylda_amd import _capi
    rng = np.random.default_rng(40)
    D, K, N = 40, 6, 64
    rows = rng.standard_normal((D, K))
    own = np.arange(D, dtype=np.int32)
    ctx = _capi.Context(K, V)
    try:
        ctx.similarity_set_base(rows, 0)
        ids, scores = ctx.similar_documents(rows, N, 0, own)
        _assert_equal((ids, scores), spec.nearest(rows, 0, rows, 0, N, own))
        assert not np.any(ids == own[:, None])
        assert np.all(ids[:, :D - 1] >= 0) and np.all(ids[:, D - 1:] == -1) and np.all(scores[:, D - 1:] == -np.inf)
        assert np.all(np.isfinite(scores[:, :D - 1]))
        for nobody in (np.full(D, -1, dtype=np.int32), None):
            ids, scores = ctx.similar_documents(rows, N, 0, nobody)
            _assert_equal((ids, scores), spec.nearest(rows, 0, rows, 0, N))
            assert np.all(np.sort(ids[:, :D], axis=1) == np.arange(D)) and np.all(ids[:, D:] == -1)
        # some queries leave a document out, others none; the document left out need not be the query's own
        mixed = np.where(np.arange(D) % 3 == 0, -1, (np.arange(D) * 7) % D).astype(np.int32)
        _assert_equal(ctx.similar_documents(rows, 5, 0, mixed), spec.nearest(rows, 0, rows, 0, 5, mixed))
    finally:
        ctx.close()


def _gamma_rows(rng, n, K):
    """rng.gamma rows scaled over [1e-12, 1e6]: a scale per row, in every third row a scale per entry; some entries 0.0."""
    rows = rng.gamma(0.5, size=(n, K)) + 1e-300
    rows *= 10.0 ** rng.uniform(-12, 6, size=(n, 1))
    rows[::3] *= 10.0 ** rng.uniform(-9, 0, size=rows[::3].shape)
    if K > 1:
        rows[1::4, rng.integers(0, K)] = 0.0
    return rows


@pytest.mark.parametrize("K", [1, 10, 130])
@pytest.mark.parametrize("t", [1, 2])
def test_transforms_1_and_2_equal_the_restatement(K, t):
    """The device's double divide and sqrt are correctly rounded: theta and sqrt(theta) have numpy's bits, and so do the scores."""
    from pylda_amd import _capi
    rng = np.random.default_rng(100 * K + t)
    base, queries = _gamma_rows(rng, 300, K), _gamma_rows(rng, 70, K)
    ctx = _capi.Context(K, V)
    try:
        ctx.similarity_set_base(base, t)
        _assert_equal(ctx.similar_documents(queries, 10, t), spec.nearest(base, t, queries, t, 10), "both sides")
        # the transformed base by itself: one-hot queries as given read its columns
        ids, scores = ctx.similar_documents(np.eye(K), 64, 0)
        _assert_equal((ids, scores), spec.nearest(base, t, np.eye(K), 0, 64), "columns of the base")
        # ... and the transformed queries by themselves, against a base taken as given
        ctx.similarity_set_base(np.eye(K), 0)
        _assert_equal(ctx.similar_documents(queries, min(K, 64), t), spec.nearest(np.eye(K), 0, queries, t, min(K, 64)), "columns of the queries")
    finally:
        ctx.close()


def test_bad_rows_are_counted_and_refused():
    from pylda_amd import _capi
    K = 4
    good = np.random.default_rng(1).gamma(1.0, size=(6, K))
    ctx = _capi.Context(K, V)

    def refused(call, rows, t, count, *more):
        with pytest.raises(_capi.PyldaError) as e:
            call(rows, *more) if more else call(rows, t)
        assert e.value.status == -1 and ("%d of %d rows" % (count, len(rows))) in str(e.value), str(e.value)

    try:
        zero, negative, infinite, nan = good.copy(), good.copy(), good.copy(), good.copy()
        zero[2] = 0.0
        negative[1, 3] = -1e-9
        negative[4, 0] = -2.0
        infinite[5, 1] = np.inf
        nan[0, 0] = np.nan
        ctx.similarity_set_base(good, 1)
        want = spec.nearest(good, 1, good, 1, 3)
        for t in (1, 2):
            refused(ctx.similarity_set_base, zero, t, 1)
            refused(ctx.similarity_set_base, negative, t, 2)
            refused(ctx.similarity_set_base, infinite, t, 1)
            refused(ctx.similarity_set_base, nan, t, 1)
            refused(ctx.similar_documents, negative, t, 2, 3, t)
            refused(ctx.similar_documents, zero, t, 1, 3, t)
        refused(ctx.similarity_set_base, infinite, 0, 1)
        refused(ctx.similarity_set_base, nan, 0, 1)
        refused(ctx.similar_documents, infinite, 0, 1, 3, 0)
        # a refused base leaves the one before it in place; transform 0 takes zero rows and negative entries
        _assert_equal(ctx.similar_documents(good, 3, 1), want)
        ctx.similarity_set_base(negative, 0)
        _assert_equal(ctx.similar_documents(zero, 3, 0), spec.nearest(negative, 0, zero, 0, 3))
    finally:
        ctx.close()


def test_status_codes():
    """Argument checks, all made before anything is launched; the next valid call is still right."""
    from pylda_amd import _capi
    K, D, Q, N = 3, 9, 4, 2
    rng = np.random.default_rng(9)
    base, queries = rng.standard_normal((D, K)), rng.standard_normal((Q, K))
    want = spec.nearest(base, 0, queries, 0, N)
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    ctx = _capi.Context(K, V)
    try:
        def status(call, *args, **kwargs):
            with pytest.raises(_capi.PyldaError) as e:
                call(*args, **kwargs)
            assert len(str(e.value)) > len("pylda_hip error -1: "), "no message"
            return e.value.status

        def valid():
            _assert_equal(ctx.similar_documents(queries, N, 0), want)
        assert status(ctx.similar_documents, queries, N, 0) == -4                     # no base yet
        assert status(ctx.similarity_set_base, np.zeros((0, K)), 0) == -1             # D = 0
        assert status(ctx.similarity_set_base, base, 3) == -1
        assert status(ctx.similar_documents, queries, N, 0) == -4                     # (the refused calls set none)
        ctx.similarity_set_base(base, 0)
        valid()
        for bad_n in (0, 65, -1):
            assert status(ctx.similar_documents, queries, bad_n, 0) == -1
            valid()
        assert status(ctx.similar_documents, np.zeros((0, K)), N, 0) == -1            # Q = 0
        for bad_t in (3, -1):
            assert status(ctx.similar_documents, queries, N, bad_t) == -1
        valid()
        for bad_self in (D, -2):
            selfs = np.array([0, -1, bad_self, 1], dtype=np.int32)
            assert status(ctx.similar_documents, queries, N, 0, selfs) == -1
            valid()
        ids, scores = np.zeros((Q, N), np.int32), np.zeros((Q, N))
        pointers = (queries.ctypes.data_as(f64p), ids.ctypes.data_as(i32p), scores.ctypes.data_as(f64p))
        for missing in range(3):
            rows_p, ids_p, scores_p = [None if i == missing else p for i, p in enumerate(pointers)]
            assert ctx._lib.pylda_similar_documents(ctx._h, Q, rows_p, 0, N, None, ids_p, scores_p) == -1
            assert b"NULL" in ctx._lib.pylda_last_error(ctx._h)
            valid()
        assert ctx._lib.pylda_similarity_set_base(ctx._h, D, None, 0) == -1 and b"NULL" in ctx._lib.pylda_last_error(ctx._h)
        valid()
        # a later base replaces the first
        other = rng.standard_normal((D + 200, K))
        ctx.similarity_set_base(other, 0)
        _assert_equal(ctx.similar_documents(queries, N, 0), spec.nearest(other, 0, queries, 0, N))
    finally:
        ctx.close()


def test_one_hot_queries_read_theta():
    from pylda_amd import _capi
    rng = np.random.default_rng(11)
    K, N = 10, 64
    distinct = rng.gamma(0.4, size=(6, K)) + 1e-6
    gamma = np.concatenate([distinct[rng.integers(0, 6, size=250)], rng.gamma(0.4, size=(50, K)) + 1e-6])   # repeated rows: ties
    theta = spec.transform(gamma, 1)
    ctx = _capi.Context(K, V)
    try:
        ctx.similarity_set_base(gamma, 1)
        ids, scores = ctx.similar_documents(np.eye(K), N, 0)
        for k in range(K):
            order = np.lexsort((np.arange(len(theta)), -theta[:, k]))[:N]
            assert np.array_equal(ids[k], order), k
            assert np.array_equal(_bits(scores[k]), _bits(theta[order, k])), k
    finally:
        ctx.close()


def test_kernel_time_reports_the_passes():
    from pylda_amd import _capi
    rng = np.random.default_rng(2)
    base, queries = rng.gamma(1.0, size=(500, 12)), rng.gamma(1.0, size=(70, 12))
    ctx = _capi.Context(12, V)
    try:
        ctx.set_profiling(True)
        ctx.kernel_time()
        ctx.similarity_set_base(base, 2)
        ctx.similar_documents(queries, 5, 2)
        documents_ms, statistics_ms = ctx.kernel_time()[:2]
        assert documents_ms > 0 and statistics_ms > 0
    finally:
        ctx.close()


# ---- the engines ----
def _documents(words, ptr, ids, cts, docs):
    return [" ".join(" ".join([words[t]] * int(c)) for t, c in zip(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]])) for d in docs]


def _assert_result(result, base, queries, top, metric, self_ids, what):
    t = {"hellinger": 2, "dot": 1}[metric]
    want = spec.nearest(base, t, queries, t, top, self_ids)
    _assert_equal((result.ids, result.affinity), want, what)
    assert result.metric == metric and result.documents == len(base), what
    if metric == "hellinger":
        assert np.array_equal(result.distance, spec.hellinger(want[1], want[0])), what
    else:
        assert result.distance is None, what


def _same_result(a, b):
    return np.array_equal(a.ids, b.ids) and np.array_equal(_bits(a.affinity), _bits(b.affinity)) and np.array_equal(a.distance, b.distance)


def _assert_top_documents(listed, base, top):
    ids, values = spec.nearest(base, 1, np.eye(base.shape[1]), 0, top)
    assert [[d for d, _ in topic] for topic in listed] == ids.tolist()
    assert [[x for _, x in topic] for topic in listed] == values.tolist()


def _train(m, ap_train, ap_test):
    words = [str(w) for w in ap_train["words"]]
    m._verbose = False
    np.random.seed(0)
    m._initialize(_documents(words, ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300)), words, 10, 0.1,
                  1.0 / len(words))
    m.learning()
    m.learning()
    return _documents(words, ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"], range(40))


def test_variational_bayes(ap_train, ap_test):
    from pylda_amd.variational_bayes import VariationalBayes
    m = VariationalBayes()
    test_docs = _train(m, ap_train, ap_test)
    gamma, eta = np.array(m._gamma), np.array(m._eta)
    own = m.similar_documents()
    _assert_result(own, gamma, gamma, 10, "hellinger", np.arange(300), "training documents")
    assert not np.any(own.ids == np.arange(300)[:, None]) and np.all(own.ids >= 0)
    assert np.all(np.diff(own.distance, axis=1) >= 0)                           # nearest first
    other = m.similar_documents(test_docs, top=7)
    assert np.array_equal(other.query_rows, m.inference(test_docs)[1])
    _assert_result(other, gamma, other.query_rows, 7, "hellinger", None, "test documents")
    _assert_result(m.similar_documents(other.query_rows[:3], top=4, metric="dot"), gamma, other.query_rows[:3], 4, "dot", None, "rows")
    _assert_top_documents(m.top_documents(5), gamma, 5)
    assert np.array_equal(np.array(m._gamma), gamma) and np.array_equal(np.array(m._eta), eta)      # read, never written
    restored = pickle.loads(pickle.dumps(m))
    restored._verbose = False
    assert _same_result(restored.similar_documents(), own) and _same_result(restored.similar_documents(test_docs, top=7), other)
    assert restored.top_documents(5) == m.top_documents(5)


def test_hybrid_and_online(ap_train, ap_test):
    from pylda_amd.hybrid import Hybrid
    from pylda_amd.online_vb import OnlineVariationalBayes
    for cls, args, kwargs in ((Hybrid, (), {"seed": 5}), (OnlineVariationalBayes, (4,), {})):
        m = cls(*args, **kwargs)
        test_docs = _train(m, ap_train, ap_test)
        gamma = np.array(m._gamma)
        result = m.similar_documents(test_docs, top=5)
        assert result.query_rows.shape == (40, 10)
        _assert_result(result, gamma, result.query_rows, 5, "hellinger", None, cls.__name__)
        _assert_top_documents(m.top_documents(3), gamma, 3)


def test_monte_carlo(ap_train, ap_test):
    from pylda_amd.monte_carlo import MonteCarlo
    m = MonteCarlo(hyper_parameter_optimize_interval=1000, seed=21, blocks=16)
    test_docs = _train(m, ap_train, ap_test)
    before = m._counts(True, True)
    rows = np.array(m._n_dk) + m._alpha_alpha[np.newaxis, :]
    own = m.similar_documents()
    _assert_result(own, rows, rows, 10, "hellinger", np.arange(300), "training documents")
    frozen = pickle.dumps(m)                                                    # (with the number of the next fold-in stream)
    other = m.similar_documents(test_docs, top=7, number_of_samples=8, burn_in_samples=4)
    assert other.query_rows.shape == (40, 10)
    _assert_result(other, rows, other.query_rows, 7, "hellinger", None, "test documents")
    _assert_top_documents(m.top_documents(5), rows, 5)
    assert all(np.array_equal(x, y) for x, y in zip(m._counts(True, True), before))      # the state is read, never written
    restored = pickle.loads(frozen)
    assert _same_result(restored.similar_documents(), own)
    assert _same_result(restored.similar_documents(test_docs, top=7, number_of_samples=8, burn_in_samples=4), other)
    assert restored.top_documents(5) == m.top_documents(5)
    assert restored._train_corpus is None


def test_launch_test_with_the_flag(ap_train, tmp_path, capsys):
    from pylda_amd import cli
    words = [str(w) for w in ap_train["words"]]
    ptr, ids, cts = ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"]
    source = tmp_path / "in" / "ap120"
    source.mkdir(parents=True)
    heldout = _documents(words, ptr, ids, cts, range(300, 330))
    (source / "train.dat").write_text("\n".join(_documents(words, ptr, ids, cts, range(120))) + "\n")
    (source / "test.dat").write_text("\n".join(heldout + ["not-a-word"]) + "\n")
    (source / "voc.dat").write_text("\n".join(words) + "\n")
    assert cli.train_main(["--input_directory=%s" % source, "--number_of_topics=5", "--training_iterations=2", "--snapshot_interval=2",
                           "--output_directory=%s" % (tmp_path / "vb")]) == 0
    run = tmp_path / "vb" / "ap120" / os.listdir(tmp_path / "vb" / "ap120")[0]
    trained = sorted(os.listdir(run))
    capsys.readouterr()
    # without the flag: the files and the output of today
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % run]) == 0
    plain = capsys.readouterr().out
    assert "similar" not in plain and sorted(os.listdir(run)) == sorted(trained + ["test-2"])
    gamma_file = (run / "test-2").read_bytes()
    # with it: the line, similar-2, and the rest as before
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % run, "--similar_documents=3"]) == 0
    out = capsys.readouterr().out
    assert sorted(os.listdir(run)) == sorted(trained + ["test-2", "similar-2"]) and (run / "test-2").read_bytes() == gamma_file
    lines = [l for l in out.splitlines() if l.startswith("similar documents of snapshot")]
    assert len(lines) == 1 and [l for l in out.splitlines() if not l.startswith("similar documents")] == plain.splitlines()
    with open(run / "model-2", "rb") as stream:
        engine = pickle.load(stream)
    test_gamma = np.loadtxt(run / "test-2")
    assert test_gamma.shape == (30, 5)
    want_ids, want_scores = spec.nearest(np.array(engine._gamma), 2, test_gamma, 2, 3)
    want_distance = spec.hellinger(want_scores, want_ids)
    rows = (run / "similar-2").read_text().splitlines()
    assert len(rows) == 30
    for d, row in enumerate(rows):
        fields = [field.split(":") for field in row.split("\t")]
        assert [int(i) for i, _ in fields] == want_ids[d].tolist() and [float(x) for _, x in fields] == want_distance[d].tolist()
    assert lines[0].endswith("mean nearest Hellinger distance %g" % np.mean(want_distance[:, 0])) and "120 training documents" in lines[0]
    # a snapshot without the rows of its training documents
    engine._gamma_host, engine._gamma_init_pending, engine._gamma_host_stale = None, False, False
    with open(run / "model-2", "wb") as stream:
        pickle.dump(engine, stream)
    os.remove(run / "similar-2")
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % run, "--similar_documents=3"]) == 2
    captured = capsys.readouterr()
    assert "holds no rows of its training documents" in captured.err and not (run / "similar-2").exists()

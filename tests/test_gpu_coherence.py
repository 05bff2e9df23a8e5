"""Topic coherence on the GPU (pylda_top_words / pylda_codocument_counts, coherence_kernels.h) against its numpy restatement
(tests/coherence_restatement.py), and the engines' topic_coherence() / top_words() and launch_test --topic_coherence built
on them.  Ids, values and counts are exact: every comparison of them is array_equal."""
import ctypes
import os
import pickle

import numpy as np
import pytest

import coherence_restatement as spec

pytestmark = pytest.mark.gpu

EDGE_IDS = (0, 63, 64, 255, 256, 257)       # lane, wavefront and stride edges of the selection kernel, and V - 1


def _tables(K, V):
    """name -> (K, V) table: continuous; integer-valued with heavy ties; constant rows; the best entries at the edges."""
    rng = np.random.default_rng(7 * K + V)
    edges = rng.random((K, V))
    at = [v for v in EDGE_IDS if v < V - 1] + [V - 1]
    for k in range(K):
        edges[k, at] = 10.0 + np.roll(np.arange(len(at)), k) * (1.0 if k % 3 else 0.0)     # (every third row: all of them tie)
    return {"continuous": rng.random((K, V)) - 0.5,
            "ties": rng.integers(0, 3, size=(K, V)).astype(np.float64) + 0.25,
            "constant": np.full((K, V), 1.5),
            "edges": edges}


@pytest.mark.parametrize("K,V,M", [(1, 5, 5), (2, 64, 64), (3, 257, 64), (10, 500, 1), (10, 500, 10), (129, 5000, 20), (1024, 300, 64)])
def test_selection_equals_the_restatement(K, V, M):
    from pylda_amd import _capi
    ctx = _capi.Context(K, V)
    try:
        for name, table in _tables(K, V).items():
            want_ids, want_values = spec.top_words(table, M)
            ids, values = ctx.top_words(M, table=table)
            assert ids.dtype == np.int32 and values.dtype == np.float64 and ids.shape == values.shape == (K, M)
            assert np.array_equal(ids, want_ids), (name, int(np.argmax(np.any(ids != want_ids, axis=1))))
            assert np.array_equal(values.view(np.int64), want_values.view(np.int64)), name      # the table's own bits
            if name == "constant":
                assert np.array_equal(ids, np.tile(np.arange(M, dtype=np.int32), (K, 1)))
            again = ctx.top_words(M, table=table)
            assert np.array_equal(again[0], ids) and np.array_equal(again[1].view(np.int64), values.view(np.int64)), name
            # the device eta ranked in place
            ctx.set_eta(table)
            from_eta = ctx.top_words(M)
            assert np.array_equal(from_eta[0], ids) and np.array_equal(from_eta[1].view(np.int64), values.view(np.int64)), name
    finally:
        ctx.close()


def _corpus(rng, V, D, top_ids):
    """CSR over V words: empty documents first and last (D >= 3), one document that holds every top word but `absent`, a
    term with count 300, and `absent` - a top word - in no document."""
    tops = np.unique(top_ids)
    absent = int(tops[len(tops) // 2])
    allowed = np.setdiff1d(np.arange(V), [absent])
    every = np.setdiff1d(tops, [absent])
    documents = []
    for d in range(D):
        if D >= 3 and d in (0, D - 1):
            ids = np.zeros(0, dtype=np.int64)
        elif d == (1 if D >= 3 else 0):
            ids = every
        else:
            n = int(rng.integers(0, min(len(allowed), 30) + 1))
            # top words often, so that pairs do co-occur
            ids = np.unique(np.concatenate([rng.choice(allowed, size=n, replace=False),
                                            rng.choice(every, size=min(len(every), 3), replace=False) if len(every) else every]))
        documents.append(ids)
    doc_ptr = np.concatenate([[0], np.cumsum([len(i) for i in documents])]).astype(np.int64)
    term_id = np.concatenate(documents).astype(np.int32)
    term_ct = rng.integers(1, 4, size=len(term_id)).astype(np.int32)
    if len(term_ct):
        term_ct[len(term_ct) // 2] = 300
    return (doc_ptr, term_id, term_ct), absent


def _assert_counts(ctx, csr, ids, what, want=None):
    corpus = ctx.corpus(*csr)
    try:
        doc_freq, co = ctx.codocument_counts(corpus, ids)
        again = ctx.codocument_counts(corpus, ids)
    finally:
        corpus.close()
    want_doc_freq, want_co = want or spec.counts(csr[0], csr[1], ids)
    assert doc_freq.dtype == co.dtype == np.int64
    assert np.array_equal(doc_freq, want_doc_freq), what
    assert np.array_equal(co, want_co), what
    assert np.array_equal(again[0], doc_freq) and np.array_equal(again[1], co), what
    assert np.array_equal(np.diagonal(co, axis1=1, axis2=2), doc_freq), what
    assert np.array_equal(co, np.transpose(co, (0, 2, 1))), what
    return doc_freq, co


@pytest.mark.parametrize("D", [1, 63, 64, 65, 300, 4097])
def test_counts_equal_the_restatement(D):
    from pylda_amd import _capi
    K, V, M = 10, 500, 10
    rng = np.random.default_rng(D)
    ctx = _capi.Context(K, V)
    try:
        selected = ctx.top_words(M, table=rng.random((K, V)))[0]
        shared = (np.arange(M)[None, :] * 3 + (np.arange(K)[:, None] % 2)).astype(np.int32)      # two lists, five topics each
        repeats = rng.integers(0, V, size=(K, M)).astype(np.int32)
        repeats[:, 1::2] = repeats[:, ::2]                                                      # every word twice in its topic
        repeats[3] = 7
        for name, ids in (("selected", selected), ("shared", shared), ("repeats", repeats)):
            csr, absent = _corpus(rng, V, D, ids)
            doc_freq, co = _assert_counts(ctx, csr, ids, (name, D))
            assert np.all(doc_freq[ids == absent] == 0) and np.any(ids == absent)
            assert doc_freq.max() <= D and (D < 3 or doc_freq.max() >= 1)
    finally:
        ctx.close()


@pytest.mark.parametrize("K,V,M,D", [(1, 5, 1, 65), (129, 5000, 20, 300), (1024, 300, 64, 65)])
def test_counts_whatever_the_chunk(K, V, M, D):
    """(1024, 300, 64): 65536 top ids over 300 words - the slots are capped by the vocabulary."""
    from pylda_amd import _capi
    rng = np.random.default_rng(K + D)
    ctx = _capi.Context(K, V)
    try:
        ids = ctx.top_words(M, table=rng.random((K, V)))[0]
        csr, _ = _corpus(rng, V, D, ids)
        results, want = [], spec.counts(csr[0], csr[1], ids)
        for chunk in (64, 128, 0):
            ctx.set_option("coherence_chunk_docs", chunk)
            results.append(_assert_counts(ctx, csr, ids, (K, V, M, D, chunk), want))
        for doc_freq, co in results[1:]:
            assert np.array_equal(doc_freq, results[0][0]) and np.array_equal(co, results[0][1])
    finally:
        ctx.close()


def test_error_codes():
    """Argument checks, all made before anything is launched; the next valid call still succeeds."""
    from pylda_amd import _capi
    K, V, M = 3, 5, 2
    table = np.random.default_rng(3).random((K, V))
    csr = (np.array([0, 2, 3], dtype=np.int64), np.array([1, 4, 0], dtype=np.int32), np.array([1, 2, 1], dtype=np.int32))
    nothing = (np.array([0], dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    good = np.array([[0, 1], [4, 4], [2, 0]], dtype=np.int32)
    ctx, other = _capi.Context(K, V), _capi.Context(K, V)
    i32p, i64p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    try:
        corpus, empty, foreign = ctx.corpus(*csr), ctx.corpus(*nothing), other.corpus(*csr)

        def status(call, *args, **kwargs):
            with pytest.raises(_capi.PyldaError) as e:
                call(*args, **kwargs)
            assert len(str(e.value)) > len("pylda_hip error -1: "), "no message"
            return e.value.status

        def valid():
            ids, values = ctx.top_words(M, table=table)
            assert np.array_equal(ids, spec.top_words(table, M)[0])
            doc_freq, co = ctx.codocument_counts(corpus, good)
            assert np.array_equal(co, spec.counts(csr[0], csr[1], good)[1]) and np.array_equal(doc_freq, [[1, 1], [1, 1], [0, 1]])
        assert status(ctx.top_words, M) == -4                                  # NULL table, and eta was never set
        valid()
        for bad in (0, -1, 65, V + 1):
            assert status(ctx.top_words, bad, table=table) == -1
            valid()
        ids_out, values_out = np.zeros((K, M), np.int32), np.zeros((K, M))
        for ids_p, values_p in ((None, values_out.ctypes.data_as(f64p)), (ids_out.ctypes.data_as(i32p), None)):
            assert ctx._lib.pylda_top_words(ctx._h, table.ctypes.data_as(f64p), M, ids_p, values_p) == -1
            assert b"NULL" in ctx._lib.pylda_last_error(ctx._h)
            valid()
        assert status(ctx.codocument_counts, corpus, np.zeros((K, 0), np.int32)) == -1       # M < 1
        assert status(ctx.codocument_counts, corpus, np.zeros((K, 65), np.int32)) == -1      # M > 64
        valid()
        for bad in (-1, V):
            wrong = good.copy()
            wrong[2, 1] = bad
            assert status(ctx.codocument_counts, corpus, wrong) == -1
            valid()
        assert status(ctx.codocument_counts, empty, good) == -1                # D = 0
        assert status(ctx.codocument_counts, foreign, good) == -1
        valid()
        doc_freq, co = np.zeros((K, M), np.int64), np.zeros((K, M, M), np.int64)
        pointers = (good.ctypes.data_as(i32p), doc_freq.ctypes.data_as(i64p), co.ctypes.data_as(i64p))
        for missing in range(3):
            args = [None if i == missing else p for i, p in enumerate(pointers)]
            assert ctx._lib.pylda_codocument_counts(ctx._h, corpus._h, M, *args) == -1
            assert b"NULL" in ctx._lib.pylda_last_error(ctx._h)
        assert status(ctx.set_option, "coherence_chunk_docs", 65) == -1
        assert status(ctx.set_option, "coherence_chunk_docs", -64) == -1
        valid()
        # a corpus that holds a Gibbs state is read like any other
        ctx.gibbs_init(corpus, 1)
        valid()
        for c in (corpus, empty, foreign):
            c.close()
    finally:
        ctx.close()
        other.close()


def _documents(words, ptr, ids, cts, docs):
    return [" ".join(" ".join([words[t]] * int(c)) for t, c in zip(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]])) for d in docs]


def _assert_result(result, want, what):
    for name in ("top_ids", "doc_freq", "co_doc_freq", "undefined_pairs"):
        assert np.array_equal(getattr(result, name), want[name]), (what, name)
    assert np.array_equal(result.top_values.view(np.int64), want["top_values"].view(np.int64)), what
    assert result.documents == want["documents"] and result.top_words_count == want["top_words_count"], what
    np.testing.assert_allclose(result.umass, want["umass"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(result.npmi, want["npmi"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose([result.umass_mean, result.npmi_mean], [want["umass_mean"], want["npmi_mean"]], rtol=1e-12, atol=1e-13)


def _same_result(a, b):
    return all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ("top_ids", "top_values", "doc_freq", "co_doc_freq", "umass", "npmi",
                                                                      "undefined_pairs"))


def _vb_family(cls, ap_train, ap_test, *args, **kwargs):
    words = [str(w) for w in ap_train["words"]]
    m = cls(*args, **kwargs)
    m._verbose = False
    np.random.seed(0)
    m._initialize(_documents(words, ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300)), words, 10, 0.1,
                  1.0 / len(words))
    m.learning()
    m.learning()
    test_docs = _documents(words, ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"], range(40))
    return m, words, test_docs


def test_variational_bayes(ap_train, ap_test):
    from pylda_amd.variational_bayes import VariationalBayes
    m, words, test_docs = _vb_family(VariationalBayes, ap_train, ap_test)
    eta = np.array(m._eta)
    own = m.topic_coherence()
    _assert_result(own, spec.coherence(eta, 10, m._train_csr[0], m._train_csr[1]), "training documents")
    assert own.documents == 300 and np.all(own.doc_freq >= 1) and np.all(own.undefined_pairs == 0)
    test_csr = m.parse_to_csr(test_docs)
    other = m.topic_coherence(test_docs + ["not-a-word"], top_words=7)
    _assert_result(other, spec.coherence(eta, 7, test_csr[0], test_csr[1]), "test documents")
    assert other.documents == 40
    listed = m.top_words(7)
    assert [[w for w, _ in topic] for topic in listed] == [[words[v] for v in row] for row in other.top_ids]
    assert [[x for _, x in topic] for topic in listed] == other.top_values.tolist()
    assert np.array_equal(np.array(m._eta), eta)                               # the model is read, never written
    restored = pickle.loads(pickle.dumps(m))
    assert restored._train_corpus is None
    assert _same_result(restored.topic_coherence(), own) and _same_result(restored.topic_coherence(test_docs, 7), other)
    assert restored._train_corpus is None                                      # the corpus opened for the call is closed again


def test_hybrid_and_online(ap_train, ap_test):
    from pylda_amd.hybrid import Hybrid
    from pylda_amd.online_vb import OnlineVariationalBayes
    for cls, args, kwargs in ((Hybrid, (), {"seed": 5}), (OnlineVariationalBayes, (4,), {})):
        m, words, test_docs = _vb_family(cls, ap_train, ap_test, *args, **kwargs)
        eta = np.array(m._eta)
        _assert_result(m.topic_coherence(top_words=5), spec.coherence(eta, 5, m._train_csr[0], m._train_csr[1]), cls.__name__)
        test_csr = m.parse_to_csr(test_docs)
        _assert_result(m.topic_coherence(test_docs, 5), spec.coherence(eta, 5, test_csr[0], test_csr[1]), cls.__name__)
        assert len(m.top_words(3)) == 10 and all(len(topic) == 3 for topic in m.top_words(3))


def test_monte_carlo(ap_train, ap_test):
    from pylda_amd.hybrid import _grouped_csr
    from pylda_amd.monte_carlo import MonteCarlo
    words = [str(w) for w in ap_train["words"]]
    m = MonteCarlo(hyper_parameter_optimize_interval=1000, seed=21, blocks=16)
    m._verbose = False
    m._initialize(_documents(words, ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300)), words, 10, 0.1,
                  1.0 / len(words))
    m.learning()
    m.learning()
    before = m._counts(True, True)
    table = before[0].astype(np.float64) + m._alpha_beta[np.newaxis, :]
    own = m.topic_coherence()
    _assert_result(own, spec.coherence(table, 10, m._train_csr[0], m._train_csr[1]), "training documents")
    test_docs = _documents(words, ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"], range(40))
    test_csr = _grouped_csr(m.parse_data(test_docs))
    other = m.topic_coherence(test_docs, top_words=6)
    _assert_result(other, spec.coherence(table, 6, test_csr[0], test_csr[1]), "test documents")
    assert [[w for w, _ in topic] for topic in m.top_words(6)] == [[words[v] for v in row] for row in other.top_ids]
    assert all(np.array_equal(x, y) for x, y in zip(m._counts(True, True), before))      # the state is read, never written
    restored = pickle.loads(pickle.dumps(m))
    assert _same_result(restored.topic_coherence(), own) and _same_result(restored.topic_coherence(test_docs, 6), other)
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
    K = 5
    assert cli.train_main(["--input_directory=%s" % source, "--number_of_topics=%d" % K, "--training_iterations=2", "--snapshot_interval=2",
                           "--output_directory=%s" % (tmp_path / "vb")]) == 0
    run = tmp_path / "vb" / "ap120" / os.listdir(tmp_path / "vb" / "ap120")[0]
    trained = sorted(os.listdir(run))
    capsys.readouterr()
    # without the flag: the files and the output of today
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % run]) == 0
    plain = capsys.readouterr().out
    assert "coherence" not in plain and sorted(os.listdir(run)) == sorted(trained + ["test-2"])
    gamma = (run / "test-2").read_bytes()
    # with it: the line, coherence-2, and the rest as before
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % run, "--topic_coherence=5"]) == 0
    out = capsys.readouterr().out
    assert sorted(os.listdir(run)) == sorted(trained + ["test-2", "coherence-2"]) and (run / "test-2").read_bytes() == gamma
    lines = [l for l in out.splitlines() if l.startswith("topic coherence of snapshot")]
    # (the rest of the output: what it was, and the line of the engine's parser once more - the test documents are parsed twice)
    rest = [l for l in out.splitlines() if not l.startswith("topic coherence")]
    rest.remove("successfully parse 30 documents...")
    assert len(lines) == 1 and rest == plain.splitlines()
    assert out.index("topic coherence of snapshot") < out.index("held-out likelihood of snapshot")
    with open(run / "model-2", "rb") as stream:
        engine = pickle.load(stream)
    engine._verbose = False
    want = engine.topic_coherence(heldout, 5)
    assert lines[0] == ("topic coherence of snapshot %s over its top 5 words on 30 documents: UMass %g, NPMI %g (means over %d topics, "
                        "%d undefined pairs)" % (os.path.abspath(run / "model-2"), want.umass_mean, want.npmi_mean, K,
                                                 int(want.undefined_pairs.sum())))
    rows = (run / "coherence-2").read_text().splitlines()
    assert len(rows) == K
    for k, row in enumerate(rows):
        fields = row.split("\t")
        assert fields[0] == str(k) and fields[1] == "%g" % want.umass[k] and fields[2] == "%g" % want.npmi[k]
        assert fields[3:] == [words[v] for v in want.top_ids[k]]

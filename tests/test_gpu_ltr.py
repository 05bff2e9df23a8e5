"""The left-to-right held-out likelihood on the GPU (pylda_left_to_right, left_to_right.h) against its numpy restatement
(tests/ltr_restatement.py) draw for draw, the enumerated p(w) of the K = 3 fixture, and the engines' left_to_right() and
launch_test --left_to_right built on it.

The topics and the predictive probabilities are held to array_equal: the restatement mirrors every sum's order and the
chains hold no transcendental.  The bar per document is derived, not tuned (ltr_restatement.bar):
    |delta| <= N_d (K + R + 16) 2^-53 + 4 * 2^-53 * sum_n |log m_n| + N_d 2^-53 |ll_d|
Largest |delta| / bar measured on an MI355X, over all cases of test_kernel_equals_the_restatement: see DESIGN.md section 19."""
import math
import os
import pickle

import numpy as np
import pytest

import foldin_fixture as fx
import foldin_restatement as foldin_spec
import ltr_fixture as lf
import ltr_restatement as spec
from conftest import csr_slice

pytestmark = pytest.mark.gpu

V = 500
SEED, STREAM = 0x5EED0123456789AB, (3 << 30) + 512


def _stack(documents):
    """CSR of documents given as (term ids, counts)."""
    ptr = np.concatenate([[0], np.cumsum([len(i) for i, _ in documents])]).astype(np.int64)
    return (ptr, np.concatenate([np.asarray(i, dtype=np.int64) for i, _ in documents]).astype(np.int32),
            np.concatenate([np.asarray(c, dtype=np.int64) for _, c in documents]).astype(np.int32))


_cases = {}


def _case(K, D, R, resample):
    """(csr, (n_kv, n_k, beta), alpha, want = the restatement's result); computed once, shared, never written."""
    key = (K, D, R, resample)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(1000 * K + 10 * D + R + resample)

    def doc(n, last_word=False):
        """n tokens: random words grouped, a term's copies back to back"""
        words = rng.integers(V, size=n)
        if last_word and n:
            words[rng.integers(n)] = V - 1
        ids, cts = np.unique(words, return_counts=True)
        order = rng.permutation(len(ids))                 # (CSR terms need not be sorted: the order is the token order)
        return ids[order], cts[order]
    if D == 1:
        documents = [doc(63)]
    elif D == 5:
        # with resampling only K = 10 pays for the 300-fold term (45150 steps a particle); without, the 3000-term document
        # (3000 CSR terms over 500 words: the words repeat, each entry a run of one or two tokens)
        long_one = (rng.integers(V, size=3000), rng.integers(1, 3, size=3000)) if not resample else \
            ([V - 1], [300]) if K == 10 else doc(64)
        documents = [doc(0), doc(1), ([7], [2]), doc(65, last_word=True), long_one]
    else:
        edges = [doc(0), doc(1), doc(2), doc(63), doc(64), doc(65), ([V - 1], [1]), doc(64, last_word=True)]
        if not resample:
            edges.append(([17], [300]))
        documents = [doc(int(rng.integers(1, 41))) for _ in range(D - len(edges) - 1)]
        for at, e in zip((0, 3, 5, 64, 65, 66, 130, 131, 190), edges):
            documents.insert(at, e)
        documents.append(doc(0))                          # an empty document at the end of the grid
    assert len(documents) == D
    csr = _stack(documents)
    n_kv = (rng.gamma(0.3, 20.0, (K, V)) * (rng.random((K, V)) < 0.3)).astype(np.int32)
    n_k = n_kv.sum(axis=1).astype(np.int32)
    beta = rng.gamma(2.0, 0.02, V) + 1e-3
    alpha = rng.gamma(0.5, 1.0, K) + 0.01
    P = foldin_spec.predictive_table(n_kv, n_k, beta, float(np.sum(beta)))
    want = spec.left_to_right(*csr, P, alpha, R, resample, SEED, STREAM, first_document=3)
    _cases[key] = (csr, (n_kv, n_k, beta), alpha, want)
    return _cases[key]


def _run(ctx, csr, alpha, R, resample, first_document=3, step_budget=0, state=True, stream=STREAM):
    """One pylda_left_to_right through the binding: (total, tokens, per-document values, z, p)."""
    heldout = ctx.corpus(*csr)
    try:
        total, tokens = ctx.left_to_right(heldout, alpha, R, resample, SEED, stream, first_document, step_budget)
        doc_ll, doc_wll, iters = ctx.get_doc_values(heldout)
        assert np.all(doc_ll == 0.0) and np.all(iters == R)
        assert ctx.estep_results(heldout)[1] == total
        z, p = ctx.test_left_to_right_state(heldout, R) if state else (None, None)
    finally:
        heldout.close()
    return total, tokens, np.array(doc_wll), z, p


def _assert_equals_the_restatement(what, K, R, got, want):
    total, tokens, doc_wll, z, p = got
    assert tokens == want["tokens"], what
    if z is not None:
        assert np.array_equal(z, want["z"]), (what, int(np.sum(z != want["z"])))
        assert np.array_equal(p, want["p"]), what
        assert np.all(np.abs(p - want["p"]) <= (K + 8) * 2.0 ** -53 * want["p"]), what
    bar = spec.bar(K, R, want["doc_tok"], want["doc_ll"], want["abs_logs"])
    delta = np.abs(doc_wll - want["doc_ll"])
    ratio = float(np.max(delta[bar > 0] / bar[bar > 0])) if np.any(bar > 0) else 0.0
    print("%s: largest |delta| / bar %.3f over %d documents, %d tokens" % (what, ratio, len(bar), tokens))
    assert np.all(doc_wll[np.diff(want["doc_tok"]) == 0] == 0.0), what        # an empty document scores exactly 0
    assert np.all(delta <= bar), (what, ratio, int(np.argmax(delta - bar)))
    assert abs(total - want["log_likelihood"]) <= float(bar.sum()) + len(bar) * 2.0 ** -53 * abs(want["log_likelihood"]), what
    return ratio


CASES = [(1, 1, 1, 1), (10, 5, 2, 1), (10, 203, 7, 0), (64, 203, 2, 1), (65, 5, 20, 0), (128, 203, 1, 1), (129, 5, 7, 1),
         (256, 203, 2, 0), (257, 5, 2, 1), (512, 1, 20, 1), (513, 5, 1, 1), (1024, 203, 1, 0), (1024, 5, 2, 1)]


@pytest.mark.parametrize("K,D,R,resample", CASES)
def test_kernel_equals_the_restatement(K, D, R, resample):
    """A host-given table through pylda_foldin_set_model (its bits are the restatement's: add, add, divide) and a vector
    alpha.  K = 1 draws topic 0 throughout: the case checks the predictive probabilities alone."""
    from pylda_amd import _capi
    csr, (n_kv, n_k, beta), alpha, want = _case(K, D, R, resample)
    ctx = _capi.Context(K, V)
    try:
        ctx.foldin_set_model(beta, n_kv=n_kv, n_k=n_k)
        got = _run(ctx, csr, alpha, R, resample)
    finally:
        ctx.close()
    _assert_equals_the_restatement("K=%d D=%d R=%d resample=%d" % (K, D, R, resample), K, R, got, want)


def test_same_input_same_bits_whatever_the_corpora_the_launches_and_the_chunks():
    from pylda_amd import _capi
    K, D, R, resample = 64, 203, 2, 1
    (ptr, ids, cts), (n_kv, n_k, beta), alpha, want = _case(K, D, R, resample)
    n = np.diff(want["doc_tok"]).astype(np.float64)
    steps = float(np.sum(R * (n * (n - 1) / 2 + n)))
    ctx = _capi.Context(K, V)
    try:
        ctx.foldin_set_model(beta, n_kv=n_kv, n_k=n_k)
        first = _run(ctx, (ptr, ids, cts), alpha, R, resample)
        again = _run(ctx, (ptr, ids, cts), alpha, R, resample)
        cut_doc = 67                                      # not a multiple of a workgroup's four wavefronts
        cut = int(ptr[cut_doc])
        lo = _run(ctx, (ptr[:cut_doc + 1], ids[:cut], cts[:cut]), alpha, R, resample, first_document=3)
        hi = _run(ctx, (ptr[cut_doc:] - cut, ids[cut:], cts[cut:]), alpha, R, resample, first_document=3 + cut_doc)
        quarter = _run(ctx, (ptr, ids, cts), alpha, R, resample, step_budget=int(steps / 4))     # four launches at least
        single = _run(ctx, (ptr, ids, cts), alpha, R, resample, step_budget=1)                   # a launch per document
        ctx.set_option("ltr_chunk_tokens", 70)            # (the longest document has 65 tokens)
        heldout = ctx.corpus(ptr, ids, cts)
        chunked = ctx.left_to_right(heldout, alpha, R, resample, SEED, STREAM, 3, int(steps / 4))
        chunked_docs = np.array(ctx.get_doc_values(heldout)[1])
        with pytest.raises(_capi.PyldaError) as e:
            ctx.test_left_to_right_state(heldout, R)      # the buffers hold the last chunk only
        assert e.value.status == -4 and "chunks" in str(e.value)
        ctx.set_option("ltr_chunk_tokens", 64)
        with pytest.raises(_capi.PyldaError) as e:
            ctx.left_to_right(heldout, alpha, R, resample, SEED, STREAM, 3)
        assert e.value.status == -3 and "65 tokens" in str(e.value)
        heldout.close()
    finally:
        ctx.close()
    for other in (again, quarter, single):
        assert other[0] == first[0] and other[1] == first[1] and np.array_equal(other[2], first[2])
        assert np.array_equal(other[3], first[3]) and np.array_equal(other[4], first[4])
    assert np.array_equal(np.concatenate([lo[2], hi[2]]), first[2]) and lo[1] + hi[1] == first[1]
    assert chunked == (first[0], first[1]) and np.array_equal(chunked_docs, first[2])
    assert np.array_equal(first[3], want["z"])


@pytest.mark.parametrize("words,resample", [(lf.SEVEN, 0), (lf.TWO, 1)])
def test_unbiased_on_the_enumeration_fixture(words, resample):
    """D = 1600 copies of the document, R = 1, one launch: mean exp(ll_d) within 5 standard errors of the enumerated p(w),
    and the chains are the restatement's (tests/test_ltr_host.py holds those to the same bar and to its controls)."""
    from pylda_amd import _capi
    csr = lf.corpus(words, lf.REPLICAS)
    want = spec.left_to_right(*csr, fx.table(), fx.ALPHA, 1, resample, 20240607, 3 << 30)
    ctx = _capi.Context(3, 5)
    try:
        ctx.foldin_set_model(fx.BETA, n_kv=fx.N_KV.astype(np.int32), n_k=fx.N_KV.sum(axis=1).astype(np.int32))
        heldout = ctx.corpus(*csr)
        ctx.left_to_right(heldout, fx.ALPHA, 1, resample, 20240607, 3 << 30, 0, 1 << 40)
        doc_wll = np.array(ctx.get_doc_values(heldout)[1])
        z, _ = ctx.test_left_to_right_state(heldout, 1)
        heldout.close()
    finally:
        ctx.close()
    score = lf.z_score(np.exp(doc_wll), lf.exact_probability(words, fx.table(), fx.ALPHA))
    print("z", round(score, 2))
    assert abs(score) < 5.0
    assert np.array_equal(z, want["z"])


# ---------------------------------------------------------------- engines
def _documents(words, ptr, ids, cts, docs):
    return [" ".join(" ".join([words[t]] * int(c)) for t, c in zip(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]])) for d in docs]


def _vb_engine(cls, ap_train, *args, **kwargs):
    """An engine over the first 100 associated-press documents that holds the golden model (alpha, eta)."""
    words = [str(w) for w in ap_train["words"]]
    m = cls(*args, **kwargs)
    m._verbose = False
    np.random.seed(0)
    m._initialize(_documents(words, ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(100)), words, 10, 0.1,
                  1.0 / len(words))
    m._alpha_alpha = ap_train["alpha"].copy()
    m._eta = ap_train["eta"].copy()
    return m, words


def _table_of_eta(eta):
    """completion_set_model's table with the device's row sums: thread t of 256 adds v = t, t + 256, .. in turn, then the
    wavefronts pairwise by lane and the four of them in order; the division rounded once."""
    return (eta / np.array([foldin_spec.fixed_order_total(row) for row in eta])[:, np.newaxis]).T.copy()


def _assert_engine_result(what, got, want, R):
    ll, tokens, per_document = got
    assert tokens == want["tokens"] and per_document.shape == want["doc_ll"].shape, what
    bar = spec.bar(10, R, want["doc_tok"], want["doc_ll"], want["abs_logs"])
    delta = np.abs(per_document - want["doc_ll"])
    print("%s: %.6f per token (perplexity %.1f), largest |delta| / bar %.3f" % (what, ll / tokens, math.exp(-ll / tokens),
                                                                                 float(np.max(delta / bar))))
    assert np.all(delta <= bar), what
    assert abs(ll - want["log_likelihood"]) <= float(bar.sum()) + len(bar) * 2.0 ** -53 * abs(want["log_likelihood"]), what


def test_variational_engines(ap_train, ap_test):
    """VariationalBayes, OnlineVariationalBayes and Hybrid share the method: the table of eta, the engine's alpha, streams
    (3 << 30) + 256 n, the engine's sampler seed where it has one."""
    from pylda_amd.hybrid import Hybrid, _grouped_csr
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import LEFT_TO_RIGHT_STREAM_BASE, VariationalBayes
    R = 4
    m, words = _vb_engine(VariationalBayes, ap_train)
    test_docs = _documents(words, ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"], range(40))
    P = _table_of_eta(ap_train["eta"])
    plug_in_before = m.inference(test_docs)
    completion_before = m.document_completion(test_docs)
    first = m.left_to_right(test_docs + ["not-a-word"], R, False)                      # (call 0)
    csr = m.parse_to_csr(test_docs)
    _assert_engine_result("variational Bayes", first, spec.left_to_right(*csr, P, ap_train["alpha"], R, 0, 0, LEFT_TO_RIGHT_STREAM_BASE), R)
    second = m.left_to_right(test_docs, R, False)                                      # (call 1: other streams)
    assert m._left_to_right_calls == 2 and second[0] != first[0]
    _assert_engine_result("variational Bayes, call 1", second,
                          spec.left_to_right(*csr, P, ap_train["alpha"], R, 0, 0, LEFT_TO_RIGHT_STREAM_BASE + 256), R)
    default = m.left_to_right(test_docs[:8], R)                                         # resampling, the default
    assert np.isfinite(default[0]) and default[0] < 0 and default[2].shape == (8,)
    # inference() and document_completion() are what they were, and a pickled engine carries the call counter
    plug_in_after, completion_after = m.inference(test_docs), m.document_completion(test_docs)
    assert plug_in_after[0] == plug_in_before[0] and np.array_equal(plug_in_after[1], plug_in_before[1])
    assert completion_after[0] == completion_before[0] and np.array_equal(completion_after[2], completion_before[2])
    restored = pickle.loads(pickle.dumps(m))
    assert restored._left_to_right_calls == 3
    restored._left_to_right_calls = 0
    again = restored.left_to_right(test_docs, R, False)
    assert again[0] == first[0] and again[1] == first[1] and np.array_equal(again[2], first[2])
    online, _ = _vb_engine(OnlineVariationalBayes, ap_train, 4)
    got = online.left_to_right(test_docs, R, False)
    assert got[0] == first[0] and np.array_equal(got[2], first[2])
    # the hybrid engine parses to token lists and draws with its sampler seed; its held-out stream counter stays
    hybrid, _ = _vb_engine(Hybrid, ap_train, seed=5)
    hybrid_plug_in = hybrid.inference(test_docs)
    got = hybrid.left_to_right(test_docs, R, False)
    assert hybrid._heldout_calls == 1
    grouped = _grouped_csr(hybrid.parse_data(test_docs))
    _assert_engine_result("hybrid", got, spec.left_to_right(*grouped, P, ap_train["alpha"], R, 0, 5, LEFT_TO_RIGHT_STREAM_BASE), R)
    hybrid._heldout_calls = 0
    assert hybrid.inference(test_docs)[0] == hybrid_plug_in[0]


def test_monte_carlo_from_the_device_corpus_and_from_a_snapshot(ap_train, ap_test):
    from pylda_amd.hybrid import _grouped_csr
    from pylda_amd.monte_carlo import MonteCarlo
    from pylda_amd.variational_bayes import LEFT_TO_RIGHT_STREAM_BASE
    R = 4
    words = [str(w) for w in ap_train["words"]]
    m = MonteCarlo(hyper_parameter_optimize_interval=1000, seed=21, blocks=16)
    m._verbose = False
    m._initialize(_documents(words, ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300)), words, 10, 0.1,
                  1.0 / len(words))
    for _ in range(3):
        m.learning()
    test_docs = _documents(words, ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"], range(40))
    before = m._counts(True, True)
    blob = pickle.dumps(m)
    fold_in_before = m.fold_in(test_docs, 6, 3)                                        # (fold-in stream 0)
    completion_before = m.document_completion(test_docs, 6, 3)                         # (fold-in stream 1)
    got = m.left_to_right(test_docs + ["not-a-word"], R, False)
    assert m._fold_in_calls == 2 and m._left_to_right_calls == 1
    assert all(np.array_equal(x, y) for x, y in zip(m._counts(True, True), before))    # the training state is read, never written
    n_kv, n_k, _ = before
    P = foldin_spec.predictive_table(n_kv, n_k, m._alpha_beta, float(np.sum(m._alpha_beta)))
    csr = _grouped_csr(m.parse_data(test_docs))
    _assert_engine_result("collapsed Gibbs", got, spec.left_to_right(*csr, P, m._alpha_alpha, R, 0, 21, LEFT_TO_RIGHT_STREAM_BASE), R)
    # a restored snapshot scores from its host counts: the same bits; fold_in() and document_completion() keep theirs
    restored = pickle.loads(blob)
    restored._verbose = False
    same = restored.left_to_right(test_docs, R, False)
    assert restored._train_corpus is None
    assert same[0] == got[0] and same[1] == got[1] and np.array_equal(same[2], got[2])
    assert restored.fold_in(test_docs, 6, 3)[0] == fold_in_before[0]
    again = restored.document_completion(test_docs, 6, 3)
    assert again[0] == completion_before[0] and np.array_equal(again[2], completion_before[2])
    m._fold_in_calls = 0
    fold_in_after = m.fold_in(test_docs, 6, 3)
    assert fold_in_after[0] == fold_in_before[0] and np.array_equal(fold_in_after[1], fold_in_before[1])


# ---------------------------------------------------------------- errors and the command line
def test_error_codes():
    from pylda_amd import _capi
    csr = _stack([([1, 2], [1, 2]), ([3], [1])])
    K, W = 4, 6
    alpha = np.full(K, 0.5)
    ctx, other = _capi.Context(K, W), _capi.Context(K, W)
    try:
        heldout, trained, foreign = ctx.corpus(*csr), ctx.corpus(*csr), other.corpus(*csr)

        def status(*args, **kwargs):
            with pytest.raises(_capi.PyldaError) as e:
                ctx.left_to_right(*args, **kwargs)
            assert len(str(e.value)) > len("pylda_hip error -1: "), "no message"
            return e.value.status
        assert status(heldout, alpha, 2) == -4                          # no predictive table
        with pytest.raises(_capi.PyldaError) as e:
            ctx.test_left_to_right_state(heldout, 2)                    # no call yet
        assert e.value.status == -4
        ctx.foldin_set_model(np.full(W, 0.1), n_kv=np.ones((K, W), np.int32), n_k=np.full(K, W, np.int32))
        for particles in (0, -3, 257):
            assert status(heldout, alpha, particles) == -1
        assert status(heldout, alpha, 2, 2) == -1 and status(heldout, alpha, 2, -1) == -1      # resample
        assert status(heldout, alpha, 2, 1, 0, 2 ** 32 - 1) == -1       # stream + particles > 2^32
        assert status(heldout, alpha, 2, 1, 0, 0, -1) == -1             # first_document
        assert status(heldout, alpha, 2, 1, 0, 0, 0, -5) == -1          # step_budget
        assert status(foreign, alpha, 2) == -1
        total, tokens = ctx.left_to_right(heldout, alpha, 2, 1, 0, 2 ** 32 - 2)      # the last two streams
        assert tokens == 4 and abs(total - 4 * math.log(1.0 / W)) < 1e-12            # (rows constant over the topics)
        with pytest.raises(_capi.PyldaError) as e:
            ctx.test_left_to_right_state(heldout, 3)                    # another number of particles
        assert e.value.status == -4
        ctx.gibbs_init(trained, 1)
        assert status(trained, alpha, 2) == -4                          # a Gibbs training state
        # either model's table serves; with neither the call is refused again
        ctx.set_alpha(alpha)
        ctx.set_eta(np.ones((K, W)))
        ctx.completion_set_model()
        assert abs(ctx.left_to_right(heldout, alpha, 1, 0)[0] - 4 * math.log(1.0 / W)) < 1e-12
        for c in (heldout, trained, foreign):
            c.close()
    finally:
        ctx.close()
        other.close()
    wide = _capi.Context(1025, W)
    try:
        heldout = wide.corpus(*csr)
        with pytest.raises(_capi.PyldaError) as e:
            wide.left_to_right(heldout, np.ones(1025), 2)
        assert e.value.status == -1 and "1024" in str(e.value)
        heldout.close()
    finally:
        wide.close()


def _line(out):
    lines = [l for l in out.splitlines() if l.startswith("left-to-right likelihood of snapshot")]
    assert len(lines) == 1, out
    words = lines[0].split()
    ll, tokens, perplexity = float(words[words.index("is") + 1]), int(words[words.index("over") + 1]), float(words[-1].rstrip(")"))
    assert abs(perplexity - math.exp(-ll / tokens)) <= 1e-4 * perplexity
    return ll, tokens


def test_launch_test_with_the_flag(ap_train, tmp_path, capsys):
    from pylda_amd import cli
    words = [str(w) for w in ap_train["words"]]
    ptr, ids, cts = ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"]
    source = tmp_path / "in" / "ap120"
    source.mkdir(parents=True)
    heldout = _documents(words, ptr, ids, cts, range(300, 312))
    (source / "train.dat").write_text("\n".join(_documents(words, ptr, ids, cts, range(120))) + "\n")
    (source / "test.dat").write_text("\n".join(heldout + ["not-a-word"]) + "\n")
    (source / "voc.dat").write_text("\n".join(words) + "\n")
    all_tokens = sum(len(d.split()) for d in heldout)
    common = ["--input_directory=%s" % source, "--number_of_topics=5", "--training_iterations=2", "--snapshot_interval=2"]

    def trained(name, *flags):
        assert cli.train_main(common + ["--output_directory=%s" % (tmp_path / name)] + list(flags)) == 0
        return tmp_path / name / "ap120" / os.listdir(tmp_path / name / "ap120")[0]
    vb = trained("vb")
    capsys.readouterr()
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % vb]) == 0
    assert "left-to-right" not in capsys.readouterr().out and (vb / "test-2").exists()
    os.remove(vb / "test-2")
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % vb, "--left_to_right=3"]) == 0
    out = capsys.readouterr().out
    ll, tokens = _line(out)
    assert tokens == all_tokens and ll < 0 and "held-out likelihood of snapshot" not in out and not (vb / "test-2").exists()
    with open(vb / "model-2", "rb") as stream:
        engine = pickle.load(stream)
    engine._verbose = False
    assert ("is %g" % engine.left_to_right(heldout, 3)[0]) in out
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % vb, "--left_to_right=3",
                          "--left_to_right_resample=0"]) == 0
    sequential = _line(capsys.readouterr().out)
    assert sequential[1] == all_tokens and sequential[0] != ll
    # a mode-1 snapshot needs no fold-in sweeps for it
    gibbs = trained("gibbs", "--inference_mode=1", "--sampler_seed=3", "--gibbs_blocks=8")
    capsys.readouterr()
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % gibbs, "--left_to_right=3"]) == 0
    ll, tokens = _line(capsys.readouterr().out)
    assert tokens == all_tokens and ll < 0

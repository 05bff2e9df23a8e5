"""The collapsed variational Bayes engine (CVB0) on the GPU (pylda_cvb0_*, estep_cvb0.h) against its numpy restatement
(tests/cvb0_restatement.py), bit for bit - there is no transcendental in the chain - and CollapsedVariationalBayes /
launch_train --inference_mode=3 built on it."""
import os
import pickle

import numpy as np
import pytest

import cvb0_restatement as spec
import foldin_restatement
from conftest import csr_slice, rel_err

pytestmark = pytest.mark.gpu

STAGES = (0, 1, 2, 5)          # sweeps after which the states are compared


def _stack(*documents):
    """CSR of documents given as (term ids, counts)."""
    ptr = np.concatenate([[0], np.cumsum([len(i) for i, _ in documents])]).astype(np.int64)
    return (ptr, np.concatenate([np.asarray(i) for i, _ in documents]).astype(np.int32),
            np.concatenate([np.asarray(c) for _, c in documents]).astype(np.int32))


def _synthetic(D, V, lo, hi, seed, max_count=3):
    rng = np.random.default_rng(seed)
    documents = []
    for _ in range(D):
        u = rng.choice(V, size=min(int(rng.integers(lo, hi + 1)), V), replace=False)
        documents.append((u, rng.integers(1, max_count + 1, size=u.size)))
    return _stack(*documents)


def _case(name):
    """(K, V, csr, alpha, beta, blocks, first_document): vector priors everywhere but "scalar"."""
    rng = np.random.default_rng(sum(map(ord, name)))
    first = 0
    if name.startswith("k") and name[1:].isdigit():          # 37 documents over 300 words: more than one workgroup
        K, V, blocks = int(name[1:]), 300, 4
        csr = _synthetic(37, V, 3, 30, K)
    elif name == "long":                                       # a document of 3000 terms
        K, V, blocks = 16, 3500, 2
        csr = _stack((rng.choice(V, 3000, replace=False), rng.integers(1, 3, 3000)), *[
            (rng.choice(V, 12, replace=False), np.ones(12, int)) for _ in range(5)])
    elif name == "edges":                                      # a term with count 300, one-token documents, an empty document
        K, V, blocks = 16, 50, 3
        ptr, ids, cts = _synthetic(10, V, 2, 20, 4)
        every = [(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]]) for d in range(10)]
        csr = _stack(([7], [1]), *every[:4], ([17, 3], [300, 2]), ([], []), *every[4:], ([9], [1]))
    elif name == "more_blocks":                                # G > D, and global indices that do not start at 0
        K, V, blocks, first = 70, 120, 50, 5
        csr = _synthetic(9, V, 2, 25, 6)
    elif name.startswith("v"):                                 # the n_k chunks of 1024 words
        K, V, blocks = 8, int(name[1:]), 2
        csr = _synthetic(12, V, 1, 40, V, max_count=4)
    elif name.startswith("post"):                              # word 0 in n documents of block 0: the apply segments of 256
        n = int(name[4:])
        K, V, blocks = 4, 40, 2
        documents = []
        for d in range(2 * n + 5):
            rest = rng.choice(np.arange(1, V), size=int(rng.integers(1, 4)), replace=False)
            ids = np.concatenate([rest[:1], [0], rest[1:]]) if d % 2 == 0 and d // 2 < n else rest
            documents.append((ids, rng.integers(1, 3, size=ids.size)))
        csr = _stack(*documents)
    else:
        assert name == "scalar"
        K, V, blocks = 20, 200, 3
        csr = _synthetic(30, V, 2, 30, 8)
        return K, V, csr, np.full(K, 0.1), np.full(V, 0.01), blocks, first
    return K, V, csr, rng.uniform(0.02, 0.5, K), rng.uniform(0.005, 0.2, V), blocks, first


def _device_state(ctx, corpus):
    n_kv, n_k, n_dk, g = ctx.cvb0_get_state(corpus)
    assert np.array_equal(n_dk, np.array(ctx.get_gamma(corpus)))        # N_dk lives in the gamma buffer
    return n_kv, n_k, n_dk, g


def _assert_state(got, chain, what):
    for name, a, b in zip(("T", "n_k", "N_dk", "g"), got, chain.state()):
        assert np.array_equal(a, b), "%s: %s differs in %d of %d entries (largest %.3g)" % (
            what, name, int(np.sum(a != b)), a.size, float(np.max(np.abs(a - b))))


def _assert_likelihood(ctx, corpus, chain, alpha, beta, what):
    total, change = ctx.cvb0_log_likelihood(corpus, alpha, beta)
    _, doc_wll, _ = ctx.get_doc_values(corpus)
    want_total, want_docs, want_change = chain.log_likelihood(alpha, beta)
    errs = rel_err(doc_wll, want_docs), rel_err(total, want_total), rel_err(change, want_change)
    print("%s: per-document likelihood rel. error %.3g, total %.3g, change %.3g" % ((what,) + errs))
    assert max(errs) < 1e-12, what
    return total, change


def _run_against_the_restatement(K, V, csr, alpha, beta, blocks, first, seed, what):
    from pylda_amd import _capi
    chain = spec.Cvb0Chain(*csr, K, V, first_document=first)
    chain.init(seed)
    ctx = _capi.Context(K, V)
    try:
        corpus = ctx.corpus(*csr)
        ctx.cvb0_init(corpus, seed, first)
        done = 0
        for stage in STAGES:
            for _ in range(stage - done):
                chain.sweep(alpha, beta, blocks)
                ctx.cvb0_sweep(corpus, alpha, beta, blocks, first)
            done = stage
            _assert_state(_device_state(ctx, corpus), chain, "%s after %d sweeps" % (what, stage))
            _assert_likelihood(ctx, corpus, chain, alpha, beta, "%s after %d sweeps" % (what, stage))
        corpus.close()
    finally:
        ctx.close()
    return chain


@pytest.mark.parametrize("name", ["k1", "k63", "k64", "k65", "k128", "k129", "k256", "k257", "k700", "k1024", "long", "edges",
                                  "more_blocks", "v1", "v1023", "v1024", "v1025", "post257", "post513", "scalar"])
def test_kernels_equal_the_restatement(name):
    K, V, csr, alpha, beta, blocks, first = _case(name)
    chain = _run_against_the_restatement(K, V, csr, alpha, beta, blocks, first, 1000 + len(name), name)
    tokens = float(np.sum(csr[2]))
    assert abs(chain.T.sum() - tokens) <= tokens * 1e-9
    if name == "edges":
        empty = np.nonzero(np.diff(csr[0]) == 0)[0]
        assert len(empty) == 1 and np.all(chain.n_dk[empty] == 0.0)


@pytest.mark.parametrize("blocks", [1, 16, 300])
def test_associated_press_equals_the_restatement(ap_train, blocks):
    csr = csr_slice(ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300))
    K, V = 10, len(ap_train["words"])
    _run_against_the_restatement(K, V, csr, np.full(K, 1.0 / K), np.full(V, 1.0 / V), blocks, 0, 5, "associated press, %d blocks" % blocks)


def _trained(ctx, csr, alpha, beta, blocks, seed, sweeps, first=0):
    corpus = ctx.corpus(*csr)
    ctx.cvb0_init(corpus, seed, first)
    for _ in range(sweeps):
        ctx.cvb0_sweep(corpus, alpha, beta, blocks, first)
    return corpus


def test_same_input_same_bits_and_two_seeds_differ():
    from pylda_amd import _capi
    K, V, csr, alpha, beta, blocks, first = _case("k129")
    ctx = _capi.Context(K, V)
    try:
        results = []
        for seed in (3, 3, 4):
            corpus = _trained(ctx, csr, alpha, beta, blocks, seed, 0)
            start = ctx.cvb0_get_state(corpus)
            for _ in range(3):
                ctx.cvb0_sweep(corpus, alpha, beta, blocks, first)
            results.append((start, ctx.cvb0_get_state(corpus), ctx.cvb0_log_likelihood(corpus, alpha, beta),
                            ctx.get_doc_values(corpus)[1]))
            corpus.close()
        a, b, other = results
        assert all(np.array_equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
        assert a[2] == b[2] and np.array_equal(a[3], b[3]) and a[2][1] > 0.0
        assert not np.array_equal(a[0][3], other[0][3]) and not np.array_equal(a[0][0], other[0][0])
        assert a[2][0] != other[2][0]
    finally:
        ctx.close()


def test_state_round_trip_continues_bit_for_bit():
    from pylda_amd import _capi
    K, V, csr, alpha, beta, blocks, first = _case("k65")
    ctx = _capi.Context(K, V)
    try:
        original = _trained(ctx, csr, alpha, beta, blocks, 9, 3)
        state = ctx.cvb0_get_state(original)
        fresh = ctx.corpus(*csr)
        with pytest.raises(_capi.PyldaError) as e:
            ctx.cvb0_set_state(fresh, n_kv=state[0], n_k=state[1], n_dk=state[2])       # a corpus without a state needs all four
        assert e.value.status == -4
        ctx.cvb0_set_state(fresh, *state)
        for corpus in (original, fresh):
            for _ in range(3):
                ctx.cvb0_sweep(corpus, alpha, beta, blocks, first)
        assert all(np.array_equal(x, y) for x, y in zip(ctx.cvb0_get_state(original), ctx.cvb0_get_state(fresh)))
        assert ctx.cvb0_log_likelihood(original, alpha, beta)[0] == ctx.cvb0_log_likelihood(fresh, alpha, beta)[0]
        # n_k is taken as given, not recomputed
        ctx.cvb0_set_state(fresh, n_k=state[1] + 1.0)
        assert np.array_equal(ctx.cvb0_get_state(fresh, False, False)[1], state[1] + 1.0)
        original.close()
        fresh.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- fold-in
def _hand_made_counts(K, V, rng):
    return (rng.integers(0, 40, (K, V)) * (rng.random((K, V)) < 0.3)).astype(np.int32)


def _fold(ctx, csr, alpha, sweeps, seed, stream, first_document=0):
    corpus = ctx.corpus(*csr)
    try:
        total = ctx.cvb0_foldin(corpus, alpha, sweeps, seed, stream, first_document)
        gamma = np.array(ctx.get_gamma(corpus))
        doc_ll, doc_wll, iters = ctx.get_doc_values(corpus)
        assert np.all(doc_ll == 0.0) and np.all(iters == sweeps)
        assert ctx.estep_results(corpus)[1] == total
    finally:
        corpus.close()
    return total, gamma, doc_wll


def _assert_fold(device, want, what):
    total, gamma, doc_wll = device
    assert np.array_equal(gamma, want["gamma"]), "%s: gamma differs in %d documents" % (
        what, int(np.sum(np.any(gamma != want["gamma"], axis=1))))
    err, err_total = rel_err(doc_wll, want["doc_words_ll"]), rel_err(total, want["words_log_likelihood"])
    print("%s: per-document likelihood rel. error %.3g, total %.3g" % (what, err, err_total))
    assert err < 1e-12 and err_total < 1e-12, what


@pytest.mark.parametrize("K", [65, 1024])
@pytest.mark.parametrize("sweeps", [1, 50])
def test_fold_in_equals_the_restatement(K, sweeps):
    """Against the table of frozen integer counts (pylda_foldin_set_model), whose bits the restatement knows."""
    from pylda_amd import _capi
    rng = np.random.default_rng(K)
    V = 400
    csr = _synthetic(9 if K == 1024 else 40, V, 1, 25, K + 1)
    n_kv, alpha, beta = _hand_made_counts(K, V, rng), rng.uniform(0.02, 0.5, K), rng.uniform(0.005, 0.2, V)
    n_k = n_kv.sum(axis=1).astype(np.int32)
    P = foldin_restatement.predictive_table(n_kv, n_k, beta, float(np.sum(beta)))
    want = spec.fold_in(*csr, P, alpha, 77, 2 ** 31 + 2, sweeps)
    ctx = _capi.Context(K, V)
    try:
        ctx.foldin_set_model(beta, n_kv=n_kv, n_k=n_k)
        _assert_fold(_fold(ctx, csr, alpha, sweeps, 77, 2 ** 31 + 2), want, "K=%d, %d sweeps" % (K, sweeps))
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def ap_model(ap_train):
    """The first 300 associated-press documents after 5 device sweeps, K = 10, 16 blocks: the context with the predictive
    table of n_kv + beta (pylda_set_eta, pylda_completion_set_model), the state read back, the priors."""
    from pylda_amd import _capi
    K, V = 10, len(ap_train["words"])
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    ctx = _capi.Context(K, V)
    trained = _trained(ctx, csr_slice(ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300)), alpha, beta, 16, 5, 5)
    state = ctx.cvb0_get_state(trained)
    ctx.set_eta(state[0] + beta[np.newaxis, :])
    ctx.completion_set_model()
    yield {"ctx": ctx, "trained": trained, "state": state, "alpha": alpha, "beta": beta, "K": K, "V": V}
    trained.close()
    ctx.close()


@pytest.mark.parametrize("sweeps", [1, 50])
def test_fold_in_of_the_press_test_documents(ap_model, ap_test, sweeps):
    """60 documents of the test split (it has word types the training slice never saw) against the table the Python class
    builds; the result does not depend on how the documents are dealt to corpora; the training state is as it was."""
    m = ap_model
    ctx, alpha = m["ctx"], m["alpha"]
    csr = csr_slice(ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"], range(60))
    seen = np.zeros(m["V"], bool)
    seen[m["state"][0].sum(axis=0) > 0] = True
    assert not np.all(seen[csr[1]])
    P = spec.predictive_table(m["state"][0], m["beta"])
    want = spec.fold_in(*csr, P, alpha, 31, 2 ** 31, sweeps)
    whole = _fold(ctx, csr, alpha, sweeps, 31, 2 ** 31)
    _assert_fold(whole, want, "press test documents, %d sweeps" % sweeps)
    again = _fold(ctx, csr, alpha, sweeps, 31, 2 ** 31)
    assert again[0] == whole[0] and np.array_equal(again[1], whole[1]) and np.array_equal(again[2], whole[2])
    ptr, ids, cts = csr
    cut_doc = 23
    cut = int(ptr[cut_doc])
    lo = _fold(ctx, (ptr[:cut_doc + 1], ids[:cut], cts[:cut]), alpha, sweeps, 31, 2 ** 31, 0)
    hi = _fold(ctx, (ptr[cut_doc:] - cut, ids[cut:], cts[cut:]), alpha, sweeps, 31, 2 ** 31, cut_doc)
    assert np.array_equal(np.concatenate([lo[1], hi[1]]), whole[1]) and np.array_equal(np.concatenate([lo[2], hi[2]]), whole[2])
    unshifted = _fold(ctx, (ptr[cut_doc:] - cut, ids[cut:], cts[cut:]), alpha, sweeps, 31, 2 ** 31, 0)
    assert not np.array_equal(unshifted[1], hi[1])
    assert all(np.array_equal(x, y) for x, y in zip(ctx.cvb0_get_state(m["trained"]), m["state"]))


# ---------------------------------------------------------------- error codes
def test_error_codes_leave_the_state_alone():
    from pylda_amd import _capi
    csr = _stack(([1, 2], [1, 2]), ([0], [3]))
    K, V = 4, 6
    alpha, beta = np.full(K, 0.1), np.full(V, 0.1)
    ctx = _capi.Context(K, V)

    def status(call, *args):
        with pytest.raises(_capi.PyldaError) as e:
            call(*args)
        assert str(e.value)
        return e.value.status
    try:
        corpus = ctx.corpus(*csr)
        assert status(ctx.cvb0_sweep, corpus, alpha, beta, 1) == -4                  # a sweep before init
        assert status(ctx.cvb0_log_likelihood, corpus, alpha, beta) == -4
        assert status(ctx.cvb0_get_state, corpus) == -4
        assert status(ctx.cvb0_foldin, corpus, alpha, 5) == -4                       # no predictive table
        ctx.foldin_set_model(beta, n_kv=np.ones((K, V), np.int32), n_k=np.full(K, V, np.int32))
        assert status(ctx.cvb0_foldin, corpus, alpha, 0) == -1
        assert status(ctx.cvb0_foldin, corpus, alpha, 5, 0, 2 ** 32) == -1
        assert np.isfinite(ctx.cvb0_foldin(corpus, alpha, 5, 0, 2 ** 32 - 1))
        ctx.cvb0_init(corpus, 1)
        ctx.cvb0_sweep(corpus, alpha, beta, 2)
        before = ctx.cvb0_get_state(corpus)
        assert status(ctx.cvb0_foldin, corpus, alpha, 5) == -4                       # a training corpus is not folded in
        assert status(ctx.cvb0_sweep, corpus, alpha, beta, 0) == -1
        assert status(ctx.cvb0_init, corpus, 1, 2 ** 32) == -1
        assert all(np.array_equal(x, y) for x, y in zip(ctx.cvb0_get_state(corpus), before))
        gibbs = ctx.corpus(*csr)
        ctx.gibbs_init(gibbs, 1)
        assert status(ctx.cvb0_init, gibbs, 1) == -4                                 # the gamma buffer holds another engine's n_dk
        gibbs.close()
        corpus.close()
    finally:
        ctx.close()
    wide = _capi.Context(1025, V)
    try:
        corpus = wide.corpus(*csr)
        assert status(wide.cvb0_init, corpus, 1) == -1
        assert status(wide.cvb0_foldin, corpus, np.full(1025, 0.1), 5) == -1
        corpus.close()
    finally:
        wide.close()


# ---------------------------------------------------------------- the Python class
def _ap_text(ap_train, docs):
    words = [str(w) for w in ap_train["words"]]
    ptr, ids, cts = ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"]
    return [" ".join(" ".join([words[t]] * int(c)) for t, c in zip(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]]))
            for d in docs], words


def _engine(ap_train, sweeps=3, documents=120):
    from pylda_amd.cvb0 import CollapsedVariationalBayes
    docs, words = _ap_text(ap_train, range(documents))
    m = CollapsedVariationalBayes(seed=21, blocks=8)
    m._verbose = False
    m._initialize(docs, words, 10, 0.1, 1.0 / len(words))
    for _ in range(sweeps):
        m.learning()
    return m


def test_a_pickle_at_iteration_3_continues_bit_for_bit(ap_train):
    m = _engine(ap_train)
    assert m._counter == 3 and 0.0 < m.last_change < 2.0
    blob = pickle.dumps(m)
    restored = pickle.loads(blob)
    assert restored._ctx is None and restored._train_corpus is None and len(restored._host_state) == 4
    assert restored._counter == 3
    heldout, _ = _ap_text(ap_train, range(300, 320))
    ll, gamma = m.inference(heldout + ["not-a-word"], 10)
    ll_r, gamma_r = restored.inference(heldout, 10)                  # from the host state: nothing is uploaded
    assert restored._train_corpus is None
    assert gamma.shape == (20, 10) and ll == ll_r and np.array_equal(gamma, gamma_r) and np.all(gamma > 0)
    assert m.inference(heldout, 10)[0] != ll                        # the n-th call has a stream of its own
    for _ in range(2):
        assert m.learning() == restored.learning()
    assert all(np.array_equal(x, y) for x, y in zip(m._state(True, True), restored._state(True, True)))
    assert m.last_change == restored.last_change
    with pytest.raises(NotImplementedError):
        type(m)(process_group=object())


def test_inspection_methods_delegate_to_the_existing_entries(ap_train):
    """Each equals, bit for bit, what the existing entry gives when called directly with the table n_kv + beta and the same
    gamma."""
    from pylda_amd import _capi, coherence, topics
    from pylda_amd.corpus import split_for_completion
    from pylda_amd.hybrid import _grouped_csr
    from pylda_amd.variational_bayes import LEFT_TO_RIGHT_STREAM_BASE
    m = _engine(ap_train)
    heldout, _ = _ap_text(ap_train, range(300, 315))
    table = m._n_kv + m._alpha_beta[np.newaxis, :]
    csr = _grouped_csr(m.parse_data(heldout))
    held_ll, held_tokens, gamma = m.document_completion(heldout, 10)
    ltr = m.left_to_right(heldout, 4)
    top = m.top_words(6)
    scored = m.topic_coherence(heldout, 6)
    distances = m.topic_distances()
    nearest = m.similar_documents(gamma, 3)
    assert nearest.ids.shape == (15, 3) and len(m.top_documents(2)) == 10

    ctx = _capi.Context(10, m._number_of_types)
    try:
        ctx.set_eta(table)
        ctx.completion_set_model()
        observed_csr, held_csr = split_for_completion(*csr)
        held = ctx.corpus(*held_csr)
        assert ctx.completion_score(held, gamma=gamma) == (held_ll, held_tokens)
        held.close()
        whole = ctx.corpus(*csr)
        assert ctx.left_to_right(whole, m._alpha_alpha, 4, True, 21, LEFT_TO_RIGHT_STREAM_BASE) == ltr[:2]
        assert np.array_equal(ctx.get_doc_values(whole)[1], ltr[2])
        ids, values = ctx.top_words(6, table=table)
        assert top == coherence.words_of(m, ids, values)
        direct = coherence.score_topics(ctx, ids, values, whole)
        assert np.array_equal(direct.umass, scored.umass) and np.array_equal(direct.npmi, scored.npmi)
        whole.close()
        assert np.array_equal(topics.topic_distances(m, table, None, "jensen_shannon").values, distances.values)
        assert np.array_equal(ctx.topic_distances(table, None, 1), distances.values)
    finally:
        ctx.close()


def test_launch_train_mode_3_and_launch_test(ap_train, tmp_path, capsys):
    from pylda_amd import launch_test, launch_train
    from pylda_amd.cvb0 import CollapsedVariationalBayes
    docs, words = _ap_text(ap_train, range(120))
    corpus_dir = tmp_path / "mini-press"
    corpus_dir.mkdir()
    (corpus_dir / "train.dat").write_text("\n".join(docs[:100]) + "\n")
    (corpus_dir / "test.dat").write_text("\n".join(docs[100:120]) + "\n")
    (corpus_dir / "voc.dat").write_text("".join("%s\t1\t1\n" % w for w in words))
    out_dir = tmp_path / "out"
    assert launch_train.main(["--input_directory=%s" % corpus_dir, "--output_directory=%s" % out_dir, "--number_of_topics=5",
                              "--training_iterations=4", "--snapshot_interval=2", "--inference_mode=3", "--sampler_seed=1",
                              "--cvb0_blocks=8"]) == 0
    out = capsys.readouterr().out
    assert "cvb0_blocks=8" in out and "gibbs_blocks" not in out
    runs = list((out_dir / "mini-press").iterdir())
    assert len(runs) == 1 and runs[0].name.endswith("-im3")
    assert sorted(p.name for p in runs[0].iterdir()) == ["exp_beta-2", "exp_beta-4", "exp_gamma-2", "exp_gamma-4", "model-4", "option.txt"]
    opts = dict(l.split("=", 1) for l in (runs[0] / "option.txt").read_text().splitlines())
    assert opts["inference_mode"] == "3" and opts["sampler_seed"] == "1" and opts["cvb0_blocks"] == "8" and "gibbs_blocks" not in opts
    with open(runs[0] / "model-4", "rb") as f:
        model = pickle.load(f)
    assert isinstance(model, CollapsedVariationalBayes) and model._sampler_seed == 1 and model._counter == 4
    base = ["--input_directory=%s" % corpus_dir, "--model_directory=%s" % runs[0], "--snapshot_index=4"]
    assert launch_test.main(base) == 0
    assert "held-out likelihood of snapshot" in capsys.readouterr().out
    gamma = np.loadtxt(runs[0] / "test-4")
    assert gamma.shape == (20, 5) and np.all(gamma > 0)
    os.remove(runs[0] / "test-4")
    assert launch_test.main(base + ["--document_completion=1", "--topic_coherence=5"]) == 0
    out = capsys.readouterr().out
    assert "document-completion likelihood of snapshot" in out and "topic coherence of snapshot" in out
    assert (runs[0] / "test-4").exists() and (runs[0] / "coherence-4").exists()
    assert launch_test.main(base + ["--left_to_right=2", "--topic_coherence=5"]) == 0
    assert "left-to-right likelihood of snapshot" in capsys.readouterr().out

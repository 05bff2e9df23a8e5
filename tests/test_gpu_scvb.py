"""Stochastic collapsed variational Bayes (SCVB0) on the GPU (pylda_scvb_*, scvb_kernels.h) against its numpy restatement
(tests/scvb_restatement.py), bit for bit - a step is add, multiply and divide, the step sizes are the host's - and
StochasticCollapsedVariationalBayes / launch_train --inference_mode=3 --cvb0_minibatches built on it."""
import pickle

import numpy as np
import pytest

import cvb0_restatement
import scvb_restatement as spec
from conftest import csr_slice, rel_err
from test_gpu_cvb0 import _ap_text, _case as _cvb0_case, _stack

pytestmark = pytest.mark.gpu

SCHEDULE = dict(tau0=10.0, kappa=0.9, theta_tau0=10.0, theta_kappa=0.9)


def _case(name):
    """(K, V, csr, alpha, beta, batches, first_document): the CVB0 engine's cases (its `blocks` are the minibatches), and"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "counts":            # term counts 1, 2, 3, 300 and 10^6: the power's bit pattern and its underflow to 0
        K, V = 12, 30
        documents = [([1, 4, 7, 9, 2], [1, 2, 3, 300, 10 ** 6]), ([4, 2, 11], [10 ** 6, 1, 3]), ([9, 1], [300, 2]), ([5], [10 ** 6])]
        documents += [(rng.choice(V, 6, replace=False), rng.integers(1, 4, 6)) for _ in range(5)]
        return K, V, _stack(*documents), rng.uniform(0.02, 0.5, K), rng.uniform(0.005, 0.2, V), 3, 0
    if name == "infinite":          # alpha of topic 1 is 1e308 and every word is heavy: every slot's total is infinite
        K, V = 4, 5
        csr = _stack(*[(np.arange(V), np.full(V, 40)) for _ in range(6)])
        return K, V, csr, np.array([0.1, 1e308, 0.1, 0.1]), rng.uniform(0.005, 0.2, V), 2, 0
    if name == "partly_infinite":   # ... and beside the heavy words a light one per document, whose total stays finite
        K, V = 4, 12
        csr = _stack(*[([0, 1, 5 + d, 2, 3, 4], [40, 40, 1, 40, 40, 40]) for d in range(6)])
        return K, V, csr, np.array([0.1, 1e308, 0.1, 0.1]), rng.uniform(0.005, 0.02, V), 2, 0
    return _cvb0_case(name)


def _block_tokens(csr, batches, first, block):
    ptr, _, cts = csr
    offsets = np.concatenate([[0], np.cumsum(cts, dtype=np.int64)])
    tokens = offsets[ptr[1:]] - offsets[ptr[:-1]]
    return int(tokens[(first + np.arange(len(tokens))) % batches == block].sum())


def _device_step(ctx, corpus, csr, t, batches, first, burn_in, alpha, beta, schedule=SCHEDULE):
    """Step t through the C ABI, with the parameters the restatement forms"""
    block_tokens = _block_tokens(csr, batches, first, t % batches)
    if block_tokens == 0:
        return
    keep, gain, rho_theta, _ = spec.step_parameters(t, batches, burn_in, schedule["tau0"], schedule["kappa"], schedule["theta_tau0"],
                                                    schedule["theta_kappa"], int(np.sum(csr[2])), block_tokens)
    ctx.scvb_step(corpus, t % batches, batches, alpha, beta, keep, gain, rho_theta, first)


def _device_state(ctx, corpus):
    n_kv, n_k, n_dk, doc_change = ctx.scvb_get_state(corpus)
    assert np.array_equal(n_dk, np.array(ctx.get_gamma(corpus)))        # N_dk lives in the gamma buffer
    return n_kv, n_k, n_dk, doc_change


def _assert_state(got, chain, what):
    for name, a, b in zip(("T", "n_k", "N_dk", "doc_change"), got, chain.state() + (chain.doc_change,)):
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


def _run_against_the_restatement(K, V, csr, alpha, beta, batches, first, seed, what, burn_in=1):
    """The start, and 1, 2 and B + 1 steps (the last crosses the epoch boundary, where the documents' schedule moves on)"""
    from pylda_amd import _capi
    chain = spec.ScvbChain(*csr, K, V, first_document=first)
    chain.init(seed)
    ctx = _capi.Context(K, V)
    try:
        corpus = ctx.corpus(*csr)
        ctx.scvb_init(corpus, seed, first)
        done = 0
        for stage in sorted({0, 1, 2, batches + 1}):
            for t in range(done, stage):
                chain.step(alpha, beta, batches, burn_in=burn_in, **SCHEDULE)
                _device_step(ctx, corpus, csr, t, batches, first, burn_in, alpha, beta)
            done = stage
            label = "%s after %d steps" % (what, stage)
            _assert_state(_device_state(ctx, corpus), chain, label)
            _assert_likelihood(ctx, corpus, chain, alpha, beta, label)
        corpus.close()
    finally:
        ctx.close()
    return chain


@pytest.mark.parametrize("name", ["k1", "k63", "k64", "k65", "k128", "k129", "k256", "k257", "k512", "k513", "k700", "k1024", "long",
                                  "edges", "counts", "more_blocks", "v1", "v1023", "v1024", "v1025", "post255", "post256", "post257",
                                  "post513", "scalar"])
def test_kernels_equal_the_restatement(name):
    K, V, csr, alpha, beta, batches, first = _case(name)
    chain = _run_against_the_restatement(K, V, csr, alpha, beta, batches, first, 1000 + len(name), name, burn_in=0 if name == "long" else 1)
    tokens = float(np.sum(csr[2]))
    assert np.all(np.abs(chain.n_dk.sum(axis=1) - chain.doc_tokens) <= 1e-9 * chain.doc_tokens)      # a row keeps the sum C_j
    assert abs(chain.T.sum() - tokens) <= tokens * 1e-9                                               # ... and T the sum C
    if name == "edges":
        empty = np.nonzero(np.diff(csr[0]) == 0)[0]
        assert len(empty) == 1 and np.all(chain.n_dk[empty] == 0.0)
    if name == "counts":
        assert spec.binary_power(1.0 - 11.0 ** -0.9, [10 ** 6])[0] == 0.0


@pytest.mark.parametrize("burn_in", [0, 1, 3, 15])
def test_burn_in_passes_equal_the_restatement(burn_in):
    K, V, csr, alpha, beta, batches, first = _case("k65")
    _run_against_the_restatement(K, V, csr, alpha, beta, batches, first, 77, "burn_in %d" % burn_in, burn_in=burn_in)


@pytest.mark.parametrize("batches", [1, 8, 300])
def test_associated_press_equals_the_restatement(ap_train, batches):
    from pylda_amd import _capi
    csr = csr_slice(ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300))
    K, V = 10, len(ap_train["words"])
    alpha, beta = np.full(K, 1.0 / K), np.full(V, 1.0 / V)
    steps = min(batches + 1, 12)
    chain = spec.ScvbChain(*csr, K, V)
    chain.init(5)
    ctx = _capi.Context(K, V)
    try:
        corpus = ctx.corpus(*csr)
        ctx.scvb_init(corpus, 5)
        for t in range(steps):
            chain.step(alpha, beta, batches, **SCHEDULE)
            _device_step(ctx, corpus, csr, t, batches, 0, 1, alpha, beta)
        _assert_state(_device_state(ctx, corpus), chain, "associated press, %d minibatches" % batches)
        _assert_likelihood(ctx, corpus, chain, alpha, beta, "associated press, %d minibatches" % batches)
        corpus.close()
    finally:
        ctx.close()


def test_an_infinite_total_leaves_the_document_alone():
    """alpha_k = 1e308 for one topic: a * b overflows, total is infinite, the slot neither moves N_dk nor contributes: the
    step only decays the table, in the restatement as on the device."""
    from pylda_amd import _capi
    K, V, csr, alpha, beta, batches, first = _case("infinite")
    chain = _run_against_the_restatement(K, V, csr, alpha, beta, batches, first, 3, "infinite total")
    start = spec.ScvbChain(*csr, K, V)
    start.init(3)
    assert np.array_equal(chain.n_dk, start.n_dk) and np.all(chain.doc_change == 0.0)
    T = start.T.copy()
    for t in range(batches + 1):
        T = spec.step_parameters(t, batches, 1, 10.0, 0.9, 10.0, 0.9, 1, 1)[0] * T
    assert np.array_equal(chain.T, T) and T.sum() > 0.0


def test_an_infinite_total_beside_slots_that_move():
    """The same alpha, and in every document one word of count 1 between the heavy ones: its table entry for the heavy topic
    is 0 or 1, a * b stays below the largest double and the slot moves, while the slots before and after it in the same
    document do not - the prefetch and nd carry over a skipped slot, and the blend sums zero rows beside others."""
    K, V, csr, alpha, beta, batches, first = _case("partly_infinite")
    start = spec.ScvbChain(*csr, K, V)
    start.init(3)
    entry = start.T[csr[1], 1] + beta[csr[1]]
    assert np.all((entry > 1.8) == (csr[2] == 40)) and np.all(entry[csr[2] == 1] < 1.7)      # heavy: overflow; light: none
    chain = _run_against_the_restatement(K, V, csr, alpha, beta, batches, first, 3, "partly infinite total")
    assert np.all(chain.doc_change > 0.0) and not np.array_equal(chain.n_dk, start.n_dk)     # every document moved ...
    light = csr[1][csr[2] == 1]
    assert np.all(chain.T[light].sum(axis=1) > 0.0)
    assert np.allclose(chain.n_dk.sum(axis=1), chain.doc_tokens, rtol=1e-9)


def test_a_word_outside_the_minibatch_decays_by_keep_alone():
    from pylda_amd import _capi
    K, V, csr, alpha, beta, batches, first = _case("scalar")
    ptr, ids, _ = csr
    ctx = _capi.Context(K, V)
    try:
        corpus = ctx.corpus(*csr)
        ctx.scvb_init(corpus, 6, first)
        before = ctx.scvb_get_state(corpus)[0]
        _device_step(ctx, corpus, csr, 0, batches, first, 1, alpha, beta)
        after = ctx.scvb_get_state(corpus)[0]
        in_block = np.zeros(V, bool)
        for d in range(0, len(ptr) - 1, batches):
            in_block[ids[ptr[d]:ptr[d + 1]]] = True
        outside = ~in_block & (before.sum(axis=0) > 0)
        assert outside.sum() > 5 and in_block.sum() > 5
        keep = spec.step_parameters(0, batches, 1, 10.0, 0.9, 10.0, 0.9, 1, 1)[0]
        assert np.array_equal(after[:, outside], keep * before[:, outside])
        assert not np.array_equal(after[:, in_block], keep * before[:, in_block])
        corpus.close()
    finally:
        ctx.close()


def _trained(ctx, csr, alpha, beta, batches, seed, steps, first=0, burn_in=1):
    corpus = ctx.corpus(*csr)
    ctx.scvb_init(corpus, seed, first)
    for t in range(steps):
        _device_step(ctx, corpus, csr, t, batches, first, burn_in, alpha, beta)
    return corpus


def test_same_input_same_bits_and_two_seeds_differ():
    from pylda_amd import _capi
    K, V, csr, alpha, beta, batches, first = _case("k129")
    ctx = _capi.Context(K, V)
    try:
        results = []
        for seed in (3, 3, 4):
            corpus = _trained(ctx, csr, alpha, beta, batches, seed, 5, first)
            results.append((ctx.scvb_get_state(corpus), ctx.cvb0_log_likelihood(corpus, alpha, beta), ctx.get_doc_values(corpus)[1]))
            corpus.close()
        a, b, other = results
        assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and a[1][1] > 0.0
        assert not np.array_equal(a[0][0], other[0][0]) and a[1][0] != other[1][0]
    finally:
        ctx.close()


def test_state_round_trip_continues_bit_for_bit():
    from pylda_amd import _capi
    K, V, csr, alpha, beta, batches, first = _case("k65")
    ctx = _capi.Context(K, V)
    try:
        original = _trained(ctx, csr, alpha, beta, batches, 9, 3, first)
        state = ctx.scvb_get_state(original)
        fresh = ctx.corpus(*csr)
        with pytest.raises(_capi.PyldaError) as e:
            ctx.scvb_set_state(fresh, n_kv=state[0], n_k=state[1])       # a corpus without a state needs all three
        assert e.value.status == -4
        ctx.scvb_set_state(fresh, *state[:3])
        for corpus in (original, fresh):
            for t in range(3, 6):
                _device_step(ctx, corpus, csr, t, batches, first, 1, alpha, beta)
        # (doc_change is no part of the state: block 2 is not visited again in steps 3 .. 5, its documents' stay 0 in `fresh`)
        assert all(np.array_equal(x, y) for x, y in zip(ctx.scvb_get_state(original)[:3], ctx.scvb_get_state(fresh)[:3]))
        visited = np.arange(len(csr[0]) - 1) % batches != 2
        assert np.array_equal(ctx.scvb_get_state(original)[3][visited], ctx.scvb_get_state(fresh)[3][visited])
        assert ctx.cvb0_log_likelihood(original, alpha, beta)[0] == ctx.cvb0_log_likelihood(fresh, alpha, beta)[0]
        ctx.scvb_set_state(fresh, n_k=state[1] + 1.0)                    # n_k is taken as given, not recomputed
        assert np.array_equal(ctx.scvb_get_state(fresh, False)[1], state[1] + 1.0)
        original.close()
        fresh.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- error codes
def test_error_codes():
    from pylda_amd import _capi
    csr = _stack(([1, 2], [1, 2]), ([0], [3]))
    K, V = 4, 6
    alpha, beta = np.full(K, 0.1), np.full(V, 0.1)
    ctx = _capi.Context(K, V)

    def status(call, *args, **kwargs):
        with pytest.raises(_capi.PyldaError) as e:
            call(*args, **kwargs)
        assert str(e.value)
        return e.value.status
    try:
        corpus = ctx.corpus(*csr)
        assert status(ctx.scvb_step, corpus, 0, 1, alpha, beta, 0.5, 0.5, [0.5]) == -4          # a step before the start
        assert status(ctx.scvb_get_state, corpus) == -4
        ctx.scvb_init(corpus, 1)
        ctx.scvb_step(corpus, 0, 2, alpha, beta, 0.5, 1.0, [0.5, 0.25])
        before = ctx.scvb_get_state(corpus)
        assert status(ctx.scvb_step, corpus, 0, 0, alpha, beta, 0.5, 0.5, [0.5]) == -1          # B < 1
        assert status(ctx.scvb_step, corpus, 2, 2, alpha, beta, 0.5, 0.5, [0.5]) == -1          # a block outside [0, B)
        assert status(ctx.scvb_step, corpus, 0, 2, alpha, beta, 0.5, 0.5, [0.5] * 17) == -1     # burn_in 16
        assert status(ctx.scvb_step, corpus, 0, 2, alpha, beta, 0.5, 0.5, []) == -1
        assert status(ctx.scvb_step, corpus, 0, 2, alpha, beta, 0.5, 0.5, [1.5]) == -1
        assert status(ctx.scvb_step, corpus, 0, 2, alpha, beta, 1.0, 0.5, [0.5]) == -1
        assert status(ctx.scvb_step, corpus, 0, 2, alpha, beta, 0.5, float("inf"), [0.5]) == -1
        # the CVB0 entries on a SCVB0 state: all but the likelihood refuse it
        assert status(ctx.cvb0_init, corpus, 1) == -4
        assert status(ctx.cvb0_sweep, corpus, alpha, beta, 2) == -4
        assert status(ctx.cvb0_get_state, corpus) == -4
        assert status(ctx.cvb0_set_state, corpus, n_k=before[1]) == -4
        ctx.foldin_set_model(beta, n_kv=np.ones((K, V), np.int32), n_k=np.full(K, V, np.int32))
        assert status(ctx.cvb0_foldin, corpus, alpha, 5) == -4
        assert np.isfinite(ctx.cvb0_log_likelihood(corpus, alpha, beta)[0])
        assert all(np.array_equal(x, y) for x, y in zip(ctx.scvb_get_state(corpus), before))
        before = before[:3]
        # ... and the reverse, and a Gibbs state
        other = ctx.corpus(*csr)
        ctx.cvb0_init(other, 1)
        assert status(ctx.scvb_init, other, 1) == -4
        assert status(ctx.scvb_step, other, 0, 1, alpha, beta, 0.5, 0.5, [0.5]) == -4
        assert status(ctx.scvb_get_state, other) == -4
        assert status(ctx.scvb_set_state, other, *before) == -4
        other.close()
        gibbs = ctx.corpus(*csr)
        ctx.gibbs_init(gibbs, 1)
        assert status(ctx.scvb_init, gibbs, 1) == -4
        gibbs.close()
        corpus.close()
    finally:
        ctx.close()
    wide = _capi.Context(1025, V)
    try:
        corpus = wide.corpus(*csr)
        assert status(wide.scvb_init, corpus, 1) == -1
        corpus.close()
    finally:
        wide.close()


# ---------------------------------------------------------------- the Python class
def _engine(ap_train, epochs=2, documents=120, batches=8):
    from pylda_amd.scvb0 import StochasticCollapsedVariationalBayes
    docs, words = _ap_text(ap_train, range(documents))
    m = StochasticCollapsedVariationalBayes(batches, seed=21)
    m._verbose = False
    m._initialize(docs, words, 10, 0.1, 1.0 / len(words))
    for _ in range(epochs):
        m.learning()
    return m


def test_the_class_runs_the_restatements_chain(ap_train):
    from pylda_amd.hybrid import _grouped_csr
    m = _engine(ap_train, epochs=0)
    csr = _grouped_csr(m._parsed_corpus)
    chain = spec.ScvbChain(*csr, 10, m._number_of_types)
    chain.init(21)
    start = m.log_likelihood()[0]
    for _ in range(2):
        got = m.learning()
        chain.epoch(m._alpha_alpha, m._alpha_beta, 8, burn_in=1, **SCHEDULE)
    _assert_state(m._state(), chain, "the class after 2 epochs")
    want, _, change = chain.log_likelihood(m._alpha_alpha, m._alpha_beta)
    assert rel_err(got, want) < 1e-12 and rel_err(m.last_change * m._number_of_tokens, change) < 1e-12
    assert m._step == 16 and m._counter == 2 and got > start


def test_a_pickle_after_two_epochs_continues_bit_for_bit(ap_train):
    m = _engine(ap_train)
    blob = pickle.dumps(m)
    restored = pickle.loads(blob)
    assert restored._ctx is None and restored._train_corpus is None and len(restored._host_state) == 3
    assert restored._step == 16 and restored._counter == 2 and restored._burn_in == 1 and restored._tau0 == 10.0
    # held-out documents: the parent's fold-in against the frozen counts, from the host state
    heldout, _ = _ap_text(ap_train, range(300, 320))
    from pylda_amd.hybrid import _grouped_csr
    n_kv = restored._state()[0]
    P = cvb0_restatement.predictive_table(n_kv, m._alpha_beta)
    want = cvb0_restatement.fold_in(*_grouped_csr(m.parse_data(heldout)), P, m._alpha_alpha, 21, 2 ** 31, 10)
    ll, gamma = m.inference(heldout + ["not-a-word"], 10)
    ll_r, gamma_r = restored.inference(heldout, 10)
    assert restored._train_corpus is None
    assert np.array_equal(gamma, want["gamma"]) and rel_err(ll, want["words_log_likelihood"]) < 1e-12
    assert ll == ll_r and np.array_equal(gamma, gamma_r)
    for _ in range(3):
        m.step()
        restored.step()
    assert all(np.array_equal(x, y) for x, y in zip(m._state(), restored._state()))
    assert m.learning() == restored.learning() and m.last_change == restored.last_change


def test_inspection_methods_are_the_parents_on_the_same_tables(ap_train):
    from pylda_amd.cvb0 import CollapsedVariationalBayes
    m = _engine(ap_train)
    snapshot = pickle.loads(pickle.dumps(m))
    parent = CollapsedVariationalBayes.__new__(CollapsedVariationalBayes)
    parent.__dict__.update(snapshot.__dict__)
    parent._host_state = snapshot._host_state + (None,)
    heldout, _ = _ap_text(ap_train, range(300, 315))
    for model in (m, parent):
        model._inference_calls = 0
    a, b = m.document_completion(heldout, 10), parent.document_completion(heldout, 10)
    assert a[:2] == b[:2] and np.array_equal(a[2], b[2])
    a, b = m.left_to_right(heldout, 4), parent.left_to_right(heldout, 4)
    assert a[:2] == b[:2] and np.array_equal(a[2], b[2])
    assert m.top_words(6) == parent.top_words(6)
    a, b = m.topic_coherence(heldout, 6), parent.topic_coherence(heldout, 6)
    assert np.array_equal(a.umass, b.umass) and np.array_equal(a.npmi, b.npmi)
    assert np.array_equal(m.topic_distances().values, parent.topic_distances().values)
    a, b = m.similar_documents(heldout, 3, sweeps=5), parent.similar_documents(heldout, 3, sweeps=5)
    assert np.array_equal(a.ids, b.ids) and a.ids.shape == (15, 3)
    assert m.top_documents(2) == parent.top_documents(2)


def test_launch_train_minibatches_and_launch_test(ap_train, tmp_path, capsys):
    from pylda_amd import launch_test, launch_train
    from pylda_amd.scvb0 import StochasticCollapsedVariationalBayes
    docs, words = _ap_text(ap_train, range(120))
    corpus_dir = tmp_path / "mini-press"
    corpus_dir.mkdir()
    (corpus_dir / "train.dat").write_text("\n".join(docs[:100]) + "\n")
    (corpus_dir / "test.dat").write_text("\n".join(docs[100:120]) + "\n")
    (corpus_dir / "voc.dat").write_text("".join("%s\t1\t1\n" % w for w in words))
    out_dir = tmp_path / "out"
    base = ["--input_directory=%s" % corpus_dir, "--output_directory=%s" % out_dir, "--number_of_topics=5",
            "--training_iterations=4", "--snapshot_interval=2", "--inference_mode=3", "--sampler_seed=1"]
    assert launch_train.main(base + ["--cvb0_minibatches=101"]) == 2                 # more minibatches than documents
    assert "--cvb0_minibatches" in capsys.readouterr().err
    assert launch_train.main(base + ["--cvb0_minibatches=8"]) == 0
    out = capsys.readouterr().out
    assert "cvb0_minibatches=8" in out and "cvb0_blocks" not in out
    runs = [p for p in (out_dir / "mini-press").iterdir() if (p / "model-4").exists()]
    assert len(runs) == 1 and runs[0].name.endswith("-im3")
    opts = dict(l.split("=", 1) for l in (runs[0] / "option.txt").read_text().splitlines())
    assert opts["cvb0_minibatches"] == "8" and opts["cvb0_burn_in"] == "1" and opts["cvb0_tau0"] == "10.0" and opts["cvb0_kappa"] == "0.9"
    assert "cvb0_blocks" not in opts and opts["sampler_seed"] == "1"
    with open(runs[0] / "model-4", "rb") as f:
        model = pickle.load(f)
    assert isinstance(model, StochasticCollapsedVariationalBayes) and model._counter == 4 and model._step == 32
    test = ["--input_directory=%s" % corpus_dir, "--model_directory=%s" % runs[0], "--snapshot_index=4"]
    assert launch_test.main(test) == 0
    assert "held-out likelihood of snapshot" in capsys.readouterr().out
    gamma = np.loadtxt(runs[0] / "test-4")
    assert gamma.shape == (20, 5) and np.all(gamma > 0)

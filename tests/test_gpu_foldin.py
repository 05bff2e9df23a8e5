"""The held-out fold-in on the GPU (pylda_foldin_set_model / pylda_foldin, estep_foldin.h) against its numpy restatement
(tests/foldin_restatement.py) and an exactly enumerated posterior, and MonteCarlo.fold_in / launch_test --fold_in_samples
built on it."""
import os
import pickle

import numpy as np
import pytest

import foldin_fixture as fixture
import foldin_restatement as spec
from conftest import csr_slice, rel_err

pytestmark = pytest.mark.gpu


def _synthetic(D, V, lo, hi, seed, max_count=3):
    rng = np.random.default_rng(seed)
    ptr, ids, cts = [0], [], []
    for _ in range(D):
        n = int(rng.integers(lo, hi + 1))
        u = rng.choice(V, size=min(n, V), replace=False)
        ids.append(u)
        cts.append(rng.integers(1, max_count + 1, size=u.size))
        ptr.append(ptr[-1] + u.size)
    return np.array(ptr, np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(cts).astype(np.int32)


def _stack(*documents):
    """CSR of documents given as (term ids, counts)."""
    ptr = np.concatenate([[0], np.cumsum([len(i) for i, _ in documents])]).astype(np.int64)
    return (ptr, np.concatenate([np.asarray(i) for i, _ in documents]).astype(np.int32),
            np.concatenate([np.asarray(c) for _, c in documents]).astype(np.int32))


def _hand_made_model(K, V, rng):
    """Counts with empty cells and empty-ish topics, vector alpha and beta."""
    n_kv = rng.integers(0, 40, (K, V)) * (rng.random((K, V)) < 0.3)
    return n_kv.astype(np.int32), rng.uniform(0.02, 0.5, K), rng.uniform(0.005, 0.2, V)


def _case(name):
    """(K, V, csr, n_kv, alpha, beta, samples, burn-in)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    samples, burn_in = 4, 2
    if name.startswith("k") and name[1:].isdigit():
        K, V = int(name[1:]), 1500
        csr = _synthetic(300 if K <= 128 else 60, V, 1, 60, K)
    elif name == "edges":                   # K = 1 is a case of its own below
        K, V = 16, 500
        ptr, ids, cts = _synthetic(40, V, 3, 30, 9)
        every = [(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]]) for d in range(40)]
        # a single token, an empty document, one term repeated 300 times - at the start, inside and at the end of workgroups
        csr = _stack(([7], [1]), *every[:5], ([], []), *every[5:], ([17], [300]), ([], []))
    elif name == "long":                    # 3000 terms; exactly 2048 and 2049 tokens (where a variant with topics in LDS switched)
        K, V = 32, 4000
        a = rng.choice(V, 3000, replace=False)
        b = rng.choice(V, 1024, replace=False)
        c = rng.choice(V, 1025, replace=False)
        csr = _stack((a, np.ones(3000, int)), (b, np.full(1024, 2)), (c, np.concatenate([np.full(1024, 2), [1]])), (a[:9], np.ones(9, int)))
        samples, burn_in = 3, 1
    elif name in ("burn_in_0", "burn_in_last", "one_sample"):
        K, V = 65, 800
        csr = _synthetic(70, V, 1, 40, 3)
        samples, burn_in = {"burn_in_0": (5, 0), "burn_in_last": (5, 4), "one_sample": (1, 0)}[name]
    else:
        assert name == "k_one"
        K, V = 1, 50
        csr = _synthetic(9, V, 1, 20, 4)
    n_kv, alpha, beta = _hand_made_model(K, V, rng)
    return K, V, csr, n_kv, alpha, beta, samples, burn_in


def _run(ctx, csr, alpha, samples, burn_in, seed, stream, first_document=0):
    """One fold-in through the C ABI: (total, gamma, per-document likelihoods, iters)."""
    corpus = ctx.corpus(*csr)
    try:
        total = ctx.foldin(corpus, alpha, samples, burn_in, seed, stream, first_document)
        gamma = np.array(ctx.get_gamma(corpus))
        doc_ll, doc_wll, iters = ctx.get_doc_values(corpus)
        assert np.all(doc_ll == 0.0)
        assert ctx.estep_results(corpus)[1] == total
    finally:
        corpus.close()
    return total, gamma, doc_wll, iters


def _assert_equals_restatement(device, want, samples, what):
    total, gamma, doc_wll, iters = device
    assert np.array_equal(gamma, want["gamma"]), "%s: gamma differs in %d documents" % (
        what, int(np.sum(np.any(gamma != want["gamma"], axis=1))))
    err, err_total = rel_err(doc_wll, want["doc_words_ll"]), rel_err(total, want["words_log_likelihood"])
    print("%s: per-document likelihood rel. error %.3g, total %.3g" % (what, err, err_total))
    assert err < 1e-12 and err_total < 1e-12, what
    assert np.all(iters == samples)


@pytest.mark.parametrize("name", ["k64", "k65", "k128", "k256", "k400", "k700", "k1024", "k_one", "edges", "long", "burn_in_0",
                                  "burn_in_last", "one_sample"])
def test_kernel_equals_the_restatement(name):
    from pylda_amd import _capi
    K, V, csr, n_kv, alpha, beta, samples, burn_in = _case(name)
    n_k = n_kv.sum(axis=1).astype(np.int32)
    seed, stream = 4321 + len(name), 2 ** 31 + 5
    want = spec.fold_in(*csr, spec.predictive_table(n_kv, n_k, beta, float(np.sum(beta))), alpha, seed, stream, samples, burn_in)
    ctx = _capi.Context(K, V)
    try:
        ctx.foldin_set_model(beta, n_kv=n_kv, n_k=n_k)
        _assert_equals_restatement(_run(ctx, csr, alpha, samples, burn_in, seed, stream), want, samples, name)
    finally:
        ctx.close()
    if name == "edges":
        empty = np.nonzero(np.diff(csr[0]) == 0)[0]
        assert len(empty) == 2 and np.array_equal(want["gamma"][empty], np.tile(alpha, (2, 1)))
        assert np.all(want["doc_words_ll"][empty] == 0.0)


@pytest.fixture(scope="module")
def ap_model(ap_train):
    """A model from a few device training sweeps over the first 300 associated-press documents, K = 10: the context (its
    fold-in model set from the device corpus), the trained corpus, the counts read back, the priors."""
    from pylda_amd import _capi
    K, V = 10, len(ap_train["words"])
    alpha, beta = np.full(K, 0.1), np.full(V, 1.0 / V)
    ctx = _capi.Context(K, V)
    trained = ctx.corpus(*csr_slice(ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300)))
    ctx.gibbs_init(trained, 8)
    for sweep in range(1, 31):
        ctx.gibbs_sweep(trained, alpha, beta, 16, 8, sweep)
    ctx.foldin_set_model(beta, trained=trained)
    yield {"ctx": ctx, "trained": trained, "counts": ctx.gibbs_get_counts(trained), "alpha": alpha, "beta": beta, "K": K, "V": V,
           "heldout": csr_slice(ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300, 600))}
    trained.close()
    ctx.close()


def test_associated_press_against_the_restatement_and_the_model_from_host_counts(ap_model):
    """300 held-out documents under the device corpus' counts: the restatement, bit for bit in gamma; the same call again
    and the model set from the counts read back to the host give the same bits; another stream does not; the training state
    is as it was."""
    from pylda_amd import _capi
    m = ap_model
    ctx, alpha, beta = m["ctx"], m["alpha"], m["beta"]
    n_kv, n_k, topics = m["counts"]
    seed, stream, samples, burn_in = 99, 2 ** 31, 6, 3
    want = spec.fold_in(*m["heldout"], spec.predictive_table(n_kv, n_k, beta, float(np.sum(beta))), alpha, seed, stream, samples,
                        burn_in)
    first = _run(ctx, m["heldout"], alpha, samples, burn_in, seed, stream)
    _assert_equals_restatement(first, want, samples, "associated press")
    again = _run(ctx, m["heldout"], alpha, samples, burn_in, seed, stream)
    assert again[0] == first[0] and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    other = _run(ctx, m["heldout"], alpha, samples, burn_in, seed, stream + 1)
    assert other[0] != first[0] and not np.array_equal(other[1], first[1])
    after = ctx.gibbs_get_counts(m["trained"])
    assert all(np.array_equal(a, b) for a, b in zip(after, m["counts"]))
    host = _capi.Context(m["K"], m["V"])
    try:
        host.foldin_set_model(beta, n_kv=n_kv, n_k=n_k)
        from_host = _run(host, m["heldout"], alpha, samples, burn_in, seed, stream)
    finally:
        host.close()
    assert from_host[0] == first[0] and np.array_equal(from_host[1], first[1]) and np.array_equal(from_host[2], first[2])


def test_two_shards_equal_the_whole_run(ap_model):
    m = ap_model
    ptr, ids, cts = m["heldout"]
    cut_doc = 130
    cut = int(ptr[cut_doc])
    whole = _run(m["ctx"], m["heldout"], m["alpha"], 5, 2, 7, 3)
    lo = _run(m["ctx"], (ptr[:cut_doc + 1], ids[:cut], cts[:cut]), m["alpha"], 5, 2, 7, 3, 0)
    hi = _run(m["ctx"], (ptr[cut_doc:] - cut, ids[cut:], cts[cut:]), m["alpha"], 5, 2, 7, 3, cut_doc)
    assert np.array_equal(np.concatenate([lo[1], hi[1]]), whole[1])
    assert np.array_equal(np.concatenate([lo[2], hi[2]]), whole[2])
    unshifted = _run(m["ctx"], (ptr[cut_doc:] - cut, ids[cut:], cts[cut:]), m["alpha"], 5, 2, 7, 3, 0)
    assert not np.array_equal(unshifted[1], hi[1])


def test_fold_in_beats_the_prior_proportions(ap_model):
    """Gross-error check: 30 training sweeps on documents 0-299, documents 300-399 folded in; the likelihood per token is
    higher than the same sum with theta = alpha / sum(alpha), from the same P."""
    m = ap_model
    ptr, ids, cts = m["heldout"]
    end = int(ptr[100])
    csr = (ptr[:101], ids[:end], cts[:end])
    total, gamma, doc_wll, _ = _run(m["ctx"], csr, m["alpha"], 50, 25, 1, 2 ** 31)
    n_kv, n_k, _ = m["counts"]
    P = spec.predictive_table(n_kv, n_k, m["beta"], float(np.sum(m["beta"])))
    prior = float(np.sum(cts[:end] * np.log(P[ids[:end]] @ (m["alpha"] / m["alpha"].sum()))))
    tokens = float(np.sum(cts[:end]))
    print("likelihood per token: fold-in %.4f, prior proportions %.4f" % (total / tokens, prior / tokens))
    assert np.isfinite(total) and total / tokens > prior / tokens
    assert np.allclose(gamma.sum(axis=1) - m["alpha"].sum(), np.add.reduceat(cts[:end], ptr[:100]), rtol=0, atol=1e-9)


def test_exact_posterior_on_the_device():
    """The enumeration fixture of tests/test_foldin_host.py on the device: 4000 replicas (global documents 0..3999), 100
    sweeps, burn-in 40, each topic's mean count within 5 standard errors of the exact E[n_dk]."""
    from pylda_amd import _capi
    ctx = _capi.Context(3, 5)
    try:
        ctx.foldin_set_model(fixture.BETA, n_kv=fixture.N_KV, n_k=fixture.N_KV.sum(axis=1))
        _, gamma, _, _ = _run(ctx, fixture.corpus(), fixture.ALPHA, fixture.SWEEPS, fixture.BURN_IN, 11, 2 ** 31)
    finally:
        ctx.close()
    z = fixture.z_scores(gamma)
    print("z per topic:", np.round(z, 2))
    assert np.all(np.abs(z) < 5.0), z


def test_error_codes():
    from pylda_amd import _capi
    csr = _stack(([1, 2], [1, 2]))
    ctx = _capi.Context(4, 6)
    alpha, beta = np.full(4, 0.1), np.full(6, 0.1)
    n_kv = np.ones((4, 6), np.int32)
    try:
        corpus = ctx.corpus(*csr)

        def status(*args):
            with pytest.raises(_capi.PyldaError) as e:
                ctx.foldin(corpus, alpha, *args)
            return e.value.status
        assert status(5, 2, 0, 0) == -4                      # no model
        with pytest.raises(_capi.PyldaError) as e:
            ctx.foldin_set_model(beta, trained=corpus)       # a corpus without a Gibbs state
        assert e.value.status == -4
        ctx.foldin_set_model(beta, n_kv=n_kv, n_k=n_kv.sum(axis=1))
        assert status(5, 5, 0, 0) == -1 and status(5, 6, 0, 0) == -1 and status(5, -1, 0, 0) == -1
        assert status(0, 0, 0, 0) == -1 and status(65535, 0, 0, 0) == -1
        assert status(5, 2, 0, 2 ** 32) == -1
        assert status(5, 2, 0, 0, 2 ** 32) == -1             # first_document
        assert np.isfinite(ctx.foldin(corpus, alpha, 5, 2, 0, 2 ** 32 - 1))
        ctx.gibbs_init(corpus, 1)                            # a training corpus is not folded in: its state would be overwritten
        assert status(5, 2, 0, 0) == -4
        corpus.close()
    finally:
        ctx.close()
    wide = _capi.Context(1025, 6)
    try:
        with pytest.raises(_capi.PyldaError) as e:
            wide.foldin_set_model(beta, n_kv=np.ones((1025, 6), np.int32), n_k=np.full(1025, 6, np.int32))
        assert e.value.status == -1
        corpus = wide.corpus(*csr)
        with pytest.raises(_capi.PyldaError) as e:
            wide.foldin(corpus, np.full(1025, 0.1), 5, 2)
        assert e.value.status == -1
        corpus.close()
    finally:
        wide.close()


def _ap_text(ap_train, docs):
    words = [str(w) for w in ap_train["words"]]
    ptr, ids, cts = ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"]
    return [" ".join(" ".join([words[t]] * int(c)) for t, c in zip(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]]))
            for d in docs], words


def _engine(ap_train, sweeps=3):
    from pylda_amd.monte_carlo import MonteCarlo
    docs, words = _ap_text(ap_train, range(300))
    m = MonteCarlo(hyper_parameter_optimize_interval=1000, seed=21, blocks=16)
    m._verbose = False
    m._initialize(docs, words, 10, 0.1, 1.0 / len(words))
    for _ in range(sweeps):
        m.learning()
    return m


def test_fold_in_leaves_the_training_state_and_survives_a_pickle(ap_train):
    """MonteCarlo.fold_in: the tuple inference() returns elsewhere; n_kv, n_k and the topics are as before and the next
    learning() equals an untouched twin's; a pickled and restored snapshot - evaluated from its host counts, its training
    corpus not uploaded - gives the live object's bits for the same call number, and trains on."""
    heldout, _ = _ap_text(ap_train, range(300, 340))
    m, twin = _engine(ap_train), _engine(ap_train)
    before = m._counts(True, True)
    blob = pickle.dumps(m)
    ll, gamma = m.fold_in(heldout + ["not-a-word"], 8, 4)
    assert gamma.shape == (40, 10) and np.isfinite(ll) and np.all(gamma > 0)
    assert all(np.array_equal(a, b) for a, b in zip(m._counts(True, True), before))
    ll2, gamma2 = m.fold_in(heldout, 8, 4)
    assert ll2 != ll and m._fold_in_calls == 2           # the n-th call draws from stream 2^31 + n
    restored = pickle.loads(blob)
    assert restored._fold_in_calls == 0
    ll_r, gamma_r = restored.fold_in(heldout, 8, 4)
    assert ll_r == ll and np.array_equal(gamma_r, gamma)
    assert restored._train_corpus is None and restored._host_state is not None
    del restored.__dict__["_fold_in_calls"]              # a snapshot from before the counter existed
    assert restored.fold_in(heldout, 8, 4)[0] == ll
    with pytest.raises(NotImplementedError):
        m.inference(heldout)
    assert m.learning() == twin.learning() == restored.learning()
    assert all(np.array_equal(a, b) for a, b in zip(m._counts(True, True), twin._counts(True, True)))


def test_launch_test_folds_in_a_mode_1_snapshot(ap_train, tmp_path, capsys):
    from pylda_amd import cli
    docs, words = _ap_text(ap_train, range(120))
    heldout, _ = _ap_text(ap_train, range(300, 330))
    source = tmp_path / "in" / "ap120"
    source.mkdir(parents=True)
    (source / "train.dat").write_text("\n".join(docs) + "\n")
    (source / "test.dat").write_text("\n".join(heldout + ["not-a-word"]) + "\n")
    (source / "voc.dat").write_text("\n".join(words) + "\n")
    K = 5
    assert cli.train_main(["--input_directory=%s" % source, "--output_directory=%s" % (tmp_path / "out"), "--number_of_topics=%d" % K,
                           "--training_iterations=4", "--snapshot_interval=4", "--inference_mode=1", "--sampler_seed=3",
                           "--gibbs_blocks=8"]) == 0
    run = tmp_path / "out" / "ap120" / os.listdir(tmp_path / "out" / "ap120")[0]
    capsys.readouterr()
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % run, "--fold_in_samples=20"]) == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("held-out likelihood of snapshot")]
    assert len(line) == 1 and np.isfinite(float(line[0].split()[-1]))
    gamma = np.loadtxt(run / "test-4")
    assert gamma.shape == (30, K) and np.all(np.isfinite(gamma))
    # a variational-Bayes snapshot answers inference(): the flag is refused, by name
    assert cli.train_main(["--input_directory=%s" % source, "--output_directory=%s" % (tmp_path / "vb"), "--number_of_topics=%d" % K,
                           "--training_iterations=2", "--snapshot_interval=2"]) == 0
    vb = tmp_path / "vb" / "ap120" / os.listdir(tmp_path / "vb" / "ap120")[0]
    capsys.readouterr()
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % vb, "--fold_in_samples=20"]) == 2
    assert "fold_in" in capsys.readouterr().err

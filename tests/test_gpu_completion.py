"""Document completion on the GPU (pylda_completion_set_model / pylda_completion_score, completion_score.h) against its numpy
restatement with exact sums (tests/completion_restatement.py), and the engines' document_completion() and
launch_test --document_completion built on it.

The bar per document is derived, not tuned (completion_restatement.bar):
    |delta| <= (V + 2 K + 64) 2^-53 N_held + n_terms 2^-53 |ll_d|
Largest |delta| / bar measured on an MI355X, over all cases of test_kernel_equals_the_restatement: see DESIGN.md section 15."""
import math
import os
import pickle

import numpy as np
import pytest

import completion_restatement as spec
import foldin_restatement as foldin_spec
from conftest import csr_slice

pytestmark = pytest.mark.gpu


def _batch(K):
    """The kernel's batch of held terms: 64, 32, 16 for 1, 2, >= 4 topics per lane."""
    return 64 if K <= 64 else 32 if K <= 128 else 16


def _stack(documents):
    """CSR of documents given as (term ids, counts)."""
    ptr = np.concatenate([[0], np.cumsum([len(i) for i, _ in documents])]).astype(np.int64)
    return (ptr, np.concatenate([np.asarray(i, dtype=np.int64) for i, _ in documents]).astype(np.int32),
            np.concatenate([np.asarray(c, dtype=np.int64) for _, c in documents]).astype(np.int32))


_cases = {}


def _case(K, V, D):
    """(held csr, eta, gamma, want = the restatement's (doc_ll, tokens, terms)); computed once, shared, never written."""
    if (K, V, D) in _cases:
        return _cases[(K, V, D)]
    rng = np.random.default_rng(1000 * K + V + D)
    T = _batch(K)

    def doc(n, last_word=False):
        ids = rng.choice(V, size=n, replace=False)
        if last_word and n:
            ids[rng.integers(n)] = V - 1
            ids = np.unique(ids)[::-1]                    # (V - 1 first; still distinct)
        return ids, rng.integers(1, 4, size=len(ids))
    if D == 1:
        documents = [doc(T + 1)]
    elif D == 5:
        documents = [doc(0), doc(T), doc(2 * T + 1, last_word=True), doc(3000 if V >= 3000 else T + 1), ([V - 1], [300])]
    else:
        # 0, 1, T - 1, T, T + 1, 2 T + 1 terms, the last word alone, a 300-fold term - spread over the workgroups' wavefronts
        edges = [doc(0), doc(1), doc(T - 1), doc(T), doc(T + 1), doc(2 * T + 1), ([V - 1], [1]), ([17], [300]), doc(T, last_word=True)]
        documents = [doc(int(rng.integers(1, 41))) for _ in range(D - len(edges) - 1)]
        for at, e in zip((0, 3, 5, 64, 65, 66, 130, 131, 190), edges):
            documents.insert(at, e)
        documents.append(doc(0))                          # an empty document at the end of the grid
    assert len(documents) == D
    csr = _stack(documents)
    eta = rng.gamma(0.3, 1.0, (K, V)) + 1e-3 + 5.0 * (rng.random((K, V)) < 0.02)
    gamma = rng.gamma(0.5, 2.0, (D, K)) + 0.01
    want = spec.score(*csr, spec.predictive_table(eta), gamma)
    _cases[(K, V, D)] = (csr, eta, gamma, want)
    return _cases[(K, V, D)]


def _score(ctx, csr, gamma=None, observed=None):
    """One pylda_completion_score through the binding: (total, tokens, per-document values)."""
    held = ctx.corpus(*csr)
    try:
        total, tokens = ctx.completion_score(held, observed=observed, gamma=gamma)
        doc_ll, doc_wll, iters = ctx.get_doc_values(held)
        assert np.all(doc_ll == 0.0) and np.all(iters == 0)
        assert ctx.estep_results(held)[1] == total
    finally:
        held.close()
    return total, tokens, doc_wll


def _assert_within_the_bar(what, V, K, doc_wll, total, tokens, want):
    want_ll, want_tokens, terms = want
    assert tokens == int(want_tokens.sum()), what
    bar = spec.bar(V, K, want_tokens, terms, want_ll)
    delta = np.abs(doc_wll - want_ll)
    ratio = float(np.max(delta[bar > 0] / bar[bar > 0])) if np.any(bar > 0) else 0.0
    print("%s: largest |delta| / bar %.3f over %d documents, %d held tokens" % (what, ratio, len(want_ll), tokens))
    assert np.all(doc_wll[want_tokens == 0] == 0.0), what          # an empty held document scores exactly 0
    assert np.all(delta <= bar), (what, ratio, int(np.argmax(delta - bar)))
    want_total = math.fsum(want_ll.tolist())
    assert abs(total - want_total) <= float(bar.sum()) + len(want_ll) * 2.0 ** -53 * abs(want_total), what
    return ratio


@pytest.mark.parametrize("K,V,D", [(1, 500, 1), (10, 500, 203), (64, 500, 203), (65, 500, 5), (128, 500, 203), (129, 500, 5),
                                   (256, 500, 203), (257, 500, 5), (512, 500, 5), (513, 500, 203), (1024, 500, 203),
                                   (129, 5000, 5)])
def test_kernel_equals_the_restatement(K, V, D):
    """Host-given gamma: no E-step tolerance enters.  K = 1 makes theta = 1: the score checks the table alone."""
    from pylda_amd import _capi
    csr, eta, gamma, want = _case(K, V, D)
    ctx = _capi.Context(K, V)
    try:
        ctx.set_eta(eta)
        ctx.completion_set_model()
        total, tokens, doc_wll = _score(ctx, csr, gamma=gamma)
    finally:
        ctx.close()
    _assert_within_the_bar("K=%d V=%d D=%d" % (K, V, D), V, K, doc_wll, total, tokens, want)


def test_same_input_same_bits_and_two_shards_equal_the_whole():
    from pylda_amd import _capi
    K, V, D = 128, 500, 203
    (ptr, ids, cts), eta, gamma, _ = _case(K, V, D)
    ctx = _capi.Context(K, V)
    try:
        ctx.set_eta(eta)
        ctx.completion_set_model()
        first = _score(ctx, (ptr, ids, cts), gamma=gamma)
        ctx.completion_set_model()                        # the same eta: the same table, bit for bit
        again = _score(ctx, (ptr, ids, cts), gamma=gamma)
        cut_doc = 67                                      # not a multiple of a workgroup's four wavefronts
        cut = int(ptr[cut_doc])
        lo = _score(ctx, (ptr[:cut_doc + 1], ids[:cut], cts[:cut]), gamma=gamma[:cut_doc])
        hi = _score(ctx, (ptr[cut_doc:] - cut, ids[cut:], cts[cut:]), gamma=gamma[cut_doc:])
    finally:
        ctx.close()
    assert again[0] == first[0] and again[1] == first[1] and np.array_equal(again[2], first[2])
    assert np.array_equal(np.concatenate([lo[2], hi[2]]), first[2]) and lo[1] + hi[1] == first[1]


def test_gamma_from_the_observed_corpus_equals_gamma_from_the_host(ap_train, ap_test):
    from pylda_amd import _capi
    from pylda_amd.corpus import split_for_completion
    K, V = 10, len(ap_train["words"])
    observed_csr, held_csr = split_for_completion(*csr_slice(ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"], range(60)))
    ctx = _capi.Context(K, V)
    try:
        ctx.set_alpha(ap_train["alpha"])
        ctx.set_eta(ap_train["eta"])
        observed = ctx.corpus(*observed_csr)
        ctx.estep(observed, 50, 1e-6, True)
        gamma = np.array(ctx.get_gamma(observed))
        ctx.completion_set_model()
        from_device = _score(ctx, held_csr, observed=observed)
        from_host = _score(ctx, held_csr, gamma=gamma)
        assert np.array_equal(np.array(ctx.get_gamma(observed)), gamma)       # the observed corpus is read, never written
        observed.close()
    finally:
        ctx.close()
    assert from_device[0] == from_host[0] and from_device[1] == from_host[1] and np.array_equal(from_device[2], from_host[2])
    assert np.isfinite(from_host[0]) and from_host[0] < 0


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


def test_variational_bayes_and_the_online_engine(ap_train, ap_test):
    from pylda_amd.corpus import split_for_completion
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    m, words = _vb_engine(VariationalBayes, ap_train)
    test_docs = _documents(words, ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"], range(221))
    plug_in_before = m.inference(test_docs)
    ll, tokens, gamma = m.document_completion(test_docs)
    csr = m.parse_to_csr(test_docs)
    observed_csr, held_csr = split_for_completion(*csr)
    assert np.array_equal(gamma, m.e_step(observed_csr)[1])
    want = spec.score(*held_csr, spec.predictive_table(ap_train["eta"]), gamma)
    assert tokens == int(want[1].sum()) == int(np.sum(held_csr[2]))
    bar = spec.bar(len(words), 10, want[1], want[2], want[0])
    want_total = math.fsum(want[0].tolist())
    print("associated press: %.6f per held token (perplexity %.1f), plug-in %.6f per token" % (
        ll / tokens, math.exp(-ll / tokens), plug_in_before[0] / float(np.sum(csr[2]))))
    assert abs(ll - want_total) <= float(bar.sum()) + len(bar) * 2.0 ** -53 * abs(want_total)
    # the per-document values against the restatement fed that gamma, through the C ABI
    ctx = m._context()
    ctx.completion_set_model()
    total, _, doc_wll = _score(ctx, held_csr, gamma=gamma)
    assert total == ll
    _assert_within_the_bar("associated press K=10", len(words), 10, doc_wll, total, tokens, want)
    # inference() is what it was, the method repeats itself, and a pickled engine gives the same bits
    plug_in_after = m.inference(test_docs)
    assert plug_in_after[0] == plug_in_before[0] and np.array_equal(plug_in_after[1], plug_in_before[1])
    restored = pickle.loads(pickle.dumps(m))
    again = restored.document_completion(test_docs)
    assert again[0] == ll and again[1] == tokens and np.array_equal(again[2], gamma)
    online, _ = _vb_engine(OnlineVariationalBayes, ap_train, 4)
    got = online.document_completion(test_docs)
    assert got[0] == ll and got[1] == tokens and np.array_equal(got[2], gamma)


def test_hybrid_same_seed_and_stream_same_bits(ap_train, ap_test):
    from pylda_amd.hybrid import Hybrid
    a, words = _vb_engine(Hybrid, ap_train, seed=5)
    b, _ = _vb_engine(Hybrid, ap_train, seed=5)
    test_docs = _documents(words, ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"], range(50))
    plug_in = b.inference(test_docs)                      # (held-out stream 0 of b)
    first = a.document_completion(test_docs)              # (held-out stream 0 of a)
    assert a._heldout_calls == 1 and first[1] > 0 and np.isfinite(first[0]) and first[2].shape == (50, 10)
    a._heldout_calls = 0
    assert a.inference(test_docs)[0] == plug_in[0]        # the plug-in path is untouched by the call before it
    second = b.document_completion(test_docs)             # (stream 1 of b: another chain)
    assert second[0] != first[0]
    b._heldout_calls = 0
    same = b.document_completion(test_docs)
    assert same[0] == first[0] and same[1] == first[1] and np.array_equal(same[2], first[2])


def _gibbs_engine(ap_train, sweeps=3):
    from pylda_amd.monte_carlo import MonteCarlo
    words = [str(w) for w in ap_train["words"]]
    m = MonteCarlo(hyper_parameter_optimize_interval=1000, seed=21, blocks=16)
    m._verbose = False
    m._initialize(_documents(words, ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300)), words, 10, 0.1,
                  1.0 / len(words))
    for _ in range(sweeps):
        m.learning()
    return m, words


def test_monte_carlo_against_the_fold_in_restatement(ap_train):
    from pylda_amd.corpus import split_for_completion
    from pylda_amd.hybrid import _grouped_csr
    from pylda_amd.monte_carlo import FOLD_IN_STREAM_BASE
    m, words = _gibbs_engine(ap_train)
    heldout = _documents(words, ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(300, 340))
    before = m._counts(True, True)
    blob = pickle.dumps(m)
    plug_in = m.fold_in(heldout, 6, 3)                                        # (fold-in stream 0)
    ll, tokens, gamma = m.document_completion(heldout + ["not-a-word"], 6, 3)  # (fold-in stream 1)
    assert m._fold_in_calls == 2 and gamma.shape == (40, 10)
    assert all(np.array_equal(x, y) for x, y in zip(m._counts(True, True), before))
    observed_csr, held_csr = split_for_completion(*_grouped_csr(m.parse_data(heldout)))
    n_kv, n_k, _ = before
    P = foldin_spec.predictive_table(n_kv, n_k, m._alpha_beta, float(np.sum(m._alpha_beta)))
    want_fold = foldin_spec.fold_in(*observed_csr, P, m._alpha_alpha, m._sampler_seed, FOLD_IN_STREAM_BASE + 1, 6, 3)
    assert np.array_equal(gamma, want_fold["gamma"])
    want = spec.score(*held_csr, P, gamma)
    assert tokens == int(want[1].sum())
    bar = spec.bar(len(words), 10, want[1], want[2], want[0])
    want_total = math.fsum(want[0].tolist())
    print("collapsed Gibbs: %.6f per held token, plug-in %.6f per token" % (ll / tokens, plug_in[0] / (2 * tokens)))
    assert abs(ll - want_total) <= float(bar.sum()) + len(bar) * 2.0 ** -53 * abs(want_total)
    # fold_in() keeps its results apart from the documented stream counter, on a restored snapshot too
    restored = pickle.loads(blob)
    assert restored.fold_in(heldout, 6, 3)[0] == plug_in[0]
    got = restored.document_completion(heldout, 6, 3)
    assert got[0] == ll and got[1] == tokens and np.array_equal(got[2], gamma)
    m._fold_in_calls = 0
    again = m.fold_in(heldout, 6, 3)
    assert again[0] == plug_in[0] and np.array_equal(again[1], plug_in[1])


def test_error_codes():
    from pylda_amd import _capi
    csr = _stack([([1, 2], [1, 2]), ([3], [1])])
    short = _stack([([1, 2], [1, 2])])
    K, V = 4, 6
    gamma = np.full((2, K), 0.5)
    ctx, other = _capi.Context(K, V), _capi.Context(K, V)
    try:
        held, observed, one, foreign = ctx.corpus(*csr), ctx.corpus(*csr), ctx.corpus(*short), other.corpus(*csr)

        def status(*args, **kwargs):
            with pytest.raises(_capi.PyldaError) as e:
                ctx.completion_score(*args, **kwargs)
            assert len(str(e.value)) > len("pylda_hip error -1: "), "no message"
            return e.value.status
        with pytest.raises(_capi.PyldaError) as e:
            ctx.completion_set_model()                    # eta was never set
        assert e.value.status == -4 and "eta" in str(e.value)
        assert status(held, gamma=gamma) == -4            # no predictive table
        ctx.set_alpha(np.full(K, 0.1))
        ctx.set_eta(np.random.default_rng(1).gamma(1.0, 1.0, (K, V)))
        ctx.completion_set_model()
        assert status(held) == -1                         # neither
        assert status(held, observed=observed, gamma=gamma) == -1          # both
        assert status(held, observed=observed) == -4      # the observed corpus has had no E-step
        assert status(held, observed=foreign) == -1
        ctx.estep(one, 5, 1e-6, True)
        assert status(held, observed=one) == -1           # D differs
        for bad in (0.0, -1.0, np.inf, np.nan):
            wrong = gamma.copy()
            wrong[1] = bad
            assert status(held, gamma=wrong) == -1        # a row whose sum is not positive and finite
            with pytest.raises(_capi.PyldaError):
                ctx.get_doc_values(held)                  # ... leaves no results behind
        total, tokens = ctx.completion_score(held, gamma=gamma)
        assert np.isfinite(total) and tokens == 4
        ctx.estep(observed, 5, 1e-6, True)
        assert np.isfinite(ctx.completion_score(held, observed=observed)[0])
        ctx.gibbs_init(observed, 1)                       # a Gibbs training state: its gamma buffer holds n_dk
        assert status(held, observed=observed) == -4
        assert status(observed, gamma=gamma) == -4
        # fold-in's model replaces the table and serves the score; completion's replaces fold-in's
        ctx.foldin_set_model(np.full(V, 0.1), n_kv=np.ones((K, V), np.int32), n_k=np.full(K, V, np.int32))
        assert abs(ctx.completion_score(held, gamma=gamma)[0] - 4 * math.log(1.0 / V)) < 1e-12
        ctx.completion_set_model()
        with pytest.raises(_capi.PyldaError) as e:
            ctx.foldin(one, np.full(K, 0.1), 4, 2)
        assert e.value.status == -4
        for c in (held, observed, one, foreign):
            c.close()
    finally:
        ctx.close()
        other.close()
    wide = _capi.Context(1025, V)
    try:
        wide.set_eta(np.ones((1025, V)))
        with pytest.raises(_capi.PyldaError) as e:
            wide.completion_set_model()
        assert e.value.status == -1
        held = wide.corpus(*csr)
        with pytest.raises(_capi.PyldaError) as e:
            wide.completion_score(held, gamma=np.ones((2, 1025)))
        assert e.value.status == -1 and "1024" in str(e.value)
        held.close()
    finally:
        wide.close()


def _line(out):
    lines = [l for l in out.splitlines() if l.startswith("document-completion likelihood of snapshot")]
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
    heldout = _documents(words, ptr, ids, cts, range(300, 330))
    (source / "train.dat").write_text("\n".join(_documents(words, ptr, ids, cts, range(120))) + "\n")
    (source / "test.dat").write_text("\n".join(heldout + ["not-a-word"]) + "\n")
    (source / "voc.dat").write_text("\n".join(words) + "\n")
    held_tokens = sum(len(d.split()) // 2 for d in heldout)
    K = 5
    common = ["--input_directory=%s" % source, "--number_of_topics=%d" % K, "--training_iterations=2", "--snapshot_interval=2"]

    def trained(name, *flags):
        assert cli.train_main(common + ["--output_directory=%s" % (tmp_path / name)] + list(flags)) == 0
        return tmp_path / name / "ap120" / os.listdir(tmp_path / name / "ap120")[0]
    # a mode-2 snapshot: without the flag the plug-in line and inference()'s gamma, with it the completion line
    vb = trained("vb")
    capsys.readouterr()
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % vb]) == 0
    out = capsys.readouterr().out
    assert "document-completion" not in out
    assert len([l for l in out.splitlines() if l.startswith("held-out likelihood of snapshot")]) == 1
    with open(vb / "model-2", "rb") as stream:
        engine = pickle.load(stream)
    engine._verbose = False
    plug_in = engine.inference(heldout)
    assert ("is %g" % plug_in[0]) in out and np.allclose(np.loadtxt(vb / "test-2"), plug_in[1], rtol=1e-15, atol=0)
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % vb, "--document_completion=1"]) == 0
    out = capsys.readouterr().out
    ll, tokens = _line(out)
    assert tokens == held_tokens and ll < 0 and "held-out likelihood of snapshot" not in out
    want = engine.document_completion(heldout)
    assert ("is %g" % want[0]) in out and np.allclose(np.loadtxt(vb / "test-2"), want[2], rtol=1e-15, atol=0)
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % vb, "--document_completion=1",
                          "--fold_in_samples=8"]) == 2
    assert "fold_in" in capsys.readouterr().err
    # a mode-1 snapshot still needs the fold-in's sweeps
    gibbs = trained("gibbs", "--inference_mode=1", "--sampler_seed=3", "--gibbs_blocks=8")
    capsys.readouterr()
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % gibbs, "--document_completion=1"]) == 2
    captured = capsys.readouterr()
    assert "--fold_in_samples" in captured.err and "document-completion likelihood" not in captured.out
    assert not (gibbs / "test-2").exists()
    assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % gibbs, "--document_completion=1",
                          "--fold_in_samples=8"]) == 0
    ll, tokens = _line(capsys.readouterr().out)
    assert tokens == held_tokens and ll < 0
    gamma = np.loadtxt(gibbs / "test-2")
    assert gamma.shape == (30, K) and np.all(gamma > 0)
    # ... and the hybrid and the online engine's snapshots answer the flag as a mode-2 snapshot does
    for name, flags in (("hybrid", ["--inference_mode=0", "--sampler_seed=1"]), ("online", ["--online_batches=4"])):
        run = trained(name, *flags)
        capsys.readouterr()
        assert cli.test_main(["--input_directory=%s" % source, "--model_directory=%s" % run, "--document_completion=1"]) == 0
        ll, tokens = _line(capsys.readouterr().out)
        assert tokens == held_tokens and ll < 0

"""The collapsed Gibbs engine on the GPU (pylda_gibbs_*, estep_gibbs.h) against its numpy restatement
(tests/gibbs_restatement.py) token for token, and the MonteCarlo class / mode-1 command line built on it."""
import os
import pickle

import numpy as np
import pytest

import gibbs_golden_checks as checks
import gibbs_restatement as spec
from conftest import load_golden, rel_err
from posterior_cases import corpus_of_counts as _corpus_of_counts

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


def _case(name, ap_train):
    """(K, V, csr, alpha, beta, blocks)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("ap_k10"):
        g = ap_train
        K, V, csr = 10, len(g["words"]), (g["doc_ptr"], g["term_id"], g["term_ct"])
        return K, V, csr, np.full(K, 1.0 / K), np.full(V, 1.0 / V), int(name.split("_b")[1])
    if name in ("k128", "k256"):
        K, V, blocks = int(name[1:]), 3000, 8
        csr = _synthetic(300, V, 5, 120, K)
    elif name in ("k400", "k700"):           # 8 and 16 topics per lane
        K, V, blocks = int(name[1:]), 2000, 5
        csr = _synthetic(80, V, 5, 60, 7)
    elif name == "long_document":
        K, V, blocks = 32, 4000, 2
        csr = _synthetic(3, V, 3000, 3000, 5, max_count=3)
    else:                                   # one term repeated 300 times, beside ordinary documents
        K, V, blocks = 16, 500, 3
        ptr, ids, cts = _synthetic(40, V, 3, 30, 9)
        csr = (np.concatenate([ptr, [ptr[-1] + 1]]), np.concatenate([ids, [17]]).astype(np.int32),
               np.concatenate([cts, [300]]).astype(np.int32))
    return K, V, csr, rng.uniform(0.02, 0.5, K), rng.uniform(0.005, 0.2, V), blocks      # vector alpha, vector beta


def _device_state(ctx, corpus):
    n_kv, n_k, topics = ctx.gibbs_get_counts(corpus)
    return np.array(ctx.get_gamma(corpus)), n_kv, n_k, topics


def _assert_equal_state(ctx, corpus, chain, what):
    n_dk, n_kv, n_k, topics = _device_state(ctx, corpus)
    assert np.array_equal(topics, chain.topics()), "%s: %d of %d topics differ" % (what, int(np.sum(topics != chain.topics())), topics.size)
    assert np.array_equal(n_kv, chain.n_kv()), what
    assert np.array_equal(n_k, chain.n_k[0]), what
    assert np.array_equal(n_dk, chain.n_dk.astype(np.float64)), what


@pytest.mark.parametrize("name", ["ap_k10_b1", "ap_k10_b16", "ap_k10_b2000", "k128", "k256", "k400", "k700", "long_document",
                                  "repeated_term"])
def test_kernel_equals_the_restatement_on_every_token(name, ap_train):
    from pylda_amd import _capi
    K, V, csr, alpha, beta, blocks = _case(name, ap_train)
    seed = 1234 + len(name)
    chain = spec.GibbsChain(*csr, K, V, seed=seed)
    chain.init()
    ctx = _capi.Context(K, V)
    try:
        corpus = ctx.corpus(*csr)
        ctx.gibbs_init(corpus, seed)
        _assert_equal_state(ctx, corpus, chain, "initial assignment")
        for sweep in range(1, 6):
            ctx.gibbs_sweep(corpus, alpha, beta, blocks, seed, sweep)
            chain.sweep(alpha, beta, blocks, sweep)
            if sweep in (1, 2, 5):
                _assert_equal_state(ctx, corpus, chain, "sweep %d" % sweep)
        corpus.close()
    finally:
        ctx.close()


def test_two_shards_draw_what_the_whole_corpus_draws(ap_train):
    """Two corpora holding two contiguous halves, given their offsets and the whole corpus' table and n_k: after one round
    their topics are the single-corpus run's and their table changes add up to its change."""
    from pylda_amd import _capi
    ptr, ids, cts = checks.first_documents(ap_train, 400)
    K, V, seed = 10, len(ap_train["words"]), 77
    alpha, beta = np.full(K, 0.1), np.full(V, 0.01)
    cut_doc = 170
    cut = int(ptr[cut_doc])
    halves = [(ptr[:cut_doc + 1], ids[:cut], cts[:cut], 0), (ptr[cut_doc:] - cut, ids[cut:], cts[cut:], cut_doc)]
    ctx = _capi.Context(K, V)
    try:
        whole = ctx.corpus(ptr, ids, cts)
        ctx.gibbs_init(whole, seed)
        before_kv, before_k, before_topics = ctx.gibbs_get_counts(whole)
        ctx.gibbs_sweep(whole, alpha, beta, 1, seed, 1)
        after_kv, after_k, after_topics = ctx.gibbs_get_counts(whole)
        assert not np.array_equal(before_topics, after_topics)
        change_kv, change_k, topics = np.zeros_like(after_kv), np.zeros_like(after_k), []
        for p, i, c, first in halves:
            shard = ctx.corpus(p, i, c)
            ctx.gibbs_init(shard, seed, first)
            ctx.gibbs_set_state(shard, n_kv=before_kv, n_k=before_k)
            ctx.gibbs_sweep(shard, alpha, beta, 1, seed, 1, first)
            kv, k, t = ctx.gibbs_get_counts(shard)
            change_kv += kv - before_kv
            change_k += k - before_k
            topics.append(t)
            shard.close()
        assert np.array_equal(np.concatenate(topics), after_topics)
        assert np.array_equal(change_kv, after_kv - before_kv) and np.array_equal(change_k, after_k - before_k)
        whole.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["A", "B"])
def test_device_log_posterior_matches_the_reference(name):
    from pylda_amd import _capi
    g = load_golden("gibbs_posterior.npz")
    n_dk, n_kv = g[name + "_n_dk"].astype(np.int64), g[name + "_n_kv"].astype(np.int64)
    K, V = n_kv.shape
    csr, topics = _corpus_of_counts(n_dk, n_kv)
    ctx = _capi.Context(K, V)
    try:
        corpus = ctx.corpus(*csr)
        ctx.gibbs_set_state(corpus, n_kv, n_kv.sum(axis=1), topics)
        assert np.array_equal(np.array(ctx.get_gamma(corpus)), n_dk.astype(np.float64))
        lp = ctx.gibbs_log_posterior(corpus, g[name + "_alpha"], g[name + "_beta"])
        flat = ctx.gibbs_log_posterior(corpus, np.full(K, 1.0 / K), np.full(V, 1.0 / V))
        print("log posterior %s: device %.17g, reference %.17g" % (name, lp, float(g[name + "_lp"])))
        assert rel_err(lp, g[name + "_lp"]) < 1e-10 and rel_err(flat, g[name + "_lp_flat"]) < 1e-10
        assert ctx.gibbs_log_posterior(corpus, g[name + "_alpha"], g[name + "_beta"]) == lp       # the same bits
        corpus.close()
    finally:
        ctx.close()


def _ap_text(ap_train, n):
    words = [str(w) for w in ap_train["words"]]
    ptr, ids, cts = checks.first_documents(ap_train, n)
    docs = [" ".join(" ".join([words[t]] * int(c)) for t, c in zip(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]]))
            for d in range(n)]
    return docs, words


def _engine(ap_train, interval, seed=100, blocks=64):
    from pylda_amd.monte_carlo import MonteCarlo
    docs, words = _ap_text(ap_train, 300)
    m = MonteCarlo(hyper_parameter_optimize_interval=interval, seed=seed, blocks=blocks)
    m._verbose = False
    m._initialize(docs, words, 10, 0.1, 1.0 / len(words))
    return m


def _check_invariants(m, ap_train):
    ptr, ids, cts = checks.first_documents(ap_train, 300)
    n_kv, n_dk, n_k = m._n_kv, m._n_dk, m._n_k
    assert np.array_equal(n_kv.sum(axis=0), np.bincount(ids, weights=cts, minlength=n_kv.shape[1]))
    assert np.array_equal(n_dk.sum(axis=1), np.add.reduceat(cts, ptr[:-1])) and np.array_equal(n_k, n_kv.sum(axis=1))
    assert n_kv.min() >= 0 and n_dk.min() >= 0
    topics = m._k_dn
    assert sum(len(t) for t in topics.values()) == int(cts.sum())
    assert np.array_equal(np.bincount(np.concatenate([topics[d] for d in range(300)]), minlength=10), n_k)


def test_learning_follows_the_reference_trace_and_survives_a_pickle(ap_train):
    lo, hi = checks.trace_band(load_golden("gibbs_trace_k10.npz"))
    m = _engine(ap_train, interval=1000)
    trace, resumed = [], None
    for it in range(1, 61):
        trace.append(m.learning())
        if it == 30:
            blob = pickle.dumps(m)
            assert b"Context" not in blob
            resumed = pickle.loads(blob)
            assert resumed._ctx is None and resumed._counter == 30
    _check_invariants(m, ap_train)
    s = checks.trace_statistic(np.array(trace))
    print("S of MonteCarlo.learning(), 64 blocks: %.0f; band [%.0f, %.0f]" % (s, lo, hi))
    assert lo <= s <= hi
    again = [resumed.learning() for _ in range(10)]
    assert again == trace[30:40]                                  # bit for bit
    assert m.log_posterior(m._alpha_alpha, m._alpha_beta) == trace[-1]


def test_hyper_parameter_step_on_the_device_state_equals_the_host_routine(ap_train):
    from pylda_amd.monte_carlo import slice_sample_hyperparameters
    m = _engine(ap_train, interval=10, blocks=16)
    steps = []
    inner = m.optimize_hyperparameters

    def checked():
        n_dk, n_kv = m._n_dk.astype(np.int64), m._n_kv.astype(np.int64)
        alpha, beta, rng = m._alpha_alpha.copy(), m._alpha_beta.copy(), np.random.get_state()
        inner()
        after = np.random.get_state()
        np.random.set_state(rng)
        want = slice_sample_hyperparameters(lambda a, b: spec.log_posterior(n_dk, n_kv, a, b), alpha, beta)
        np.random.set_state(after)
        assert np.array_equal(m._alpha_alpha, want[0]) and np.array_equal(m._alpha_beta, want[1])
        steps.append(not np.array_equal(m._alpha_alpha, alpha))
    m.optimize_hyperparameters = checked
    np.random.seed(0)
    for _ in range(30):
        lp = m.learning()
        assert np.isfinite(lp)
        assert np.all(np.isfinite(m._alpha_alpha)) and np.all(m._alpha_alpha > 0)
        assert np.all(np.isfinite(m._alpha_beta)) and np.all(m._alpha_beta > 0)
    assert len(steps) == 3 and any(steps)
    _check_invariants(m, ap_train)


def test_exports_and_the_mode_1_command_line(ap_train, tmp_path):
    from pylda_amd import cli
    docs, words = _ap_text(ap_train, 120)
    source = tmp_path / "in" / "ap120"
    source.mkdir(parents=True)
    (source / "train.dat").write_text("\n".join(docs) + "\n")
    (source / "voc.dat").write_text("\n".join(words) + "\n")
    K = 5
    assert cli.train_main(["--input_directory=%s" % source, "--output_directory=%s" % (tmp_path / "out"), "--number_of_topics=%d" % K,
                           "--training_iterations=6", "--snapshot_interval=3", "--inference_mode=1", "--sampler_seed=3",
                           "--gibbs_blocks=8"]) == 0
    runs = os.listdir(tmp_path / "out" / "ap120")
    assert len(runs) == 1 and runs[0].endswith("-im1")
    run = tmp_path / "out" / "ap120" / runs[0]
    for name in ("option.txt", "exp_beta-3", "exp_gamma-3", "exp_beta-6", "exp_gamma-6", "model-6"):
        assert (run / name).exists(), name
    options = dict(line.strip().split("=", 1) for line in open(run / "option.txt"))
    assert options["sampler_seed"] == "3" and options["gibbs_blocks"] == "8" and options["inference_mode"] == "1"
    lines = open(run / "exp_beta-6").read().splitlines()
    V = len(set(words))
    assert len(lines) == K * (V + 1)
    for k in range(K):
        block = lines[k * (V + 1):(k + 1) * (V + 1)]
        assert block[0] == "==========\t%d\t==========" % k
        p = np.array([float(l.split("\t")[1]) for l in block[1:]])
        assert abs(p.sum() - 1.0) < 1e-3 and np.all(np.diff(p) <= 0)
    gamma_lines = open(run / "exp_gamma-6").read().splitlines()
    assert len(gamma_lines) == 120 and all(len(l.split("\t")) == K for l in gamma_lines)
    with open(run / "model-6", "rb") as fh:
        model = pickle.load(fh)
    assert model._counter == 6 and model._ctx is None
    with pytest.raises(NotImplementedError):
        model.inference(docs[:2])
    assert np.isfinite(model.learning())                          # a snapshot trains on

"""Online variational Bayes on the device (pylda_amd/online_vb.py, mstep_online_eta_kernel) against the numpy
restatement of tests/online_vb_restatement.py.  Needs an MI355X.

The blend is compared bit for bit: its five roundings are numpy's.  Traces are held to the bars
test_learning_trace_matches_reference (tests/test_gpu_variational_bayes.py) holds for the same E-step against the same
oracle: 1e-8 relative on the objective and on eta."""
import os
import pickle

import numpy as np
import pytest

import online_vb_restatement as spec
from conftest import rel_err

pytestmark = pytest.mark.gpu

HELDOUT_FIVE_FULL_BATCH_ITERATIONS = -2182720.73      # C oracle, alpha fixed
HELDOUT_ONE_ONLINE_EPOCH = -2177490.2286              # C oracle: B = 8, tau0 = 1, kappa = 0.7


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    _capi.load()
    assert _capi.device_count() >= 1, "no HIP device visible"
    return _capi


def documents_from_csr(words, ptr, ids, cts):
    docs = []
    for d in range(len(ptr) - 1):
        toks = []
        for n in range(int(ptr[d]), int(ptr[d + 1])):
            toks += [str(words[ids[n]])] * int(cts[n])
        docs.append(" ".join(toks))
    return docs


def first_documents(g, D):
    ptr = g["doc_ptr"][:D + 1]
    return ptr, g["term_id"][:ptr[-1]], g["term_ct"][:ptr[-1]]


def online_engine(csr, V, K, alpha, beta, eta, batches, tau0=1.0, kappa=0.7):
    from pylda_amd.online_vb import OnlineVariationalBayes
    m = OnlineVariationalBayes(batches, tau0=tau0, kappa=kappa)
    m._verbose = False
    m._initialize_parsed(csr[0], csr[1], csr[2], V, K, alpha, beta, eta=np.array(eta))
    return m


# ---- 1. the blend kernel, bit for bit ----
@pytest.mark.parametrize("K,V", [(1, 1), (10, 33), (31, 32), (33, 31), (64, 1000), (129, 65), (700, 40), (1024, 33)])
def test_blend_kernel_bit_for_bit(capi, K, V):
    rng = np.random.default_rng(K * 10007 + V)
    eta = rng.gamma(100.0, 0.01, (K, V))
    sstats = rng.gamma(0.5, 20.0, (K, V))
    beta = rng.uniform(0.3, 0.65, V)
    ctx = capi.Context(K, V)
    assert ctx.sstats_elements() // V >= K
    ctx.set_alpha(np.full(K, 0.5))
    ctx.set_eta(eta)
    corpus = ctx.corpus(np.array([0, 1], np.int64), np.array([V - 1], np.int32), np.array([3], np.int32))
    ctx.estep(corpus)
    ctx.set_sstats(sstats)
    batch_topic_ll, batch_alpha_ss = ctx.mstep(corpus, beta)
    batch_eta = np.array(ctx.get_eta())
    assert np.array_equal(batch_eta, sstats + beta)
    for rho in (1.0, 0.37, 2.0 ** -10):
        for scale in (1.0, 7.0, 2000 / 250):
            ctx.set_eta(eta)
            topic_ll, alpha_ss = ctx.mstep_online(corpus, beta, rho, scale)
            got = np.array(ctx.get_eta())
            omr = 1.0 - rho
            want = omr * eta + rho * (scale * sstats + beta)
            assert np.array_equal(got, want), (rho, scale, np.max(np.abs(got - want)))
            assert topic_ll == batch_topic_ll and np.array_equal(alpha_ss, batch_alpha_ss)
            if rho == 1.0 and scale == 1.0:
                assert np.array_equal(got, batch_eta)
    # in place: a second step blends into the first one's result
    first = np.array(ctx.get_eta())
    ctx.mstep_online(None, beta, 0.25, 3.0, want_alpha_ss=False)
    assert np.array_equal(np.array(ctx.get_eta()), 0.75 * first + 0.25 * (3.0 * sstats + beta))
    corpus.close()
    ctx.close()


# ---- 2. the trace on the associated-press documents ----
@pytest.fixture(scope="module")
def ap800_restatement(ap_train):
    g = ap_train
    run = spec.OnlineRun(*first_documents(g, 800), g["alpha"], g["beta"], g["eta"], 4)
    trace = []
    for _ in range(8):
        objective = run.step()
        trace.append((objective, run.eta.copy()))
    return trace, run.gamma.copy()


def test_trace_matches_the_restatement(ap_train, ap800_restatement):
    """First 800 associated-press documents, K = 10, B = 4, two epochs (every minibatch's corpus is visited again with
    its postings built).  Bars: 1e-8 relative on the objective of every step and on eta after steps 1, 4 and 8.
    Measured on an MI355X: objective 3.8e-14 at most, eta 2.5e-10 at most, gamma after the eight steps 2.1e-10."""
    g = ap_train
    trace, gamma = ap800_restatement
    m = online_engine(first_documents(g, 800), 6806, 10, g["alpha"], g["beta"], g["eta"], 4)
    worst_objective = worst_eta = 0.0
    for step, (want, want_eta) in enumerate(trace, 1):
        got = m.learning()
        worst_objective = max(worst_objective, abs(got - want) / abs(want))
        if step in (1, 4, 8):
            worst_eta = max(worst_eta, rel_err(m._eta, want_eta))
    print("online trace, 8 steps: objective %.2e, eta %.2e, gamma %.2e" % (worst_objective, worst_eta, rel_err(m._gamma, gamma)))
    assert worst_objective < 1e-8
    assert worst_eta < 1e-8
    assert m._counter == 8 and m._gamma.shape == (800, 10)
    assert rel_err(m._gamma, gamma) < 1e-7
    assert np.array_equal(m._alpha_alpha, g["alpha"])               # alpha is fixed


# ---- 3. words a minibatch does not contain ----
def test_words_absent_from_a_minibatch():
    """Each minibatch lacks words the other has (and both lack 35 ... 39): their statistics must be exact zeros - not the
    previous minibatch's - so that their columns of eta move to omr * eta + rho * beta, bit for bit."""
    K, V, B = 3, 40, 2
    even, odd, shared = list(range(0, 20)), list(range(20, 30)), list(range(30, 35))
    rng = np.random.default_rng(3)
    ptr, ids, cts = [0], [], []
    for d in range(6):
        own = even if d % 2 == 0 else odd
        u = np.sort(np.concatenate([rng.choice(own, size=5, replace=False), rng.choice(shared, size=2, replace=False)]))
        ids.append(u)
        cts.append(rng.integers(1, 9, u.size))
        ptr.append(ptr[-1] + u.size)
    csr = (np.array(ptr, np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(cts).astype(np.int32))
    alpha, beta = np.full(K, 0.4), rng.uniform(0.02, 0.08, V)
    eta = rng.gamma(100.0, 0.01, (K, V))
    run = spec.OnlineRun(*csr, alpha, beta, eta, B)
    m = online_engine(csr, V, K, alpha, beta, eta, B)
    for step in range(4):
        before = np.array(m._eta)
        want = run.step()
        got = m.learning()
        rho, omr = run.last["rho"], 1.0 - run.last["rho"]
        present = np.unique(np.concatenate([csr[1][csr[0][d]:csr[0][d + 1]] for d in range(step % B, 6, B)]))
        absent = np.setdiff1d(np.arange(V), present)
        assert len(absent) >= 15 and set(range(35, 40)) <= set(absent.tolist())
        assert np.all(run.last["sstats"][:, absent] == 0.0)
        after = np.array(m._eta)
        assert np.array_equal(after[:, absent], omr * before[:, absent] + rho * beta[absent]), step
        assert abs(got - want) < 1e-9 * abs(want), (step, got, want)
        assert rel_err(after, run.eta) < 1e-9, step
    assert rel_err(m._gamma, run.gamma) < 1e-9


# ---- 4. the kernel families inside a minibatch ----
def topical_corpus(rng, lengths, V, K, topics_per_document=3):
    """Documents of the given numbers of distinct terms, drawn (but for one term in fifty) from three topics each, and a
    model that knows every topic: with a small alpha most of a document's K topics die within a dozen iterations (the
    live-topic kernel takes the document over), and the few left are told apart quickly.  That matters for the bar: a
    model whose topics are copies of each other leaves most documents undecided at the iteration cap, and the
    restatement ITSELF then moves by 2e-3 in eta within two steps when its start eta is perturbed by 1e-13 relative.  On
    these corpora the same perturbation moves the restatement's eta by 3.1e-10 at most over the six steps at K = 256 and
    1.5e-10 at K = 700 (the associated-press trace: 1.6e-10 over 16 steps), which is what leaves room under 1e-8."""
    topics = rng.dirichlet(np.full(V, 0.02), size=K)
    ptr, ids, cts = [0], [], []
    for n in lengths:
        mine = rng.choice(K, size=topics_per_document, replace=False)
        theta = np.zeros(K)
        theta[mine] = rng.dirichlet(np.full(topics_per_document, 1.0))
        u = np.sort(rng.choice(V, size=int(n), replace=False, p=0.98 * (theta @ topics) + 0.02 / V))
        ids.append(u.astype(np.int32))
        cts.append((1 + rng.poisson(1.0, u.size)).astype(np.int32))
        ptr.append(ptr[-1] + len(u))
    eta = rng.gamma(100.0, 0.01, (K, V))
    for k in range(K):
        eta[k] += 40.0 * V * topics[k] * rng.uniform(0.2, 1.0)
    return (np.array(ptr, np.int64), np.concatenate(ids), np.concatenate(cts)), eta


@pytest.mark.parametrize("K,D,steps", [(128, 180, 6), (256, 180, 6), (700, 30, 6)])
def test_kernel_families_inside_a_minibatch(K, D, steps):
    """alpha = 0.01 and documents of 1 ... 300 distinct terms: at K = 128 and 256 the dense quad kernels hand documents to the
    live-topic kernel and the statistics pass reads their lists of live topics; K = 700 runs the fused streaming kernel.
    B = 3, two epochs.  Measured on an MI355X (objective at most, eta after six steps): K = 128
    3.0e-13 and 3.2e-12, K = 256 4.6e-13 and 2.7e-9, K = 700 7.3e-12 and 6.9e-11."""
    V = 3000
    rng = np.random.default_rng(K)
    lengths = rng.permutation(np.linspace(1, 300, D).astype(np.int64))
    csr, eta = topical_corpus(rng, lengths, V, K)
    assert np.diff(csr[0]).min() == 1 and np.diff(csr[0]).max() == 300
    alpha, beta = np.full(K, 0.01), np.full(V, 1.0 / V)
    run = spec.OnlineRun(*csr, alpha, beta, eta, 3, e_step=spec.threaded_e_step)
    m = online_engine(csr, V, K, alpha, beta, eta, 3)
    worst = 0.0
    for step in range(steps):
        want = run.step()
        got = m.learning()
        worst = max(worst, abs(got - want) / abs(want))
    err = rel_err(m._eta, run.eta)
    print("K=%d: objective %.2e, eta %.2e" % (K, worst, err))
    if K <= 256:
        assert all(m._batch_corpora[b].layout("gather_live") == 1 for b in range(3))
    assert err < 1e-8
    assert worst < 1e-8


def test_one_document_per_minibatch():
    K, V, D = 128, 3000, 5
    rng = np.random.default_rng(5)
    csr, eta = topical_corpus(rng, [1, 40, 300, 7, 120], V, K)
    alpha, beta = np.full(K, 0.01), np.full(V, 1.0 / V)
    run = spec.OnlineRun(*csr, alpha, beta, eta, D)
    m = online_engine(csr, V, K, alpha, beta, eta, D)
    for step in range(7):
        want = run.step()
        got = m.learning()
        assert run.last["scale"] == 5.0
        assert abs(got - want) < 1e-8 * abs(want), step
    assert rel_err(m._eta, run.eta) < 1e-8
    assert rel_err(m._gamma, run.gamma) < 1e-7
    from pylda_amd.online_vb import OnlineVariationalBayes
    too_many = OnlineVariationalBayes(D + 1)
    too_many._verbose = False
    with pytest.raises(ValueError):
        too_many._initialize_parsed(csr[0], csr[1], csr[2], V, K, alpha, beta, eta=eta.copy())


# ---- 5. one minibatch with tau0 = 1 is the batch iteration ----
def test_one_batch_first_step_is_the_batch_iteration(ap_train):
    from pylda_amd.variational_bayes import VariationalBayes
    g = ap_train
    csr = first_documents(g, 300)
    online = online_engine(csr, 6806, 10, g["alpha"], g["beta"], g["eta"], 1, tau0=1.0)
    batch = VariationalBayes(hyper_parameter_optimize_interval=10 ** 9)       # alpha never updates
    batch._verbose = False
    batch._initialize_parsed(csr[0], csr[1], csr[2], 6806, 10, g["alpha"], g["beta"], eta=g["eta"].copy())
    got, want = online.learning(), batch.learning()
    assert got == want
    assert np.array_equal(online._eta, batch._eta)
    assert np.array_equal(online._gamma, batch._gamma)
    assert np.array_equal(batch._alpha_alpha, g["alpha"])
    # ... the second one is not: rho_1 = 2 ** -0.7
    online.learning()
    batch.learning()
    assert not np.array_equal(online._eta, batch._eta)


# ---- 6. a snapshot in the middle of an epoch ----
def test_pickle_in_the_middle_of_an_epoch(ap_train):
    g = ap_train
    D, K, B = 302, 10, 4
    csr = first_documents(g, D)
    whole = online_engine(csr, 6806, K, g["alpha"], g["beta"], g["eta"], B)
    initial = np.zeros((D, K)) + g["alpha"][np.newaxis, :] + 6806.0 / K
    assert np.array_equal(whole._gamma, initial)
    for _ in range(2):
        whole.learning()
    gamma = np.array(whole._gamma)
    assert gamma.shape == (D, K)
    for b in (0, 1):                                               # visited: the minibatch's gamma, in document order
        assert np.array_equal(gamma[b::B], whole._ctx.get_gamma(whole._batch_corpora[b]))
        assert not np.any(gamma[b::B] == initial[b::B])
    for b in (2, 3):                                               # not visited yet: the initial value
        assert np.array_equal(gamma[b::B], initial[b::B])
    for _ in range(6):
        whole.learning()

    halved = online_engine(csr, 6806, K, g["alpha"], g["beta"], g["eta"], B)
    for _ in range(5):
        halved.learning()
    blob = pickle.dumps(halved)
    del halved
    restored = pickle.loads(blob)
    assert restored._ctx is None and restored._train_corpus is None and restored._batch_corpora == {}
    assert (restored._batches, restored._tau0, restored._kappa, restored._counter) == (B, 1.0, 0.7, 5)
    assert restored._gamma.shape == (D, K)
    for _ in range(3):
        restored.learning()
    assert restored._counter == whole._counter == 8
    assert np.array_equal(restored._eta, whole._eta)
    assert np.array_equal(restored._gamma, whole._gamma)
    for b in range(B):
        assert np.array_equal(whole._gamma[b::B], whole._ctx.get_gamma(whole._batch_corpora[b]))


# ---- 7. held-out documents ----
def test_inference_is_the_base_class(ap_train, ap_test):
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    g, h = ap_train, ap_test
    words = [str(w) for w in g["words"]]
    train_docs = documents_from_csr(words, *first_documents(g, 100))
    test_docs = documents_from_csr(words, h["doc_ptr"], h["term_id"], h["term_ct"])
    np.random.seed(0)
    online = OnlineVariationalBayes(4)
    online._verbose = False
    online._initialize(train_docs, words, 10, 0.1, 1.0 / len(words))
    online._alpha_alpha = g["alpha"].copy()
    online._eta = g["eta"].copy()
    for _ in range(3):
        online.learning()
    batch = VariationalBayes()
    batch._verbose = False
    batch._initialize(train_docs, words, 10, 0.1, 1.0 / len(words))
    batch._alpha_alpha = online._alpha_alpha.copy()
    batch._eta = np.array(online._eta)
    gamma_before = np.array(online._gamma)
    got_ll, got_gamma = online.inference(test_docs)
    want_ll, want_gamma = batch.inference(test_docs)
    assert got_gamma.shape == (221, 10)
    assert got_ll == want_ll and np.array_equal(got_gamma, want_gamma)
    assert np.array_equal(online._gamma, gamma_before)              # held-out mode leaves _gamma alone
    online.learning()                                               # ... and the run goes on
    assert online._counter == 4


# ---- 8. the claim of DESIGN.md section 14, on the device ----
def test_one_online_epoch_beats_five_full_batch_iterations(ap_train, ap_test):
    """Measured on an MI355X: one online epoch -2177490.2286 (7.5e-12 relative from the C oracle's figure), five full-batch
    iterations -2182720.7301."""
    from pylda_amd.variational_bayes import VariationalBayes
    g, h = ap_train, ap_test
    csr = (g["doc_ptr"], g["term_id"], g["term_ct"])
    test = (h["doc_ptr"], h["term_id"], h["term_ct"])
    online = online_engine(csr, 6806, 10, g["alpha"], g["beta"], g["eta"], 8)
    for _ in range(8):
        online.learning()
    online_ll, _ = online.e_step(test)
    batch = VariationalBayes(hyper_parameter_optimize_interval=10 ** 9)
    batch._verbose = False
    batch._initialize_parsed(csr[0], csr[1], csr[2], 6806, 10, g["alpha"], g["beta"], eta=g["eta"].copy())
    for _ in range(5):
        batch.learning()
    batch_ll, _ = batch.e_step(test)
    print("held-out words log-likelihood: one online epoch %.4f (%.1e from the oracle's), five full-batch iterations %.4f"
          % (online_ll, abs(online_ll - HELDOUT_ONE_ONLINE_EPOCH) / abs(HELDOUT_ONE_ONLINE_EPOCH), batch_ll))
    assert np.array_equal(batch._alpha_alpha, g["alpha"])
    assert online_ll > batch_ll
    assert online_ll > HELDOUT_FIVE_FULL_BATCH_ITERATIONS
    assert abs(online_ll - HELDOUT_ONE_ONLINE_EPOCH) < 1e-8 * abs(HELDOUT_ONE_ONLINE_EPOCH)


# ---- 9. error codes and the command line ----
def test_error_codes(capi):
    K, V = 5, 12
    rng = np.random.default_rng(9)
    beta = np.full(V, 0.1)
    ctx = capi.Context(K, V)

    def status(call, *args, **kwargs):
        with pytest.raises(capi.PyldaError) as refused:
            call(*args, **kwargs)
        return refused.value.status

    INVALID, STATE = -1, -4
    # nothing on the device yet
    assert status(ctx.mstep_online, None, beta, 0.5, 2.0, want_alpha_ss=False) == STATE
    ctx.set_alpha(np.full(K, 0.2))
    ctx.set_eta(rng.gamma(100.0, 0.01, (K, V)))
    corpus = ctx.corpus(np.array([0, 2, 3], np.int64), np.array([1, 4, 7], np.int32), np.array([2, 1, 5], np.int32))
    assert status(ctx.mstep_online_enqueue, corpus, beta, 0.5, 2.0) == STATE         # no E-step on this corpus
    ctx.estep(corpus, 50, 1e-6, True)
    assert status(ctx.mstep_online_enqueue, corpus, beta, 0.5, 2.0) == STATE         # ... a held-out one
    ctx.estep(corpus)
    before = np.array(ctx.get_eta())
    for rho in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        assert status(ctx.mstep_online, corpus, beta, rho, 2.0) == INVALID, rho
        assert status(ctx.mstep_online_enqueue, corpus, beta, rho, 2.0) == INVALID, rho
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert status(ctx.mstep_online, corpus, beta, 0.5, scale) == INVALID, scale
        assert status(ctx.mstep_online_enqueue, corpus, beta, 0.5, scale) == INVALID, scale
    assert status(ctx.mstep_online, corpus, None, 0.5, 2.0) == INVALID
    assert status(ctx.mstep_online_enqueue, corpus, None, 0.5, 2.0) == INVALID
    assert status(ctx.mstep_online, None, beta, 0.5, 2.0, want_alpha_ss=True) == STATE      # alpha statistics of no corpus
    assert status(ctx.mstep_online_enqueue, None, beta, 0.5, 2.0) == STATE
    assert np.array_equal(np.array(ctx.get_eta()), before)          # a refused call changes nothing
    other = capi.Context(K, V)
    assert status(other.mstep_online_enqueue, corpus, beta, 0.5, 2.0) == STATE       # another context's corpus
    other.close()
    # ... and what is accepted: the enqueued form gives what the waited one gives
    sstats = np.array(ctx.get_sstats())
    topic_ll, alpha_ss = ctx.mstep_online(corpus, beta, 1.0, 1.0)
    assert np.array_equal(np.array(ctx.get_eta()), sstats + beta)
    ctx.set_eta(before)
    ctx.mstep_online_enqueue(corpus, beta, 1.0, 1.0)
    _, docs, _, topic_ll_enqueued, alpha_ss_enqueued, _ = ctx.outer_fetch()
    assert docs == 2 and topic_ll_enqueued == topic_ll and np.array_equal(alpha_ss_enqueued, alpha_ss)
    assert np.array_equal(np.array(ctx.get_eta()), sstats + beta)
    corpus.close()
    ctx.close()


def test_launch_train_and_launch_test_online(ap_train, tmp_path, capsys):
    from pylda_amd import launch_test, launch_train
    g = ap_train
    words = [str(w) for w in g["words"]]
    corpus_dir = tmp_path / "mini-press"
    corpus_dir.mkdir()
    docs = documents_from_csr(words, *first_documents(g, 60))
    (corpus_dir / "train.dat").write_text("\n".join(docs[:50]) + "\n")
    (corpus_dir / "test.dat").write_text("\n".join(docs[50:60]) + "\n")
    (corpus_dir / "voc.dat").write_text("".join("%s\t1\t1\n" % w for w in words))
    out_dir = tmp_path / "out"
    np.random.seed(3)
    base = ["--input_directory=%s/" % corpus_dir, "--output_directory=%s" % out_dir, "--number_of_topics=5"]
    rc = launch_train.main(base + ["--training_iterations=6", "--snapshot_interval=3", "--online_batches=4"])
    assert rc == 0
    printed = capsys.readouterr().out
    assert "online_batches=4" in printed and "e_step and m_step of iteration 6 finished" in printed
    runs = list((out_dir / "mini-press").iterdir())
    assert len(runs) == 1 and "-lda-I6-S3-K5-" in runs[0].name and runs[0].name.endswith("-im2")
    names = sorted(p.name for p in runs[0].iterdir())
    assert names == ["exp_beta-3", "exp_beta-6", "exp_gamma-3", "exp_gamma-6", "model-6", "option.txt"]
    opts = dict(l.split("=", 1) for l in (runs[0] / "option.txt").read_text().splitlines())
    assert opts["online_batches"] == "4" and opts["online_tau0"] == "1.0" and opts["online_kappa"] == "0.7"
    assert opts["inference_mode"] == "2"
    assert len((runs[0] / "exp_gamma-6").read_text().splitlines()) == 50
    with open(runs[0] / "model-6", "rb") as stream:
        engine = pickle.load(stream)
    assert type(engine).__name__ == "OnlineVariationalBayes" and engine._counter == 6 and engine._batches == 4
    rc = launch_test.main(["--input_directory=%s" % corpus_dir, "--model_directory=%s" % runs[0], "--snapshot_index=6"])
    assert rc == 0
    assert "held-out likelihood of snapshot" in capsys.readouterr().out
    gamma = np.loadtxt(runs[0] / "test-6")
    assert gamma.shape == (10, 5) and np.all(gamma > 0)
    # more minibatches than documents: refused, whether the lines or the parsed documents are too few
    assert launch_train.main(base + ["--training_iterations=1", "--online_batches=51"]) == 2
    assert "--online_batches" in capsys.readouterr().err
    # without the flag nothing of it shows
    rc = launch_train.main(base + ["--training_iterations=1", "--snapshot_interval=1"])
    assert rc == 0
    assert "online" not in capsys.readouterr().out
    plain = [p for p in (out_dir / "mini-press").iterdir() if "-lda-I1-" in p.name]
    assert len(plain) == 1 and "online" not in (plain[0] / "option.txt").read_text()
    assert os.path.exists(plain[0] / "model-1")

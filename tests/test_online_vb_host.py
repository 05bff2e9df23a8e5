"""Online variational Bayes without a GPU: the schedule and the dealing of pylda_amd/online_vb.py, the restatement
(tests/online_vb_restatement.py) against the batch M-step, the rehearsal that DESIGN.md section 14 quotes, and the command
line's refusals."""
import numpy as np
import pytest

import online_vb_restatement as spec
from oracle import c_oracle, vb_numpy


def test_step_sizes():
    from pylda_amd import online_vb
    for tau0, kappa, t, want in ((1.0, 0.7, 0, 1.0), (1.0, 1.0, 3, 0.25), (4.0, 1.0, 0, 0.25), (1.0, 0.75, 15, 0.125),
                                 (1023.0, 0.75, 1, 2.0 ** -7.5), (2.0, 0.7, 5, 7.0 ** -0.7)):
        assert online_vb.step_size(tau0, kappa, t) == want, (tau0, kappa, t)
        assert spec.step_size(tau0, kappa, t) == want
    rho = [online_vb.step_size(1.0, 0.7, t) for t in range(50)]
    assert rho[0] == 1.0 and all(a > b > 0.0 for a, b in zip(rho, rho[1:]))


def test_constructor_refuses_bad_arguments():
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    m = OnlineVariationalBayes(8)
    assert isinstance(m, VariationalBayes)
    assert (m._batches, m._tau0, m._kappa, m._device) == (8, 1.0, 0.7, 0)
    assert m._hyper_parameter_optimize_interval > 0
    for bad in (dict(batches=0), dict(batches=-3), dict(batches=4, tau0=0.5), dict(batches=4, tau0=float("nan")),
                dict(batches=4, tau0=float("inf")), dict(batches=4, kappa=0.5), dict(batches=4, kappa=1.01),
                dict(batches=4, kappa=float("nan"))):
        with pytest.raises(ValueError):
            OnlineVariationalBayes(**bad)
    OnlineVariationalBayes(1, tau0=1.0, kappa=1.0)
    with pytest.raises(NotImplementedError) as refused:
        OnlineVariationalBayes(4, process_group=object())
    assert "one GPU" in str(refused.value)


def test_dealing_of_the_documents():
    from pylda_amd import online_vb
    ptr = np.array([0, 2, 3, 3, 7, 8, 10, 11], np.int64)            # 7 documents, one of them empty
    ids = np.arange(11, dtype=np.int32)
    cts = np.arange(11, dtype=np.int32) + 1
    for B in (1, 2, 3, 7):
        seen = []
        for b in range(B):
            docs = online_vb.batch_documents(7, B, b)
            assert list(docs) == spec.batch_documents(7, B, b) == [d for d in range(7) if d % B == b]
            bp, bi, bc = online_vb.batch_csr(ptr, ids, cts, B, b)
            assert len(bp) == len(docs) + 1 and bp[0] == 0 and bp[-1] == len(bi) == len(bc)
            for n, d in enumerate(docs):
                assert np.array_equal(bi[bp[n]:bp[n + 1]], ids[ptr[d]:ptr[d + 1]])
                assert np.array_equal(bc[bp[n]:bp[n + 1]], cts[ptr[d]:ptr[d + 1]])
            seen += list(docs)
        assert sorted(seen) == list(range(7))
    # B = D: one document per minibatch; D not divisible by B: the minibatches' scales differ
    assert [len(online_vb.batch_documents(7, 7, b)) for b in range(7)] == [1] * 7
    sizes = [len(online_vb.batch_documents(7, 3, b)) for b in range(3)]
    assert sizes == [3, 2, 2] and 7.0 / sizes[0] != 7.0 / sizes[1]


def small_corpus(D=12, V=30, seed=0):
    rng = np.random.default_rng(seed)
    ptr, ids, cts = [0], [], []
    for _ in range(D):
        u = np.sort(rng.choice(V, size=rng.integers(1, 9), replace=False))
        ids.append(u)
        cts.append(rng.integers(1, 6, u.size))
        ptr.append(ptr[-1] + u.size)
    return np.array(ptr, np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(cts).astype(np.int32)


def test_one_batch_with_tau0_1_is_the_batch_m_step():
    """B = 1, tau0 = 1: rho_0 = 1, 1 - rho = +0, scale = 1 - the first step's eta is the batch M-step's, bit for bit."""
    ptr, ids, cts = small_corpus()
    K, V = 4, 30
    rng = np.random.default_rng(1)
    alpha, beta, eta = np.full(K, 0.25), rng.uniform(0.01, 0.1, V), rng.gamma(100.0, 0.01, (K, V))
    run = spec.OnlineRun(ptr, ids, cts, alpha, beta, eta, 1)
    objective = run.step()
    e = c_oracle.e_step(alpha, eta, ptr, ids, cts)
    topic_ll, _, new_eta = vb_numpy.m_step(eta, beta, e["sstats"], e["gamma"])
    assert run.last["rho"] == 1.0 and run.last["scale"] == 1.0
    assert np.array_equal(run.eta, new_eta)
    assert objective == e["document_log_likelihood"] + topic_ll
    assert np.array_equal(run.gamma, e["gamma"])
    # ... and the second step is a blend: between the old eta and the batch update, element by element
    before = run.eta.copy()
    run.step()
    target = run.last["sstats"] + beta
    assert run.last["rho"] == 2.0 ** -0.7
    assert np.all(run.eta <= np.maximum(before, target) * (1 + 1e-15))
    assert np.all(run.eta >= np.minimum(before, target) * (1 - 1e-15))


def test_scales_of_uneven_minibatches():
    ptr, ids, cts = small_corpus(D=7)
    K, V = 3, 30
    rng = np.random.default_rng(2)
    run = spec.OnlineRun(ptr, ids, cts, np.full(K, 0.3), np.full(V, 0.05), rng.gamma(100.0, 0.01, (K, V)), 3)
    scales = []
    for t in range(3):
        run.step()
        scales.append(run.last["scale"])
        assert run.last["batch"] == t
        # the statistics of a minibatch sum to its tokens: the blend moves eta's total by rho * (scale * tokens + sum beta)
        docs = spec.batch_documents(7, 3, t)
        tokens = sum(int(cts[ptr[d]:ptr[d + 1]].sum()) for d in docs)
        assert abs(run.last["sstats"].sum() - tokens) < 1e-9 * tokens
    assert scales == [7.0 / 3.0, 7.0 / 2.0, 7.0 / 2.0]
    initial = np.zeros(K) + 0.3 + 30.0 / 3                          # every document has been visited once
    assert not np.any(np.all(run.gamma == initial[np.newaxis, :], axis=1))


# What the C oracle gives for the associated-press fixture (2000 documents, K = 10) from ap_train_k10.npz's eta, alpha and
# beta, scored on ap_test_k10.npz: held-out words log-likelihood at the start, after five full-batch iterations with alpha
# fixed, and after ONE online epoch (B = 8, tau0 = 1, kappa = 0.7) - the table of DESIGN.md section 14.
HELDOUT_START = -2200522.24
HELDOUT_FIVE_FULL_BATCH_ITERATIONS = -2182720.73
HELDOUT_ONE_ONLINE_EPOCH = -2177490.2286


def test_one_online_epoch_beats_five_full_batch_iterations(ap_train, ap_test):
    g, h = ap_train, ap_test
    test = (h["doc_ptr"], h["term_id"], h["term_ct"])
    start = spec.heldout_words_log_likelihood(g["alpha"], g["eta"], *test)
    assert abs(start - HELDOUT_START) < 0.01
    run = spec.OnlineRun(g["doc_ptr"], g["term_id"], g["term_ct"], g["alpha"], g["beta"], g["eta"], 8)
    for _ in range(8):
        run.step()
    after = spec.heldout_words_log_likelihood(g["alpha"], run.eta, *test)
    print("held-out words log-likelihood after one online epoch: %.4f" % after)
    assert after > HELDOUT_FIVE_FULL_BATCH_ITERATIONS
    assert abs(after - HELDOUT_ONE_ONLINE_EPOCH) < 1e-9 * abs(HELDOUT_ONE_ONLINE_EPOCH)      # the C oracle is deterministic


def test_command_line_refusals(capsys, monkeypatch):
    from pylda_amd import cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--input_directory=in", "--output_directory=out", "--number_of_topics=3", "--training_iterations=1"]
    assert cli.train_main(base + ["--online_batches=4", "--inference_mode=0", "--sampler_seed=1"]) == 2
    err = capsys.readouterr().err
    assert "--online_batches" in err and "--inference_mode=2 only" in err
    assert cli.train_main(base + ["--online_batches=4", "--inference_mode=1", "--sampler_seed=1", "--gibbs_blocks=4"]) == 2
    assert "--inference_mode=2 only" in capsys.readouterr().err
    assert cli.train_main(base + ["--online_batches=4", "--gpus=2"]) == 2
    assert "one GPU" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert cli.train_main(base + ["--online_batches=4"]) == 2
    assert "one GPU" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE")
    assert cli.train_main(base + ["--online_batches=0"]) == 2
    assert "batches" in capsys.readouterr().err
    assert cli.train_main(base + ["--online_batches=4", "--online_kappa=0.5"]) == 2
    assert "kappa" in capsys.readouterr().err
    assert cli.train_main(base + ["--online_batches=4", "--online_tau0=0.5"]) == 2
    assert "tau0" in capsys.readouterr().err
    assert cli.train_main(base + ["--online_tau0=2"]) == 2
    assert "--online_batches=B" in capsys.readouterr().err
    opt = cli._parse(cli.TRAIN_FLAGS, base, "launch_train")
    assert (opt.online_batches, opt.online_tau0, opt.online_kappa) == (-1, -1, -1)
    opt = cli._parse(cli.TRAIN_FLAGS, base + ["--online_batches=16", "--online_tau0=64", "--online_kappa=0.6"], "launch_train")
    assert (opt.online_batches, opt.online_tau0, opt.online_kappa) == (16, 64.0, 0.6)

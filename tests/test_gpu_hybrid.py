"""The hybrid E-step on the GPU (pylda_hybrid_estep, estep_hybrid.h) against its numpy restatement
(tests/hybrid_restatement.py), and the Hybrid class / mode-0 command line built on it."""
import pickle

import numpy as np
import pytest

import hybrid_restatement as spec
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


def _case(name, ap_train):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "ap_k10":
        g = ap_train
        K, csr = 10, (g["doc_ptr"], g["term_id"], g["term_ct"])
        V = len(g["words"])
    elif name in ("k128", "k256"):
        K, V = int(name[1:]), 3000
        csr = _synthetic(300, V, 5, 120, K)
    elif name in ("k400", "k700"):           # 8 and 16 topics per lane
        K, V = int(name[1:]), 2000
        csr = _synthetic(80, V, 5, 60, 7)
    elif name == "long_document":
        K, V = 32, 4000
        csr = _synthetic(3, V, 3000, 3000, 5, max_count=3)
        assert csr[2][:csr[0][1]].sum() >= 5000
    else:                                   # one term repeated 300 times, beside ordinary documents
        K, V = 16, 500
        ptr, ids, cts = _synthetic(40, V, 3, 30, 9)
        csr = (np.concatenate([ptr, [ptr[-1] + 1]]), np.concatenate([ids, [17]]).astype(np.int32),
               np.concatenate([cts, [300]]).astype(np.int32))
    eta = rng.gamma(100.0, 0.01, (K, V))
    eta[:, : V // 3] *= rng.gamma(2.0, 1.0, (K, 1))          # topics that differ, so that draws are not near-uniform
    alpha = rng.uniform(0.02, 0.3, K)
    return K, V, csr, alpha, eta


def _run_device(K, V, csr, alpha, eta, seed, stream, heldout, first_document=0, samples=10, burn=5):
    from pylda_amd import _capi
    ctx = _capi.Context(K, V)
    try:
        corpus = ctx.corpus(*csr)
        ctx.set_alpha(alpha)
        ctx.set_eta(eta)
        ctx.hybrid_estep(corpus, samples, burn, seed, stream, first_document, heldout)
        out = {}
        if not heldout:
            ctx.hybrid_scale_sstats(samples - burn)
            out["sstats"] = ctx.get_sstats()
        out["document_log_likelihood"], out["words_log_likelihood"], _ = ctx.estep_results(corpus)
        out["gamma"] = ctx.get_gamma(corpus)
        out["doc_ll"], out["doc_words_ll"], out["iters"] = ctx.get_doc_values(corpus)
        corpus.close()
        return out
    finally:
        ctx.close()


def test_device_philox_known_answers():
    from pylda_amd import _capi
    ctx = _capi.Context(4, 10)
    f = 0xFFFFFFFF
    rec = np.array([[0] * 6, [f] * 6, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0]], np.uint32)
    out = ctx.test_philox(rec)
    assert [list(map(int, r)) for r in out] == [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8],
                                                 [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
                                                 [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]]
    rng = np.random.default_rng(0)
    rec = rng.integers(0, 2 ** 32, size=(1000, 6), dtype=np.uint64).astype(np.uint32)
    host = np.stack(spec.philox4x32_10(*[rec[:, i] for i in range(6)]), axis=1)
    assert np.array_equal(ctx.test_philox(rec), host.astype(np.uint32))
    ctx.close()


@pytest.mark.parametrize("name,heldout", [(n, False) for n in ("ap_k10", "k128", "k256", "k400", "k700", "long_document", "repeated_term")]
                         + [(n, True) for n in ("ap_k10", "k128", "k400", "k700", "repeated_term")])
def test_chain_parity_with_the_restatement(name, heldout, ap_train):
    K, V, csr, alpha, eta = _case(name, ap_train)
    seed, stream = 20240917, 3
    dev = _run_device(K, V, csr, alpha, eta, seed, stream, heldout)
    ref = spec.hybrid_estep(*csr, alpha, eta, seed, stream=stream, heldout=heldout)
    D = len(csr[0]) - 1
    same = np.all(dev["gamma"] == ref["gamma"], axis=1)          # gamma = alpha + the chain's final counts, bit for bit
    divergent = np.nonzero(~same)[0]
    print("%s heldout=%d: %d of %d documents bitwise identical" % (name, heldout, int(same.sum()), D))
    assert same.sum() >= 0.999 * D, divergent
    # a draw can only move where t lies within rounding of a cumulative weight (B is computed by two digamma codes)
    assert np.all(ref["min_gap"][divergent] < 1e-12), ref["min_gap"][divergent]
    assert np.all(dev["iters"] == 10)
    ok = same
    assert rel_err(dev["doc_ll"][ok], ref["doc_ll"][ok], floor=1.0) < 1e-12
    if heldout:
        assert rel_err(dev["doc_words_ll"][ok], ref["doc_words_ll"][ok], floor=1.0) < 1e-12
        if divergent.size == 0:
            assert rel_err(dev["words_log_likelihood"], ref["words_log_likelihood"]) < 1e-12
    else:
        bad_terms = np.zeros(V, bool)
        for d in divergent:
            bad_terms[csr[1][csr[0][d]:csr[0][d + 1]]] = True
        assert np.array_equal(dev["sstats"][:, ~bad_terms], ref["sstats"][:, ~bad_terms])
        if divergent.size == 0:
            assert rel_err(dev["document_log_likelihood"], ref["document_log_likelihood"]) < 1e-12


def test_same_seed_same_result_other_seed_other_result():
    K, V = 64, 800
    csr = _synthetic(200, V, 5, 80, 3)
    rng = np.random.default_rng(4)
    eta, alpha = rng.gamma(100.0, 0.01, (K, V)), np.full(K, 0.05)
    a = _run_device(K, V, csr, alpha, eta, 5, 1, False)
    b = _run_device(K, V, csr, alpha, eta, 5, 1, False)
    c = _run_device(K, V, csr, alpha, eta, 6, 1, False)
    d = _run_device(K, V, csr, alpha, eta, 5, 2, False)
    assert np.array_equal(a["gamma"], b["gamma"]) and np.array_equal(a["sstats"], b["sstats"])
    assert not np.array_equal(a["gamma"], c["gamma"]) and not np.array_equal(a["gamma"], d["gamma"])


def test_sharded_halves_equal_the_whole_run():
    K, V = 128, 1500
    ptr, ids, cts = _synthetic(301, V, 5, 90, 8)
    rng = np.random.default_rng(2)
    eta, alpha = rng.gamma(100.0, 0.01, (K, V)), rng.uniform(0.01, 0.2, K)
    whole = _run_device(K, V, (ptr, ids, cts), alpha, eta, 77, 4, False, samples=10, burn=5)
    half = 150
    first = csr_slice(ptr, ids, cts, range(half))
    second = csr_slice(ptr, ids, cts, range(half, 301))
    # raw counts of each half: add them (what the all-reduce does), then divide once
    from pylda_amd import _capi
    parts = []
    for sub, offset in ((first, 0), (second, half)):
        ctx = _capi.Context(K, V)
        corpus = ctx.corpus(*sub)
        ctx.set_alpha(alpha)
        ctx.set_eta(eta)
        ctx.hybrid_estep(corpus, 10, 5, 77, 4, offset, False)
        parts.append((ctx.get_gamma(corpus), ctx.get_sstats()))
        corpus.close()
        ctx.close()
    assert np.array_equal(np.concatenate([parts[0][0], parts[1][0]]), whole["gamma"])
    assert np.array_equal((parts[0][1] + parts[1][1]) / 5.0, whole["sstats"])


def test_rejects_histories_that_do_not_fit():
    from pylda_amd import _capi
    ctx = _capi.Context(1024, 50)
    corpus = ctx.corpus(np.array([0, 2]), np.array([1, 2], np.int32), np.array([1, 1], np.int32))
    ctx.set_alpha(np.full(1024, 0.1))
    ctx.set_eta(np.ones((1024, 50)))
    with pytest.raises(_capi.PyldaError) as e:
        ctx.hybrid_estep(corpus, 10, 10, 1, 0, 0, False)
    assert e.value.status == -1
    with pytest.raises(_capi.PyldaError) as e:
        ctx.hybrid_estep(corpus, 12, 5, 1, 0, 0, False)          # 8 samples x 10 bits
    assert e.value.status == -1
    ctx.hybrid_estep(corpus, 10, 5, 1, 0, 0, False)               # 6 x 10 bits: fits
    corpus.close()
    ctx.close()


def _hybrid_model(ap_train, docs=300, seed=9):
    from pylda_amd.hybrid import Hybrid
    g = ap_train
    ptr, ids, cts = csr_slice(g["doc_ptr"], g["term_id"], g["term_ct"], range(docs))
    m = Hybrid(seed=seed)
    m._verbose = False
    eta = np.random.default_rng(3).gamma(100.0, 0.01, (10, len(g["words"])))
    m._initialize_parsed(ptr, ids, cts, len(g["words"]), 10, 0.1, 1.0 / len(g["words"]), eta=eta)
    return m


def test_learning_on_the_device_equals_the_public_seam(ap_train):
    """learning() fused on the device (raw counts -> scale -> device M-step) computes what the reference's template
    method computes through e_step() / m_step() with host arrays."""
    from pylda_amd.hybrid import Hybrid

    class ThroughSeam(Hybrid):
        def e_step(self, *args, **kwargs):
            return Hybrid.e_step(self, *args, **kwargs)

    fused = _hybrid_model(ap_train)
    fused._hyper_parameter_optimize_interval = 0
    seam = _hybrid_model(ap_train)
    seam.__class__ = ThroughSeam
    seam._hyper_parameter_optimize_interval = 0
    for _ in range(3):
        a, b = fused.learning(), seam.learning()
        assert np.isfinite(a) and rel_err(a, b) < 1e-12
    assert np.array_equal(fused._gamma, seam._gamma)
    assert rel_err(fused._eta, seam._eta) < 1e-12


def test_learning_improves_and_snapshot_continues_bitwise(ap_train):
    m = _hybrid_model(ap_train)
    trace = [m.learning() for _ in range(4)]
    assert all(np.isfinite(trace)) and trace[-1] > trace[0]
    assert np.all(m._alpha_alpha > 0)
    restored = pickle.loads(pickle.dumps(m))
    assert restored._sampler_seed == m._sampler_seed and restored._counter == m._counter
    a, b = m.learning(), restored.learning()
    assert a == b
    assert np.array_equal(m._gamma, restored._gamma) and np.array_equal(m._alpha_alpha, restored._alpha_alpha)
    # held-out: the reference's token lists, and the CSR of parse_to_csr, give the same gamma (grouped order)
    g = ap_train
    docs = [[int(t) for t, c in zip(g["term_id"][g["doc_ptr"][d]:g["doc_ptr"][d + 1]],
                                    g["term_ct"][g["doc_ptr"][d]:g["doc_ptr"][d + 1]]) for _ in range(c)]
            for d in range(1900, 1920)]
    m._heldout_calls = restored._heldout_calls = 0
    wll, gamma = m.e_step(docs)
    wll2, gamma2 = restored.e_step(csr_slice(g["doc_ptr"], g["term_id"], g["term_ct"], range(1900, 1920)))
    assert gamma.shape == (20, 10) and np.isfinite(wll) and wll < 0
    assert np.array_equal(gamma, gamma2) and wll == wll2


def test_launch_train_mode_0_and_launch_test(ap_train, tmp_path, capsys):
    from pylda_amd import launch_test, launch_train
    g = ap_train
    words = [str(w) for w in g["words"]]
    corpus_dir = tmp_path / "mini-press"
    corpus_dir.mkdir()
    docs = []
    for d in range(120):
        lo, hi = int(g["doc_ptr"][d]), int(g["doc_ptr"][d + 1])
        docs.append(" ".join(" ".join([words[t]] * int(c)) for t, c in zip(g["term_id"][lo:hi], g["term_ct"][lo:hi])))
    (corpus_dir / "train.dat").write_text("\n".join(docs[:100]) + "\n")
    (corpus_dir / "test.dat").write_text("\n".join(docs[100:120]) + "\n")
    (corpus_dir / "voc.dat").write_text("".join("%s\t1\t1\n" % w for w in words))
    out_dir = tmp_path / "out"
    np.random.seed(3)
    rc = launch_train.main(["--input_directory=%s" % corpus_dir, "--output_directory=%s" % out_dir,
                            "--number_of_topics=5", "--training_iterations=4", "--snapshot_interval=2",
                            "--inference_mode=0", "--sampler_seed=1"])
    assert rc == 0
    runs = list((out_dir / "mini-press").iterdir())
    assert len(runs) == 1 and runs[0].name.endswith("-im0")
    names = sorted(p.name for p in runs[0].iterdir())
    assert names == ["exp_beta-2", "exp_beta-4", "exp_gamma-2", "exp_gamma-4", "model-4", "option.txt"]
    opts = dict(l.split("=", 1) for l in (runs[0] / "option.txt").read_text().splitlines())
    assert opts["inference_mode"] == "0" and opts["sampler_seed"] == "1"
    with open(runs[0] / "model-4", "rb") as f:
        model = pickle.load(f)
    from pylda_amd.hybrid import Hybrid
    assert isinstance(model, Hybrid) and model._sampler_seed == 1
    capsys.readouterr()
    assert launch_test.main(["--input_directory=%s" % corpus_dir, "--model_directory=%s" % runs[0],
                             "--snapshot_index=4"]) == 0
    assert "held-out likelihood of snapshot" in capsys.readouterr().out
    gamma = np.loadtxt(runs[0] / "test-4")
    assert gamma.shape == (20, 5) and np.all(gamma > 0)


@pytest.mark.parametrize("heldout", [False, True])
def test_device_moments_match_the_reference_hybrid(heldout):
    """The kernel's chain against the reference's hybrid.py itself (tests/golden/hybrid_moments_k8.npz, made by
    tests/golden/make_hybrid_golden.py): one 60-token document replicated 4000 times, gamma, the likelihood per batch of
    200 documents and the statistics of the document's terms within 5 sigma of the reference's."""
    from conftest import load_golden
    from hybrid_golden_checks import moment_failures, replicated_document
    g = load_golden("hybrid_moments_k8.npz")
    K, V = g["eta"].shape
    out = _run_device(K, V, replicated_document(g), g["alpha"], g["eta"], 8642, 2 ** 31 if heldout else 1, heldout)
    stats = None if heldout else out["sstats"][:, g["terms"]] / float(g["replicas"])
    values = out["doc_words_ll"] if heldout else out["doc_ll"]
    assert moment_failures(g, "heldout" if heldout else "train", out["gamma"], values, stats) == []


def test_training_stays_in_the_reference_seeds_band(ap_train):
    """Hybrid.learning() on the first 300 associated-press documents (K=10, 15 iterations, pinned initial eta) against the
    reference's Hybrid.learning() under four numpy seeds (tests/golden/hybrid_trace_k10.npz): joint log-likelihood and
    sum(alpha) inside the seeds' range widened by three times its spread, at every iteration."""
    from conftest import load_golden
    from hybrid_golden_checks import trace_band
    from pylda_amd.hybrid import Hybrid
    golden = load_golden("hybrid_trace_k10.npz")
    band = trace_band(golden)
    g = ap_train
    V, K, docs = len(g["words"]), 10, int(golden["documents"])
    ptr, ids, cts = csr_slice(g["doc_ptr"], g["term_id"], g["term_ct"], range(docs))
    eta = np.random.default_rng(3).gamma(100.0, 1.0 / 100.0, (K, V))       # make_hybrid_golden.trace_eta
    m = Hybrid(seed=31)
    m._verbose = False
    m._initialize_parsed(ptr, ids, cts, V, K, 1.0 / K, 1.0 / V, eta=eta)
    for i in range(int(golden["iterations"])):
        ll = m.learning()
        a = float(np.sum(m._alpha_alpha))
        lo, hi = band["joint_ll"][0][i], band["joint_ll"][1][i]
        assert lo <= ll <= hi, (i, ll, lo, hi)
        lo, hi = band["alpha_sum"][0][i], band["alpha_sum"][1][i]
        assert lo <= a <= hi, (i, a, lo, hi)

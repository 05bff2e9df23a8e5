"""CPU-side checks of stochastic collapsed variational Bayes (SCVB0): the numpy restatement
(tests/scvb_restatement.py) against a step written straight from the formulas, its binary power, its two invariants and its
behaviour on the rehearsal corpus with the recorded figures of tests/golden/scvb_rehearsal.json, the class without a GPU,
the command line, the C ABI's additions, the traffic hash and the update kernel's registers."""
import hashlib
import json
import os
import pickle
import re
import sys

import numpy as np
import pytest

import scvb_restatement as spec
from conftest import GOLDEN, ROOT
from test_cvb0_host import _tiny_corpus

sys.path.insert(0, GOLDEN)
import make_scvb_golden as rehearsal  # noqa: E402

SYMBOLS = ("pylda_scvb_init", "pylda_scvb_step", "pylda_scvb_get_state", "pylda_scvb_set_state")


# ---------------------------------------------------------------- the restatement against the textbook
@pytest.mark.parametrize("batches", [1, 3, 6])
@pytest.mark.parametrize("burn_in", [0, 1, 3])
def test_restatement_equals_the_textbook_step(batches, burn_in):
    """After 1 and after B + 1 steps (the second epoch's step sizes).  The textbook form uses ** and plain sums and keeps its
    sums per word in any order; the restatement sums by lanes, segments and chunks."""
    K, V = 3, 12
    csr = _tiny_corpus()
    alpha, beta = np.array([0.3, 0.5, 0.2]), np.linspace(0.05, 0.2, V)
    chain = spec.ScvbChain(*csr, K, V)
    chain.init(11)
    start = chain.state()
    n_kv, n_k, n_dk = (x.tolist() for x in start)
    for t in range(batches + 1):
        chain.step(alpha, beta, batches, burn_in=burn_in)
        spec.textbook_step(*csr, n_kv, n_k, n_dk, alpha.tolist(), beta.tolist(), t, batches, burn_in, 10.0, 0.9, 10.0, 0.9)
        if t in (0, batches):
            for name, a, b in zip(("T", "n_k", "N_dk"), chain.state(), (n_kv, n_k, n_dk)):
                err = float(np.max(np.abs(a - np.array(b)) / np.maximum(np.abs(np.array(b)), 1e-300)))
                print("%s: largest relative difference from the textbook after %d steps %.3g" % (name, t + 1, err))
                assert err < 1e-9, name
    assert not np.array_equal(chain.state()[0], start[0]) and not np.array_equal(chain.state()[2], start[2])


def _multiplies(c):
    """the multiplies binary_power performs for the exponent c"""
    n, count = int(c), 0
    while n:
        count += n & 1
        n >>= 1
        count += 1 if n else 0
    return count


@pytest.mark.parametrize("c", [1, 2, 3, 7, 300, 10 ** 6])
def test_binary_power_is_within_an_ulp_per_multiply(c):
    """The restatement's x ** c against float ** int, within one ulp per multiply of the binary exponentiation, for the first
    step sizes of the default schedule (x = 1 - 10 ** -0.9, 1 - 11 ** -0.9) and an exact case (0.5); an underflow to 0 is 0 in
    both.  The loop in plain doubles does not hold this bound - a squaring doubles the relative error it inherits, and c = 300
    (12 multiplies) came out 54 ulp off for the first x - which is why binary_power and the kernel's scvb_power form their
    products in double-double arithmetic; observed with it: 0 ulp in every case."""
    multiplies = _multiplies(c)
    worst = 0.0
    for x in (1.0 - 10.0 ** -0.9, 1.0 - 11.0 ** -0.9, 0.5):
        got, want = float(spec.binary_power(x, [c])[0]), x ** c
        ulps = abs(got - want) / np.spacing(want)
        worst = max(worst, ulps)
        print("x=%r c=%d: %r against %r: %.1f ulp, %d multiplies" % (x, c, got, want, ulps, multiplies))
    assert worst <= multiplies
    assert np.array_equal(spec.binary_power(0.5, [0, 1, 2, 10]), [1.0, 0.5, 0.25, 2.0 ** -10])


# ---------------------------------------------------------------- the rehearsal corpus
@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "scvb_rehearsal.json")) as stream:
        return json.load(stream)


@pytest.mark.parametrize("burn_in", [0, 1])
@pytest.mark.parametrize("batches", [1, 8, 300])
def test_rehearsal_corpus(recorded, batches, burn_in):
    """300 associated-press documents, K = 10, 25 epochs, the default schedule: the two invariants (a document's row of N_dk
    keeps the sum C_j, sum(T) stays C) after every run, every recorded figure, and every run ends above its start.  The
    restatement rises on every epoch except with 300 minibatches and no burn-in, whose first epoch falls below the start
    (DESIGN.md section 22): asserted only where it shows.  No order between the figures of different B is asserted."""
    chain, trace = rehearsal.rehearsal(batches, burn_in)
    print("B=%d burn_in=%d: start %.3f, after 1 epoch %.3f, after 25 %.3f" % (batches, burn_in, trace[0], trace[1], trace[-1]))
    want = recorded["log_likelihood"]["%d/%d" % (batches, burn_in)]
    assert len(trace) == len(want) == 26
    for got, figure in zip(trace, want):
        assert abs(got - figure) <= 1e-10 * abs(figure), (got, figure)
    assert trace[-1] > trace[0]
    if (batches, burn_in) != (300, 0):
        assert all(b > a for a, b in zip(trace, trace[1:])), trace
    tokens = float(chain.tokens)
    worst_row = float(np.max(np.abs(chain.n_dk.sum(axis=1) - chain.doc_tokens) / chain.doc_tokens))
    print("largest relative error of a row sum of N_dk %.3g, of sum(T) %.3g" % (worst_row, abs(chain.T.sum() - tokens) / tokens))
    assert worst_row <= 1e-9 and abs(chain.T.sum() - tokens) <= tokens * 1e-9
    assert np.allclose(chain.T[:, :chain.K].sum(axis=0), chain.n_k[:chain.K], rtol=1e-12, atol=0)
    assert chain.T.min() >= 0.0 and chain.n_dk.min() >= 0.0


def test_a_minibatch_without_documents_changes_nothing():
    K, V = 3, 12
    csr = _tiny_corpus()
    chain = spec.ScvbChain(*csr, K, V, first_document=4)
    chain.init(2)
    before = [x.copy() for x in chain.state()]
    chain.step(0.3, 0.1, 50)                # block 0 of 50: global indices 4 .. 9 hold none
    assert chain.t == 1 and all(np.array_equal(a, b) for a, b in zip(chain.state(), before))
    for _ in range(3):
        chain.step(0.3, 0.1, 50)
    assert chain.t == 4 and all(np.array_equal(a, b) for a, b in zip(chain.state(), before))
    chain.step(0.3, 0.1, 50)                # block 4: local document 0
    assert not np.array_equal(chain.state()[2][0], before[2][0]) and np.array_equal(chain.state()[2][1:], before[2][1:])


# ---------------------------------------------------------------- the Python class
def test_class_contract_without_a_gpu():
    from pylda_amd.cvb0 import CollapsedVariationalBayes
    from pylda_amd.scvb0 import StochasticCollapsedVariationalBayes as Scvb
    import inspect
    assert issubclass(Scvb, CollapsedVariationalBayes)
    assert str(inspect.signature(Scvb.__init__)) == ("(self, batches, burn_in=1, tau0=10.0, kappa=0.9, theta_tau0=10.0, "
                                                    "theta_kappa=0.9, device=0, seed=None)")
    m = Scvb(4, seed=12)
    assert m._sampler_seed == 12 and m._batches == 4 and m._burn_in == 1 and m._step == 0 and m.last_change is None
    assert not hasattr(m, "fold_in")                     # launch_test takes the inference() path
    for inherited in ("inference", "document_completion", "left_to_right", "top_words", "topic_coherence", "similar_documents",
                      "top_documents", "topic_distances", "export_beta", "export_gamma"):
        assert getattr(Scvb, inherited) is getattr(CollapsedVariationalBayes, inherited), inherited
    for bad in (dict(batches=0), dict(batches=2, burn_in=16), dict(batches=2, burn_in=-1), dict(batches=2, tau0=0.5),
                dict(batches=2, kappa=0.5), dict(batches=2, theta_tau0=0.0), dict(batches=2, theta_kappa=1.5), dict(batches=2.5)):
        with pytest.raises(ValueError):
            Scvb(**bad)
    # the step's parameters are the restatement's
    m._train_csr = _tiny_corpus()
    m._number_of_tokens = int(m._train_csr[2].sum())
    m._first_document = 0
    for step in (0, 1, 5, 9):
        batch, keep, gain, rho_theta = m.step_parameters(step)
        docs = np.arange(batch, 6, 4)
        block_tokens = sum(int(m._train_csr[2][m._train_csr[0][d]:m._train_csr[0][d + 1]].sum()) for d in docs)
        want = spec.step_parameters(step, 4, 1, 10.0, 0.9, 10.0, 0.9, m._number_of_tokens, block_tokens)
        assert batch == step % 4 and (keep, gain, rho_theta) == want[:3]
        assert all(0.0 < rho <= 1.0 for rho in rho_theta) and 0.0 <= keep < 1.0
    # a snapshot: the counts, the step counter and the schedule, no per-slot rows
    m._host_state = (np.zeros((3, 12)), np.zeros(3), np.zeros((6, 3)))
    m._step = 7
    state = m.__getstate__()
    assert state["_ctx"] is None and state["_train_corpus"] is None and state["_sampler_seed"] == 12
    restored = pickle.loads(pickle.dumps(m))
    assert len(restored._host_state) == 3 and restored._step == 7
    assert (restored._batches, restored._burn_in, restored._tau0, restored._kappa, restored._theta_tau0, restored._theta_kappa) == \
        (4, 1, 10.0, 0.9, 10.0, 0.9)
    assert not [key for key in restored.__dict__ if key in ("g", "_g")]


# ---------------------------------------------------------------- the command line
BASE = ["--input_directory=in", "--output_directory=out", "--number_of_topics=3", "--training_iterations=1", "--inference_mode=3"]


def test_minibatch_flags_are_refused_where_they_cannot_run(capsys, monkeypatch):
    from pylda_amd import cli

    def refused(flags, *named):
        assert cli.train_main(BASE + flags) == 2
        err = capsys.readouterr().err
        for name in named:
            assert name in err, (name, err)
    refused(["--sampler_seed=4", "--cvb0_minibatches=8", "--cvb0_blocks=16"], "--cvb0_minibatches", "--cvb0_blocks")
    refused(["--sampler_seed=4", "--cvb0_minibatches=8", "--gpus=2"], "--cvb0_minibatches", "one GPU")
    refused(["--sampler_seed=4", "--cvb0_minibatches=8", "--online_batches=4"], "--online_batches")
    refused(["--cvb0_minibatches=8"], "--sampler_seed")
    refused(["--sampler_seed=4", "--cvb0_minibatches=0"], "--cvb0_minibatches")
    refused(["--sampler_seed=4", "--cvb0_minibatches=8", "--cvb0_tau0=0.5"], "--cvb0_tau0", "tau0")
    refused(["--sampler_seed=4", "--cvb0_minibatches=8", "--cvb0_tau0=-1"], "--cvb0_tau0", "tau0")     # (no value stands for "not given")
    refused(["--sampler_seed=4", "--cvb0_minibatches=8", "--cvb0_burn_in=-1"], "--cvb0_burn_in", "burn_in")
    refused(["--sampler_seed=4", "--cvb0_minibatches=8", "--cvb0_kappa=0.4"], "--cvb0_kappa", "kappa")
    refused(["--sampler_seed=4", "--cvb0_minibatches=8", "--cvb0_burn_in=16"], "--cvb0_burn_in", "burn_in")
    refused(["--sampler_seed=4", "--cvb0_blocks=8", "--cvb0_burn_in=2"], "--cvb0_burn_in", "--cvb0_minibatches")
    refused(["--sampler_seed=4", "--cvb0_blocks=8", "--cvb0_tau0=2"], "--cvb0_minibatches")
    assert cli.train_main([f for f in BASE if "inference_mode" not in f] + ["--cvb0_minibatches=8", "--sampler_seed=1"]) == 2
    assert "--cvb0_minibatches" in capsys.readouterr().err            # (the default mode, 2, has no such form)
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(["--sampler_seed=4", "--cvb0_minibatches=8"], "--cvb0_minibatches", "one GPU")


def test_existing_mode_3_refusals_keep_their_wording(capsys):
    from pylda_amd import cli
    assert cli.train_main(BASE) == 2
    err = capsys.readouterr().err
    assert "--sampler_seed" in err and "--cvb0_blocks" in err
    assert cli.train_main(BASE + ["--sampler_seed=4"]) == 2
    assert "--cvb0_blocks" in capsys.readouterr().err
    assert cli.train_main(BASE + ["--sampler_seed=4", "--cvb0_blocks=16", "--online_batches=4"]) == 2
    assert "the engines of modes 0, 1 and 3 have no minibatch form here" in capsys.readouterr().err


def test_more_minibatches_than_documents_is_refused(tmp_path, capsys):
    from pylda_amd import cli
    corpus = tmp_path / "three"
    corpus.mkdir()
    (corpus / "train.dat").write_text("a b\nb c\nc a\n")
    (corpus / "voc.dat").write_text("a\nb\nc\n")
    flags = ["--input_directory=%s" % corpus, "--output_directory=%s" % (tmp_path / "out"), "--number_of_topics=2",
             "--training_iterations=1", "--inference_mode=3", "--sampler_seed=1", "--cvb0_minibatches=4"]
    assert cli.train_main(flags) == 2
    err = capsys.readouterr().err
    assert "--cvb0_minibatches=4" in err and "3 documents" in err
    assert not (tmp_path / "out").exists()


def test_minibatch_flags_parse_and_take_their_defaults():
    from pylda_amd import cli
    opt = cli._parse(cli.TRAIN_FLAGS, BASE + ["--sampler_seed=7", "--cvb0_minibatches=64", "--cvb0_burn_in=2", "--cvb0_tau0=20",
                                              "--cvb0_kappa=0.7"], "launch_train")
    assert (opt.cvb0_minibatches, opt.cvb0_burn_in, opt.cvb0_tau0, opt.cvb0_kappa, opt.cvb0_blocks) == (64, 2, 20.0, 0.7, -1)
    assert cli._stochastic_refusal(opt) is None
    opt = cli._parse(cli.TRAIN_FLAGS, BASE + ["--sampler_seed=7", "--cvb0_minibatches=64"], "launch_train")
    assert cli._stochastic_refusal(opt) is None
    assert (opt.cvb0_burn_in, opt.cvb0_tau0, opt.cvb0_kappa) == (1, 10.0, 0.9)
    assert cli._parse(cli.TRAIN_FLAGS, BASE, "launch_train").cvb0_minibatches == -1
    assert "--cvb0_minibatches" in cli.__doc__


# ---------------------------------------------------------------- the C ABI
def test_abi_names_the_additions_and_keeps_its_version():
    from pylda_amd import _capi
    text = open(os.path.join(ROOT, "include", "pylda_hip.h")).read()
    assert _capi.ABI_VERSION == 10 and re.search(r"#define PYLDA_ABI_VERSION 10\b", text)
    line = text[text.index(" *  10  additions only"):text.index("A host compiled against another version")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES and name in line, name
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert "cvb0" not in name and re.fullmatch(r"[a-z_]+", name)
    # the argument counts of the header and of the binding
    for name in SYMBOLS:
        declaration = re.search(r"\bint %s\s*\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(declaration.split(",")) == len(_capi.SIGNATURES[name][1]), name
    for method in ("scvb_init", "scvb_step", "scvb_get_state", "scvb_set_state"):
        assert callable(getattr(_capi.Context, method))


def test_library_exports_the_additions_and_a_stale_one_asks_for_a_rebuild():
    import ctypes
    from pylda_amd import _capi, build
    build.build(verbose=False)
    lib = _capi.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name

    class Stale(object):                     # a library from before the additions: every other symbol, none of these
        def __getattr__(self, name):
            if name in SYMBOLS:
                raise AttributeError(name)
            return ctypes.CFUNCTYPE(ctypes.c_int)(lambda: 0)
    with pytest.raises(RuntimeError) as e:
        _capi._bind(Stale(), "libpylda_hip.so")
    assert "rebuild" in str(e.value) and "pylda_scvb_" in str(e.value)


# ---------------------------------------------------------------- the kernels' sources
def test_kernel_source_hash_is_what_it_was_without_the_new_files():
    """bench.kernel_source_hash() over csrc/ equals the hash of the file list that leaves this feature's files out."""
    import bench
    csrc = os.path.join(ROOT, "pylda_amd", "csrc")
    new_files = ("scvb_kernels.h",)
    for f in new_files:
        assert os.path.exists(os.path.join(csrc, f)), f
    h = hashlib.sha256()
    for f in sorted(os.listdir(csrc)):
        if f in new_files:
            continue
        if f.endswith(".h") and (f.startswith("estep_") or f.startswith("sstats_") or f in ("doc_terms.h", "special_device.h", "prepare_kernels.h")):
            h.update(f.encode())
            h.update(open(os.path.join(csrc, f), "rb").read())
    assert bench.kernel_source_hash() == h.hexdigest()[:16]
    assert not any(f.startswith(("estep_", "sstats_")) for f in new_files)


def test_scvb_kernels_use_no_scratch():
    """Every scvb_* kernel the library ships, from the compiler's own metadata: no scratch, in any instantiation."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    lines = open(kr.compile_to_asm(os.path.join(ROOT, "pylda_amd", "csrc", "launch_cvb0.hip"))).read().splitlines()
    res = kr.resources(lines, "scvb_")
    names = kr.demangle(list(res))
    shipped = sorted(names[m] for m in res)
    for kernel in ("scvb_update_kernel", "scvb_init_kernel"):
        slots = sorted(int(re.search(kernel + r"<(\d+)", n).group(1)) for n in shipped if kernel in n)
        assert slots == [1, 2, 4, 8, 16], (kernel, shipped)
    for kernel in ("scvb_blend_kernel", "scvb_run_map_kernel"):
        assert sum(kernel in n for n in shipped) == 1, shipped
    assert len(shipped) == 12, shipped
    for mangled, info in res.items():
        print(names[mangled], info)
        assert info["ScratchSize"] == 0, (names[mangled], info)
        assert info["NumVgprs"] <= 256, (names[mangled], info)

"""CPU-side checks of the collapsed variational Bayes engine (CVB0): the numpy restatement
(tests/cvb0_restatement.py) against a sequential CVB0 written straight from the formula, its behaviour on the rehearsal corpus
with the recorded figures of tests/golden/cvb0_rehearsal.json, the control that leaves the own token in, the host builder of
the blocks' postings against a direct numpy sort, the command line, and the C ABI's additions."""
import json
import os
import re
import sys

import numpy as np
import pytest

import cvb0_restatement as spec
from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_cvb0_golden as rehearsal  # noqa: E402


# ---------------------------------------------------------------- the restatement against the textbook
def _tiny_corpus():
    """6 documents over 12 word types; counts up to 4, a one-token document, a word in every document."""
    rng = np.random.default_rng(2)
    ptr, ids, cts = [0], [], []
    for d in range(6):
        n = 1 if d == 3 else int(rng.integers(2, 8))
        rest = rng.choice(np.arange(1, 12), size=n - 1, replace=False)
        u = np.concatenate([[0], rest]) if d != 3 else np.array([0])
        ids.append(u)
        cts.append(np.array([1]) if d == 3 else rng.integers(1, 5, size=u.size))
        ptr.append(ptr[-1] + u.size)
    return np.array(ptr, np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(cts).astype(np.int32)


@pytest.mark.parametrize("blocks", [6, 1000])
def test_restatement_equals_textbook_cvb0_when_every_document_is_a_block(blocks):
    """blocks >= D: a document sees every earlier document's changes, which is sequential CVB0.  The textbook form keeps
    n_k by increments and sums with plain sum(); the restatement recomputes n_k from T in chunks and sums by lanes."""
    K, V = 3, 12
    csr = _tiny_corpus()
    alpha, beta = np.array([0.3, 0.5, 0.2]), np.linspace(0.05, 0.2, V)
    chain = spec.Cvb0Chain(*csr, K, V)
    chain.init(11)
    n_kv, n_k, n_dk, g = (x.tolist() for x in chain.state())
    for _ in range(5):
        chain.sweep(alpha, beta, blocks)
        spec.textbook_sweep(*csr, n_kv, n_k, n_dk, g, alpha.tolist(), beta.tolist())
    got = chain.state()
    for name, a, b in zip(("T", "n_k", "N_dk", "g"), got, (n_kv, n_k, n_dk, g)):
        err = float(np.max(np.abs(a - np.array(b))))
        print("%s: largest difference from the textbook after 5 sweeps %.3g" % (name, err))
        assert err < 1e-9, name
    assert not np.array_equal(got[3], spec.Cvb0Chain(*csr, K, V).state()[3])


def test_one_block_differs_from_the_sequential_chain_but_keeps_its_books():
    K, V = 3, 12
    csr = _tiny_corpus()
    one, seq = spec.Cvb0Chain(*csr, K, V), spec.Cvb0Chain(*csr, K, V)
    for chain, blocks in ((one, 1), (seq, 6)):
        chain.init(11)
        for _ in range(3):
            chain.sweep(0.4, 0.1, blocks)
    assert not np.array_equal(one.g, seq.g)
    tokens = float(np.sum(csr[2]))
    for chain in (one, seq):
        assert abs(chain.T.sum() - tokens) < tokens * 1e-12 and np.allclose(chain.T[:, :K].sum(axis=0), chain.n_k[:K], rtol=0, atol=1e-12)
        assert np.allclose(chain.n_dk[:, :K].sum(axis=1), np.add.reduceat(csr[2], csr[0][:-1]), rtol=0, atol=1e-12)


def test_start_is_the_gibbs_start():
    """Every copy's start topic is the collapsed Gibbs engine's: the slots' histograms are its topics counted."""
    import gibbs_restatement
    K, V = 5, 12
    ptr, ids, cts = _tiny_corpus()
    gibbs = gibbs_restatement.GibbsChain(ptr, ids, cts, K, V, seed=8, first_document=3)
    gibbs.init()
    m = spec.start_rows(ptr, cts, K, 8, 0, first_document=3)
    slot = np.repeat(np.arange(len(ids)), cts)
    want = np.zeros((len(ids), K))
    np.add.at(want, (slot, gibbs.z), 1.0)
    assert np.array_equal(m, want)
    assert not np.array_equal(m, spec.start_rows(ptr, cts, K, 9, 0, first_document=3))


# ---------------------------------------------------------------- the rehearsal corpus
@pytest.fixture(scope="module")
def runs():
    """blocks -> (chain, the likelihood at the start and after each of the 25 sweeps)"""
    return {blocks: rehearsal.rehearsal(blocks) for blocks in (1, 16, 300)}


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "cvb0_rehearsal.json")) as stream:
        return json.load(stream)


@pytest.mark.parametrize("blocks", [1, 16, 300])
def test_rehearsal_corpus(runs, recorded, blocks):
    """300 associated-press documents, K = 10, 25 sweeps: the likelihood rises on every sweep, the table's mass stays the
    token count, every row of g stays a distribution, and the final figure is the recorded one.  (No order between the
    figures of different `blocks` is asserted: the rehearsal of the scheme showed it is not fixed.)"""
    chain, trace = runs[blocks]
    print("blocks=%d: start %.3f, after 1 sweep %.3f, after 25 %.3f" % (blocks, trace[0], trace[1], trace[-1]))
    assert all(b > a for a, b in zip(trace, trace[1:])), trace
    assert trace[-1] > trace[1]
    tokens = float(np.sum(chain.term_ct))
    assert abs(chain.T.sum() - tokens) <= tokens * 1e-9
    K = chain.K
    assert np.max(np.abs(chain.g[:, :K].sum(axis=1) - 1.0)) <= K * 2.0 ** -52
    assert chain.g.min() >= 0.0 and chain.T.min() >= 0.0
    assert trace[0] == recorded["start"]
    want = recorded["log_likelihood"][str(blocks)]
    assert abs(trace[-1] - want) <= 1e-10 * abs(want), (trace[-1], want)


def test_own_token_left_in_moves_the_figure(recorded):
    """The control: without the three `- go` the 25-sweep figure of blocks = 1 misses the recorded one by nine orders of
    magnitude more than its pin allows (LABNOTES has the figures)."""
    _, trace = rehearsal.rehearsal(1, remove_own=False)
    want = recorded["log_likelihood"]["1"]
    moved = abs(trace[-1] - want) / abs(want)
    print("own token left in: %.6f against %.6f, relative %.3g" % (trace[-1], want, moved))
    assert moved > 1e-4


# ---------------------------------------------------------------- the postings of the blocks
def _postings_case(name):
    """(doc_ptr, term_id, blocks, first_document)"""
    rng = np.random.default_rng(len(name))
    if name in ("more_blocks_than_documents", "empty_block", "offset"):
        D, V = 7, 30
        docs = [np.sort(rng.choice(V, size=int(rng.integers(0 if name == "empty_block" else 1, 9)), replace=False)) for _ in range(D)]
        blocks, first = {"more_blocks_than_documents": (50, 0), "empty_block": (3, 0), "offset": (4, 6)}[name]
        if name == "empty_block":
            # block 1's documents (1 and 4) have no term: a round with documents and without postings
            for d in (1, 4):
                docs[d] = np.zeros(0, dtype=np.int64)
    else:
        # word 0 in exactly n documents of block 0 (of 2 blocks); word 1 in every document; others at random
        n = int(name.split("_")[1])
        D, V, blocks, first = 2 * n + 6, 40, 2, 0
        docs = []
        for d in range(D):
            rest = rng.choice(np.arange(2, V), size=int(rng.integers(0, 4)), replace=False)
            head = [0, 1] if d % 2 == 0 and d // 2 < n else [1]
            docs.append(np.concatenate([rest[:1], head, rest[1:]]).astype(np.int64))       # (terms in no particular order)
    ptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return ptr, np.concatenate(docs).astype(np.int32), blocks, first


@pytest.mark.parametrize("name", ["more_blocks_than_documents", "empty_block", "offset", "word_255", "word_256", "word_257", "word_513"])
def test_block_postings_equal_a_direct_sort(name):
    from pylda_amd import _capi, build
    build.build(verbose=False)
    ptr, ids, blocks, first = _postings_case(name)
    got = _capi.cvb0_block_postings(ptr, ids, blocks, first)
    want = spec.block_rounds(ptr, ids, blocks, first)
    rounds = got["rounds"]
    assert len(rounds) == len(want)
    post0 = seg0 = run0 = 0
    for row, (block, docs, postings) in zip(rounds, want):
        g, first_doc, ndocs, post1, seg1, run1 = (int(x) for x in row)
        assert (g, first_doc, ndocs) == (block, int(docs[0]), len(docs))
        assert np.array_equal(docs, first_doc + blocks * np.arange(ndocs))
        assert np.array_equal(got["post_slot"][post0:post1], postings)
        assert np.array_equal(got["slot_place"][postings], np.arange(len(postings)))
        # runs: the distinct words in ascending order; segments: a run cut every 256 postings
        words = ids[postings]
        distinct, counts = np.unique(words, return_counts=True)
        assert np.array_equal(got["run_word"][run0:run1], distinct)
        seg_ends, run_segs = [], [seg0]
        at = post0
        for c in counts:
            seg_ends += [at + min(c, s + 256) for s in range(0, c, 256)]
            at += c
            run_segs.append(seg0 + len(seg_ends))
        assert np.array_equal(got["seg_begin"][seg0 + 1:seg1 + 1], seg_ends) and got["seg_begin"][seg0] == post0
        assert np.array_equal(got["run_seg"][run0:run1 + 1], run_segs)
        assert seg1 - seg0 == len(seg_ends)
        post0, seg0, run0 = post1, seg1, run1
    assert post0 == len(ids)
    assert got["widest_postings"] == max([len(p) for _, _, p in want] + [0])
    if name.startswith("word_"):
        n = int(name.split("_")[1])
        assert got["run_word"][0] == 0                   # block 0's first run: word 0, n postings
        sizes = np.diff(got["seg_begin"][int(got["run_seg"][0]):int(got["run_seg"][1]) + 1])
        assert sizes.tolist() == [256] * (n // 256) + ([n % 256] if n % 256 else [])
    if name == "empty_block":
        assert [int(r[0]) for r in rounds] == [0, 1, 2] and int(rounds[1][3]) == int(rounds[0][3])     # block 1: documents, no posting
    if name == "more_blocks_than_documents":
        assert [int(r[0]) for r in rounds] == list(range(7)) and all(int(r[2]) == 1 for r in rounds)


def test_postings_builder_under_asan_ubsan(tmp_path):
    """The builder is a pure function beside the planner's (host_plan.cpp, no HIP): with tests/native/cvb0_postings_fuzz.cpp
    it compiles with plain g++ -fsanitize=address,undefined and runs on random corpora on the CPU."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "cvb0_postings_fuzz")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "pylda_amd", "csrc", "host_plan.cpp"),
           os.path.join(ROOT, "tests", "native", "cvb0_postings_fuzz.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtimes not installed: " + build.stderr.splitlines()[0])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cvb0 postings sanitizer run: ok" in run.stdout


# ---------------------------------------------------------------- the command line
def test_mode_3_needs_its_two_flags_and_one_gpu(capsys):
    from pylda_amd import cli
    base = ["--input_directory=in", "--output_directory=out", "--number_of_topics=3", "--training_iterations=1",
            "--inference_mode=3"]
    assert cli.train_main(base + ["--sampler_seed=4"]) == 2
    assert "--cvb0_blocks" in capsys.readouterr().err
    assert cli.train_main(base + ["--cvb0_blocks=16"]) == 2
    assert "--sampler_seed" in capsys.readouterr().err
    assert cli.train_main(base) == 2
    err = capsys.readouterr().err
    assert "--sampler_seed" in err and "--cvb0_blocks" in err
    assert cli.train_main(base + ["--sampler_seed=4", "--cvb0_blocks=0"]) == 2
    capsys.readouterr()
    assert cli.train_main(base + ["--sampler_seed=4", "--cvb0_blocks=16", "--gpus=2"]) == 2
    assert "one GPU" in capsys.readouterr().err
    assert cli.train_main(base + ["--sampler_seed=4", "--cvb0_blocks=16", "--online_batches=4"]) == 2
    assert "--online_batches" in capsys.readouterr().err
    opt = cli._parse(cli.TRAIN_FLAGS, base + ["--sampler_seed=7", "--cvb0_blocks=64"], "launch_train")
    assert opt.sampler_seed == 7 and opt.cvb0_blocks == 64 and opt.inference_mode == 3
    assert cli._parse(cli.TRAIN_FLAGS, base, "launch_train").cvb0_blocks == -1
    assert "3:" in dict((f[0], f[3]) for f in cli.TRAIN_FLAGS)["inference_mode"]


def test_world_size_is_refused_with_mode_3(capsys, monkeypatch):
    from pylda_amd import cli
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert cli.train_main(["--input_directory=in", "--output_directory=out", "--number_of_topics=3", "--training_iterations=1",
                           "--inference_mode=3", "--sampler_seed=1", "--cvb0_blocks=2"]) == 2
    assert "one GPU" in capsys.readouterr().err


def test_class_contract_without_a_gpu():
    from pylda_amd.cvb0 import CollapsedVariationalBayes
    from pylda_amd.inferencer import Inferencer
    assert issubclass(CollapsedVariationalBayes, Inferencer)
    m = CollapsedVariationalBayes(seed=12, blocks=4)
    assert m._sampler_seed == 12 and m._blocks == 4 and m.last_change is None
    assert not hasattr(m, "fold_in")                     # launch_test takes the inference() path
    m._type_to_index = {"a": 0, "b": 1, "c": 2}
    m._verbose = False
    assert m.parse_data(["a b a zz", "zz", "c"]) == [[0, 1, 0], [2]]
    with pytest.raises(ValueError):
        CollapsedVariationalBayes(blocks=0)
    with pytest.raises(NotImplementedError):
        CollapsedVariationalBayes(process_group=object())
    state = m.__getstate__()
    assert state["_ctx"] is None and state["_train_corpus"] is None and state["_sampler_seed"] == 12


# ---------------------------------------------------------------- the C ABI
GROUPS = ("pylda_cvb0_init", "pylda_cvb0_sweep", "pylda_cvb0_log_likelihood", "pylda_cvb0_get_state", "pylda_cvb0_set_state",
          "pylda_cvb0_foldin")


def test_abi_names_the_additions_and_keeps_its_version():
    from pylda_amd import _capi
    text = open(os.path.join(ROOT, "include", "pylda_hip.h")).read()
    assert _capi.ABI_VERSION == 10 and re.search(r"#define PYLDA_ABI_VERSION 10\b", text)
    line = text[text.index(" *  10  additions only"):text.index("A host compiled against another version")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(pylda_[a-z_]*cvb0[a-z0-9_]*)\s*\(", code)))
    assert declared == sorted(_capi.CVB0_SIGNATURES)
    for name in GROUPS:
        assert name in declared and name in line, name
    # (the binding list of the symbols named in letters only is compared with the header by tests/test_capi_symbols.py)
    assert not set(_capi.CVB0_SIGNATURES) & set(_capi.SIGNATURES)


def test_library_exports_the_additions():
    from pylda_amd import _capi, build
    build.build(verbose=False)
    lib = _capi.load()
    for name in _capi.CVB0_SIGNATURES:
        assert hasattr(lib, name), name

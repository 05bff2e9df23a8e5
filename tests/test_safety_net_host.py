"""The cases of tests/test_gpu_safety_net.py, checked where no GPU is needed: every case keeps its margin around the dense
kernels' threshold, the prediction gives the counts the GPU tests assert, the two oracles agree on every case, and the
mpmath golden reproduces from its maker and bounds the C oracle's own error."""
import importlib.util
import os

import numpy as np
import pytest

import safety_net_cases as sc
from conftest import GOLDEN, load_golden
from oracle import c_oracle, vb_numpy

GAMMA_RTOL, LL_RTOL, LL_ATOL, SSTATS_ATOL = 1e-9, 1e-9, 1e-11, 1e-8


def test_every_case_keeps_its_margin():
    for name in sc.NATURAL:
        alpha, eta, ptr, ids, cts = sc.natural_case(name)
        for max_iter, tol in sc.SETTINGS:
            smallest, bad_at = sc.predict_flagged(alpha, eta, ptr, ids, cts, max_iter, tol, sc.scale_at(name, tol))
            assert sc.margin_holds(smallest), (name, max_iter, tol)
            assert np.all(smallest[bad_at > 0] < sc.MARGIN_LOW) and np.all(smallest[bad_at == 0] > sc.MARGIN_HIGH)
    for (alpha, eta, ptr, ids, cts), scale in ((sc.chunk_case(), "sum"), (sc.boundary_case(sc.LARGEST_K), "max")):
        assert sc.margin_holds(sc.predict_flagged(alpha, eta, ptr, ids, cts, scale=scale)[0])
    # the golden's K = 1024 documents without the hook: the one of one token leaves the range at once, the others stay in it
    alpha, eta, ptr, ids, cts = sc.mp_inputs("K1024")
    for max_iter in sc.MP_MAX_ITER:
        smallest, bad_at = sc.predict_flagged(alpha, eta, ptr, ids, cts, max_iter)
        assert sc.margin_holds(smallest) and bad_at.tolist() == [1, 0, 0]


def test_predicted_counts():
    # tests/test_gpu_estep.py::test_collapsed_alpha_triggers_safety_net never reaches the net: under either scale of t the
    # smallest normaliser of its twelve documents is a few hundredths
    alpha, eta, ptr, ids, cts = sc.collapsed_alpha_inputs()
    for scale, floor in (("sum", 4.4e-2), ("max", 6e-2)):
        smallest, bad_at = sc.predict_flagged(alpha, eta, ptr, ids, cts, 3, 1e-6, scale)
        assert not bad_at.any() and floor < smallest.min() < 0.1
    # per (max_iter, tol) of SETTINGS.  K = 1024: six documents of one token in iteration 1, six anchored ones in iteration
    # 2 where there is one and the first does not end the document; threshold 0 goes to the generic kernels, which finish the
    # documents of one token.  K > 1024: the anchored documents alone
    for name in sc.NATURAL:
        want = [12, 6, 12, 6, 6] if sc.NATURAL[name][0] == 1024 else [6, 0, 6, 0, 6]
        assert [len(sc.natural_flagged(name, m, tol)) for m, tol in sc.SETTINGS] == want, name
        D = len(sc.natural_case(name)[2]) - 1
        assert 0 < len(sc.natural_flagged(name)) < D
    # the issue's table, for the kernels that scale t by psi(sum gamma): K >= 1024 flags one token, 2000 up to two
    alpha, eta, ptr, ids, cts = sc.natural_case("K2000_a1e-4")
    few = sc.csr([([20], [n]) for n in (1, 2, 3)])
    assert sc.predict_flagged(alpha, eta, *few, scale="sum")[1].tolist() == [1, 1, 0]
    assert sc.predict_flagged(alpha, eta, *few, scale="max")[1].tolist() == [0, 0, 0]
    assert sc.LARGEST_K == 3325 and sc.logspace_launch_bytes(3389) <= sc.LDS_BYTES < sc.logspace_launch_bytes(3390)


def agree(a, b, heldout, what, case=None):
    assert np.array_equal(a["iters"], b["iters"]), what
    assert np.max(np.abs(a["gamma"] - b["gamma"]) / np.abs(b["gamma"])) < GAMMA_RTOL, what
    key = "doc_words_ll" if heldout else "doc_ll"
    assert np.all(np.abs(a[key] - b[key]) <= LL_RTOL * np.abs(b[key]) + LL_ATOL), what
    if not heldout:
        bar = sc.statistics_bar(case[1].shape[1], case[3], case[4]) if case is not None else SSTATS_ATOL
        assert np.all(np.abs(a["sstats"] - b["sstats"]) < bar), what


HELDOUT_OF_SETTING = (False, True, False, True, False)          # the mode each of SETTINGS runs in besides (50, 1e-6) in both


def oracles_agree(case, settings, what):
    for (max_iter, tol), heldout in settings:
        agree(c_oracle.e_step(*case, max_iter=max_iter, tol=tol, heldout=heldout),
              vb_numpy.e_step(*case, max_iter=max_iter, tol=tol, heldout=heldout), heldout, (what, max_iter, tol, heldout), case)


@pytest.mark.parametrize("name", list(sc.NATURAL) + ["boundary"])
def test_the_two_oracles_agree_where_documents_are_flagged(name):
    case = sc.natural_case(name) if name in sc.NATURAL else sc.boundary_case(sc.LARGEST_K)
    oracles_agree(case, list(zip(sc.SETTINGS, HELDOUT_OF_SETTING)) + [(sc.SETTINGS[0], True)], name)


@pytest.mark.parametrize("K", sc.BRANCH_K)
def test_the_two_oracles_agree_at_the_log_space_kernels_strides(K):
    case = sc.branch_case(K)
    assert np.array_equal(np.diff(case[2]), [min(n, 300) if K >= 700 else n for n in sc.BRANCH_LENGTHS]) and case[4].max() == 10 ** 6
    oracles_agree(case, list(zip(sc.SETTINGS, HELDOUT_OF_SETTING)) + [(sc.SETTINGS[0], True)], K)


def test_the_two_oracles_agree_on_the_long_corpus():
    oracles_agree(sc.chunk_case(), [(sc.SETTINGS[0], False), (sc.SETTINGS[0], True)], "chunk")


@pytest.mark.parametrize("K", (128, 256, 400))
def test_the_two_oracles_agree_on_the_guard_cases(K):
    oracles_agree(sc.guard_case(K), [(sc.SETTINGS[0], False), (sc.SETTINGS[0], True)], ("guard", K))


def test_the_two_oracles_agree_on_the_goldens_inputs():
    for name in (c[0] for c in sc.MP_CASES):
        oracles_agree(sc.mp_inputs(name), [((m, 1e-6), h) for m in sc.MP_MAX_ITER for h in (False, True)], name)


def maker():
    spec = importlib.util.spec_from_file_location("make_logspace_mp", os.path.join(GOLDEN, "make_logspace_mp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_golden_reproduces_from_its_maker():
    pytest.importorskip("mpmath")
    g, mod = load_golden("logspace_mp.npz"), maker()
    for name, max_iter in (("K1", 50), ("K1", 1), ("K65", 1)):
        got = mod.compute(name, max_iter)
        for key, value in got.items():
            assert np.array_equal(g["%s_m%d_%s" % (name, max_iter, key)], value), (name, max_iter, key)
    assert sorted(g) == sorted("%s_m%d_%s" % (c[0], m, key) for c in sc.MP_CASES for m in sc.MP_MAX_ITER
                               for key in ("gamma", "doc_ll", "words_ll", "sstats", "iters", "stop_margin"))


def test_c_oracle_against_the_golden():
    """The fp64 oracle's own distance to mpmath, on the golden's cases: inside the bars the device is held to (if it were
    not, the case would be wrong for the bar).  LABNOTES.md records the figures printed here."""
    g = load_golden("logspace_mp.npz")
    for name, K, lengths, _, _ in sc.MP_CASES:
        case = sc.mp_inputs(name)
        assert np.array_equal(np.diff(case[2]), lengths) and case[1].shape[0] == K
        for max_iter in sc.MP_MAX_ITER:
            ref = {key: g["%s_m%d_%s" % (name, max_iter, key)] for key in ("gamma", "doc_ll", "words_ll", "sstats", "iters", "stop_margin")}
            assert np.all(ref["stop_margin"] > 1e-6)
            train = c_oracle.e_step(*case, max_iter=max_iter)
            held = c_oracle.e_step(*case, max_iter=max_iter, heldout=True)
            assert np.array_equal(train["iters"], ref["iters"]) and np.array_equal(held["iters"], ref["iters"])
            gamma = np.max(np.abs(train["gamma"] - ref["gamma"]) / ref["gamma"])
            ll = np.max(np.abs(train["doc_ll"] - ref["doc_ll"]) / np.maximum(np.abs(ref["doc_ll"]), 1e-300))
            wll = np.max(np.abs(held["doc_words_ll"] - ref["words_ll"]) / np.abs(ref["words_ll"]))
            sstats = np.max(np.abs(train["sstats"] - ref["sstats"]))
            print("%s max_iter %d: C oracle against mpmath: gamma %.2e rel, doc_ll %.2e rel, words_ll %.2e rel, statistics %.2e abs"
                  % (name, max_iter, gamma, ll, wll, sstats))
            assert gamma < GAMMA_RTOL and sstats < SSTATS_ATOL
            assert np.all(np.abs(train["doc_ll"] - ref["doc_ll"]) <= LL_RTOL * np.abs(ref["doc_ll"]) + LL_ATOL)
            assert np.all(np.abs(held["doc_words_ll"] - ref["words_ll"]) <= LL_RTOL * np.abs(ref["words_ll"]) + LL_ATOL)

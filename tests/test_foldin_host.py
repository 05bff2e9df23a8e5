"""CPU-side checks of the held-out fold-in: the numpy restatement (tests/foldin_restatement.py) against
an exact enumeration of a tiny posterior, the command line's flags and the kernels' resources."""
import os
import sys

import numpy as np
import pytest

import foldin_fixture as fixture
import foldin_restatement as spec
from conftest import ROOT


def _restated(seed=11, alpha=fixture.ALPHA, **changes):
    return spec.fold_in(*fixture.corpus(), fixture.table(), alpha, seed, 2 ** 31, fixture.SWEEPS, fixture.BURN_IN, **changes)["gamma"]


def test_the_enumeration_gives_the_expected_counts():
    exact = fixture.exact_counts()
    assert abs(exact.sum() - len(fixture.WORDS)) < 1e-12
    assert np.max(np.abs(exact - fixture.EXPECTED)) < 1e-4, exact


def test_restatement_follows_the_exact_posterior():
    """4000 replicas (global documents 0..3999), 100 sweeps, burn-in 40: each topic's mean of gamma - alpha within 5 standard
    errors (across the replicas) of the exact E[n_dk].  A plain-numpy version of this chain gave a largest |z| of 3.1 over
    eight seeds; with the own token left in the counts z was 22 to 46, with alpha scaled by 1.5 it was 10 to 24: the two
    tests below hold the restatement to that."""
    z = fixture.z_scores(_restated())
    print("z per topic:", np.round(z, 2))
    assert np.all(np.abs(z) < 5.0), z


def test_the_posterior_test_sees_a_token_left_in_its_counts():
    z = fixture.z_scores(_restated(remove_own=False))
    print("z per topic:", np.round(z, 2))
    assert np.max(np.abs(z)) > 5.0, z


def test_the_posterior_test_sees_a_scaled_alpha():
    z = fixture.z_scores(_restated(alpha=1.5 * fixture.ALPHA), alpha=1.5 * fixture.ALPHA)
    print("z per topic:", np.round(z, 2))
    assert np.max(np.abs(z)) > 5.0, z


def test_restatement_edges_and_determinism():
    """An empty document keeps gamma = alpha and a likelihood of 0; the same names give the same bits, another stream does not;
    a shard given its offset draws what the whole corpus draws."""
    P, alpha = fixture.table(), fixture.ALPHA
    ptr = np.array([0, 2, 2, 5], dtype=np.int64)
    ids, cts = np.array([0, 3, 1, 2, 4]), np.array([2, 1, 1, 3, 1])
    a = spec.fold_in(ptr, ids, cts, P, alpha, 5, 9, 6, 2)
    assert np.array_equal(a["gamma"][1], alpha) and a["doc_words_ll"][1] == 0.0
    assert np.allclose(a["gamma"].sum(axis=1) - alpha.sum(), [3, 0, 5], rtol=0, atol=1e-12)
    b = spec.fold_in(ptr, ids, cts, P, alpha, 5, 9, 6, 2)
    assert np.array_equal(a["gamma"], b["gamma"]) and a["words_log_likelihood"] == b["words_log_likelihood"]
    fix = fixture.corpus(64)
    whole = spec.fold_in(*fix, P, alpha, 5, 9, 10, 5)
    other = spec.fold_in(*fix, P, alpha, 5, 10, 10, 5)
    assert not np.array_equal(whole["gamma"], other["gamma"])
    half = spec.fold_in(fix[0][:33], fix[1][:fix[0][32]], fix[2][:fix[0][32]], P, alpha, 5, 9, 10, 5, first_document=32)
    assert np.array_equal(half["gamma"], whole["gamma"][32:])
    assert abs(whole["words_log_likelihood"] - np.sum(whole["doc_words_ll"])) < 1e-9


def test_launch_test_has_the_fold_in_flags():
    from pylda_amd import cli
    base = ["--input_directory=in", "--model_directory=out"]
    opt = cli._parse(cli.TEST_FLAGS, base, "launch_test")
    assert opt.fold_in_samples == -1 and opt.fold_in_burn_in == -1
    opt = cli._parse(cli.TEST_FLAGS, base + ["--fold_in_samples=20", "--fold_in_burn_in=4"], "launch_test")
    assert opt.fold_in_samples == 20 and opt.fold_in_burn_in == 4


def test_monte_carlo_has_fold_in_and_keeps_inference_closed():
    from pylda_amd.monte_carlo import FOLD_IN_STREAM_BASE, MonteCarlo
    m = MonteCarlo(seed=3)
    assert callable(m.fold_in) and FOLD_IN_STREAM_BASE == 2 ** 31 and m.__getstate__()["_fold_in_calls"] == 0
    with pytest.raises(NotImplementedError):
        m.inference(["a b"])


def test_foldin_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    path = kr.compile_to_asm(os.path.join(ROOT, "pylda_amd", "csrc", "launch_foldin.hip"))
    lines = open(path).read().splitlines()
    res = kr.resources(lines, "foldin")
    names = kr.demangle(list(res))
    found = sorted(names[k] for k in res)
    assert len([n for n in found if "foldin_sample_kernel" in n]) == 5, found       # 1, 2, 4, 8, 16 topics per lane
    for wanted in ("foldin_table_kernel", "foldin_sum_kernel"):
        assert any(wanted in n for n in found), (wanted, found)
    for k, info in res.items():
        assert info["ScratchSize"] == 0, (names[k], info)
        assert info["NumVgprs"] <= 256, (names[k], info)

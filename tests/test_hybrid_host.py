"""CPU-side checks of the hybrid E-step: the numpy Philox against the Random123 known answers, the restatement's
contract (tests/hybrid_restatement.py), the mode-0 command line's refusals, and the sampler kernels' resources."""
import os
import sys

import numpy as np
import pytest

import hybrid_restatement as spec
from conftest import ROOT, load_golden
from hybrid_golden_checks import moment_failures, replicated_document

KNOWN_ANSWERS = [
    ((0, 0, 0, 0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 6, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("inputs,expected", KNOWN_ANSWERS)
def test_numpy_philox_known_answers(inputs, expected):
    assert tuple(int(x) for x in spec.philox4x32_10(*inputs)) == expected


def test_uniform_is_in_the_unit_interval_and_uniform():
    u = spec.uniform(np.arange(200000, dtype=np.uint64), 5 << 16, 3, 1, 123)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) < 0.005 and abs(u.var() - 1.0 / 12) < 0.002


def test_restatement_contract_on_tiny(tiny):
    """Shapes and bookkeeping of hybrid.py:85-171 on the two-topic fixture: gamma rows sum to sum(alpha) + N_d, the
    statistics hold (samples - burn-in) / (samples - burn-in) = one count per token, the per-document likelihoods add
    up to the returned scalar."""
    ptr, ids, cts = tiny["doc_ptr"], tiny["term_id"], tiny["term_ct"]
    alpha, eta = tiny["alpha"], tiny["eta"]
    K, V = eta.shape
    D = len(ptr) - 1
    r = spec.hybrid_estep(ptr, ids, cts, alpha, eta, seed=1, stream=0)
    n_d = np.add.reduceat(cts, ptr[:-1])
    assert r["gamma"].shape == (D, K) and r["sstats"].shape == (K, V)
    assert np.allclose(r["gamma"].sum(axis=1), alpha.sum() + n_d, rtol=1e-12)
    assert np.allclose(r["sstats"].sum(axis=0), np.bincount(ids, weights=cts, minlength=V))
    assert np.all(r["counts"] == np.round(r["counts"]))
    assert abs(r["document_log_likelihood"] - r["doc_ll"].sum()) < 1e-9 and np.all(r["doc_words_ll"] == 0)
    h = spec.hybrid_estep(ptr, ids, cts, alpha, eta, seed=1, stream=2 ** 31, heldout=True)
    assert np.all(h["doc_words_ll"] < 0)
    again = spec.hybrid_estep(ptr, ids, cts, alpha, eta, seed=1, stream=0)
    assert np.array_equal(again["gamma"], r["gamma"])


def test_restatement_samples_the_collapsed_conditional():
    """One token per document and no other tokens: the chain's draw is then exactly from alpha * B[w] normalised, so
    the topic frequencies over many replicated documents follow it."""
    K, V, D = 4, 3, 4000
    alpha = np.array([0.1, 0.5, 1.0, 2.0])
    eta = np.random.default_rng(0).gamma(5.0, 1.0, (K, V))
    ptr, ids, cts = np.arange(D + 1), np.full(D, 1, np.int32), np.ones(D, np.int32)
    r = spec.hybrid_estep(ptr, ids, cts, alpha, eta, seed=3, number_of_samples=2, burn_in_samples=1)
    B, _ = spec.shifted_table(eta)
    p = alpha * B[1]
    p /= p.sum()
    freq = r["counts"][:, 1] / D
    assert np.all(np.abs(freq - p) < 5 * np.sqrt(p * (1 - p) / D)), (freq, p)


def test_mode_0_needs_a_seed_and_mode_1_is_refused(capsys):
    from pylda_amd import cli
    base = ["--input_directory=in", "--output_directory=out", "--number_of_topics=3", "--training_iterations=1"]
    assert cli.train_main(base + ["--inference_mode=0"]) == 2
    assert "--sampler_seed" in capsys.readouterr().err
    assert cli.train_main(base + ["--inference_mode=1", "--sampler_seed=4"]) == 2
    opt = cli._parse(cli.TRAIN_FLAGS, base + ["--inference_mode=0", "--sampler_seed=7"], "launch_train")
    assert opt.sampler_seed == 7 and opt.inference_mode == 0
    assert cli._parse(cli.TRAIN_FLAGS, base, "launch_train").sampler_seed == -1


def test_hybrid_class_contract_without_a_gpu():
    from pylda_amd.hybrid import Hybrid, _grouped_csr
    from pylda_amd.variational_bayes import VariationalBayes
    assert issubclass(Hybrid, VariationalBayes)
    m = Hybrid(seed=12)
    assert m._sampler_seed == 12 and m._hyper_parameter_optimize_interval == 1
    m._type_to_index = {"a": 0, "b": 1, "c": 2}
    m._verbose = False
    assert m.parse_data(["a b a zz", "zz", "c"]) == [[0, 1, 0], [2]]
    ptr, ids, cts = _grouped_csr([[0, 1, 0], [2]])
    assert list(ptr) == [0, 2, 3] and list(ids) == [0, 1, 2] and list(cts) == [2, 1, 1]
    os.environ["PYLDA_SEED"] = "99"
    try:
        assert Hybrid()._sampler_seed == 99
    finally:
        del os.environ["PYLDA_SEED"]


def test_sampler_and_statistics_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    path = kr.compile_to_asm(os.path.join(ROOT, "pylda_amd", "csrc", "launch_hybrid.hip"))
    lines = open(path).read().splitlines()
    res = kr.resources(lines, "hybrid")
    names = kr.demangle(list(res))
    found = sorted(names[k] for k in res)
    assert len([n for n in found if "hybrid_sample_kernel" in n]) == 5, found       # 1, 2, 4, 8, 16 topics per lane
    assert any("hybrid_sstats_kernel" in n for n in found), found
    for k, info in res.items():
        assert info["ScratchSize"] == 0, (names[k], info)
        assert info["NumVgprs"] <= 256, (names[k], info)


@pytest.mark.parametrize("heldout", [False, True])
def test_restatement_moments_match_the_reference_hybrid(heldout):
    """The restatement's chain against the reference's hybrid.py (tests/golden/hybrid_moments_k8.npz): one 60-token
    document replicated 4000 times; gamma, the likelihood per batch of 200 and the statistics within 5 sigma."""
    g = load_golden("hybrid_moments_k8.npz")
    ptr, ids, cts = replicated_document(g)
    r = spec.hybrid_estep(ptr, ids, cts, g["alpha"], g["eta"], seed=4321, stream=2 ** 31 if heldout else 1, heldout=heldout)
    stats = None if heldout else r["sstats"][:, g["terms"]] / float(g["replicas"])
    assert moment_failures(g, "heldout" if heldout else "train", r["gamma"], r["doc_words_ll"] if heldout else r["doc_ll"],
                           stats) == []

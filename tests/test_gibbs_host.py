"""CPU-side checks of the collapsed Gibbs engine (inference mode 1): the numpy restatement (tests/gibbs_restatement.py)
against the reference's monte_carlo.py (goldens of tests/golden/make_gibbs_golden.py), the host hyper-parameter step, the
chain's invariants, the command line's refusals and the kernels' resources."""
import os
import sys

import numpy as np
import pytest

import gibbs_golden_checks as checks
import gibbs_restatement as spec
from conftest import ROOT, load_golden, rel_err

POSTERIOR_STATES = ("A", "B")


@pytest.mark.parametrize("name", POSTERIOR_STATES)
def test_restatement_log_posterior_matches_the_reference(name):
    g = load_golden("gibbs_posterior.npz")
    n_dk, n_kv = g[name + "_n_dk"].astype(np.int64), g[name + "_n_kv"].astype(np.int64)
    K, V = n_kv.shape
    assert rel_err(spec.log_posterior(n_dk, n_kv, g[name + "_alpha"], g[name + "_beta"]), g[name + "_lp"]) < 1e-10
    assert rel_err(spec.log_posterior(n_dk, n_kv, np.zeros(K) + 1.0 / K, np.zeros(V) + 1.0 / V), g[name + "_lp_flat"]) < 1e-10


@pytest.mark.parametrize("name,symmetric", [("A", True), ("A", False), ("B", True)])
def test_host_hyper_parameter_step_matches_the_reference(name, symmetric):
    """optimize_hyperparameters (monte_carlo.py:106-212) with the restatement's log_posterior plugged in: the same counts
    and the same numpy stream give the reference's alpha and beta, its aliased arrays included."""
    from pylda_amd.monte_carlo import slice_sample_hyperparameters
    g = load_golden("gibbs_posterior.npz")
    n_dk, n_kv = g[name + "_n_dk"].astype(np.int64), g[name + "_n_kv"].astype(np.int64)
    tag = "%s_opt_%s_" % (name, "sym" if symmetric else "vec")
    moved = False
    for i, seed in enumerate(g["opt_seeds"]):
        np.random.seed(int(seed))
        alpha, beta = slice_sample_hyperparameters(lambda a, b: spec.log_posterior(n_dk, n_kv, a, b), g[name + "_alpha"],
                                                   g[name + "_beta"], symmetric, symmetric)
        assert rel_err(alpha, g[tag + "alpha"][i]) < 1e-10 and rel_err(beta, g[tag + "beta"][i]) < 1e-10, seed
        moved = moved or not np.array_equal(alpha, g[name + "_alpha"])
    if symmetric:
        assert moved        # (the golden does pin an accepted proposal, not only the start)


def _tiny_chains(replicas=2000, **changes):
    g = load_golden("gibbs_sequential_k3.npz")
    ptr, ids, cts = checks.tiny_corpus(g)
    K, V, alpha, beta = int(g["K"]), int(g["V"]), float(g["alpha"]), float(g["beta"])
    chain = spec.GibbsChain(ptr, ids, cts, K, V, seed=0, replicas=replicas, remove_own=changes.get("remove_own", True))
    chain.init()
    marks, out = [int(m) for m in g["marks"]], []
    for it in range(1, marks[-1] + 1):
        chain.sweep(alpha * changes.get("alpha_scale", 1.0), beta, len(ptr) - 1, it)      # blocks = D: one document per round
        if it in marks:
            out.append(checks.chain_statistics(chain, alpha, beta))
    bad = []
    names = [str(n) for n in g["stat_names"]]
    for i, mark in enumerate(marks):
        bad += checks.moment_failures(g["stats"][:, i, :], out[i], names, "iteration %d" % mark)
    return bad


def test_sequential_restatement_follows_the_reference_chain():
    """blocks >= D is the reference's sampler up to the token order and the way a topic is picked from the weights: 2000
    chains (seeds 0..1999) against the reference's seeds, means within 5 sigma and variances within 5 standard errors."""
    assert _tiny_chains() == []


def test_the_moments_test_sees_a_token_left_in_its_counts():
    bad = _tiny_chains(remove_own=False)
    print("\n".join(bad))
    assert bad


def test_the_moments_test_sees_a_scaled_alpha():
    bad = _tiny_chains(alpha_scale=1.5)
    print("\n".join(bad))
    assert bad


def _trace(ap_train, blocks, replicas, seed):
    ptr, ids, cts = checks.first_documents(ap_train, 300)
    K, V = 10, len(ap_train["words"])
    chain = spec.GibbsChain(ptr, ids, cts, K, V, seed=seed, replicas=replicas)
    chain.init()
    trace = []
    for it in range(1, 61):
        chain.sweep(1.0 / K, 1.0 / V, blocks, it)
        if it >= checks.TRACE_FROM:
            trace.append([chain.log_posterior(1.0 / K, 1.0 / V, r) for r in range(replicas)])
    return np.mean(trace, axis=0)


def test_trace_of_the_block_synchronous_chain_against_the_reference(ap_train):
    """S = mean log posterior over iterations 41..60 on the first 300 associated-press documents, K = 10, against the
    band of the reference's eight seeds: 64 blocks inside it (three seeds), one block (counts frozen for a whole sweep)
    below it, the default of 16 between the two (its value is printed and recorded in DESIGN.md section 11)."""
    lo, hi = checks.trace_band(load_golden("gibbs_trace_k10.npz"))
    s64 = _trace(ap_train, 64, 3, seed=100)
    s1 = _trace(ap_train, 1, 1, seed=100)
    s16 = _trace(ap_train, 16, 1, seed=100)
    print("band [%.0f, %.0f]; S: 64 blocks %s, 16 blocks %s, 1 block %s" % (lo, hi, np.round(s64), np.round(s16), np.round(s1)))
    assert np.all((s64 >= lo) & (s64 <= hi)), (s64, lo, hi)
    assert np.all(s1 < lo), (s1, lo)
    assert np.all((s16 > s1.max()) & (s16 <= hi)), (s16, s1, hi)


def test_invariants_and_determinism_of_the_restatement(ap_train):
    ptr, ids, cts = checks.first_documents(ap_train, 60)
    K, V = 10, len(ap_train["words"])
    term_totals = np.bincount(ids, weights=cts, minlength=V)
    lengths = np.add.reduceat(cts, ptr[:-1])

    def run(seed, blocks, sweeps=3):
        chain = spec.GibbsChain(ptr, ids, cts, K, V, seed=seed)
        chain.init()
        for it in range(1, sweeps + 1):
            chain.sweep(0.1, 0.01, blocks, it)
            n_kv = chain.n_kv()
            assert np.array_equal(n_kv.sum(axis=0), term_totals) and np.array_equal(chain.n_dk.sum(axis=1), lengths)
            assert np.array_equal(chain.n_k[0], n_kv.sum(axis=1))
            assert n_kv.min() >= 0 and chain.n_dk.min() >= 0
            fresh = spec.GibbsChain(ptr, ids, cts, K, V, seed=seed)
            fresh.z[:] = chain.z
            fresh.recount()
            assert np.array_equal(fresh.T, chain.T) and np.array_equal(fresh.n_dk, chain.n_dk)
        return chain.z.copy()
    base = run(5, 4)
    assert np.array_equal(base, run(5, 4))
    assert not np.array_equal(base, run(6, 4)) and not np.array_equal(base, run(5, 8))


def test_a_shard_draws_what_the_whole_corpus_draws(ap_train):
    """A draw is named by the GLOBAL document index: the second half of a corpus, given its offset and the whole corpus'
    counts, samples the same topics in a round as the whole corpus does."""
    ptr, ids, cts = checks.first_documents(ap_train, 40)
    K, V = 10, len(ap_train["words"])
    whole = spec.GibbsChain(ptr, ids, cts, K, V, seed=9)
    whole.init()
    cut = int(ptr[20])
    half = spec.GibbsChain(ptr[20:] - cut, ids[cut:], cts[cut:], K, V, seed=9, first_document=20)
    half.init()
    first_token = int(np.sum(cts[:cut]))
    assert np.array_equal(half.z, whole.z[first_token:])
    half.T[:], half.n_k[:] = whole.T, whole.n_k
    whole.sweep(0.1, 0.01, 1, 1)
    half.sweep(0.1, 0.01, 1, 1)
    assert np.array_equal(half.z, whole.z[first_token:])


def test_mode_1_needs_its_two_flags_and_one_gpu(capsys):
    from pylda_amd import cli
    base = ["--input_directory=in", "--output_directory=out", "--number_of_topics=3", "--training_iterations=1",
            "--inference_mode=1"]
    assert cli.train_main(base + ["--sampler_seed=4"]) == 2
    err = capsys.readouterr().err
    assert "--gibbs_blocks" in err and "approximation" in err and "rounds" in err
    assert cli.train_main(base + ["--gibbs_blocks=16"]) == 2
    assert "--sampler_seed" in capsys.readouterr().err
    assert cli.train_main(base + ["--sampler_seed=4", "--gibbs_blocks=0"]) == 2
    capsys.readouterr()
    assert cli.train_main(base + ["--sampler_seed=4", "--gibbs_blocks=16", "--gpus=2"]) == 2
    assert "one GPU" in capsys.readouterr().err
    opt = cli._parse(cli.TRAIN_FLAGS, base + ["--sampler_seed=7", "--gibbs_blocks=64"], "launch_train")
    assert opt.sampler_seed == 7 and opt.gibbs_blocks == 64 and opt.inference_mode == 1
    assert cli._parse(cli.TRAIN_FLAGS, base, "launch_train").gibbs_blocks == -1


def test_monte_carlo_class_contract_without_a_gpu():
    from pylda_amd.inferencer import Inferencer
    from pylda_amd.monte_carlo import MonteCarlo
    assert issubclass(MonteCarlo, Inferencer)
    m = MonteCarlo(seed=12)
    assert m._sampler_seed == 12 and m._blocks == 16 and m._hyper_parameter_optimize_interval == 10
    assert m._symmetric_alpha_alpha and m._symmetric_alpha_beta
    m._type_to_index = {"a": 0, "b": 1, "c": 2}
    m._verbose = False
    assert m.parse_data(["a b a zz", "zz", "c"]) == [[0, 1, 0], [2]]
    with pytest.raises(NotImplementedError):
        m.inference(["a b"])
    with pytest.raises(ValueError):
        MonteCarlo(blocks=0)
    assert not hasattr(m, "sample_document")
    state = m.__getstate__()
    assert state["_ctx"] is None and state["_train_corpus"] is None and state["_sampler_seed"] == 12


def test_gibbs_kernels_have_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    path = kr.compile_to_asm(os.path.join(ROOT, "pylda_amd", "csrc", "launch_gibbs.hip"))
    lines = open(path).read().splitlines()
    res = kr.resources(lines, "gibbs")
    names = kr.demangle(list(res))
    found = sorted(names[k] for k in res)
    assert len([n for n in found if "gibbs_sample_kernel" in n]) == 5, found       # 1, 2, 4, 8, 16 topics per lane
    for wanted in ("gibbs_init_kernel", "gibbs_apply_kernel", "gibbs_doc_posterior_kernel", "gibbs_word_posterior_kernel"):
        assert any(wanted in n for n in found), (wanted, found)
    for k, info in res.items():
        assert info["ScratchSize"] == 0, (names[k], info)
        assert info["NumVgprs"] <= 256, (names[k], info)

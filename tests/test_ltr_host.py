"""The left-to-right held-out likelihood without a GPU: its numpy restatement (tests/ltr_restatement.py,
what the kernels are held to draw for draw) against the enumerated p(w) of the K = 3, V = 5 fixture, against the algorithm
as the paper prints it, and against closed forms; the entry points in header and binding, the engines' method, the command
line's flags, and the kernels' resources from the compiler's own assembly."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

import foldin_fixture as fx
import ltr_fixture as lf
import ltr_restatement as spec
from conftest import ROOT

SEED, STREAM = 20240607, 3 << 30
PAPER_REPLICAS = 6000


def _estimates(words, resample, particles=1, replicas=lf.REPLICAS, alpha=fx.ALPHA, **kw):
    return spec.left_to_right(*lf.corpus(words, replicas), fx.table(), alpha, particles, resample, SEED, STREAM, **kw)["doc_ll"]


def _exact(words):
    return lf.exact_probability(words, fx.table(), fx.ALPHA)


# ---------------------------------------------------------------- exact, by enumeration
def test_sequential_sampler_is_unbiased_on_the_seven_token_document():
    """resample=False, R = 1, 1600 replicas (global documents 0 .. 1599): mean exp(ll) within 5 standard errors of the
    enumerated p(w) = 1.9376e-06 (standard error 0.8 % of it).  z = -0.66."""
    z = lf.z_score(np.exp(_estimates(lf.SEVEN, False)), _exact(lf.SEVEN))
    print("z", round(z, 2))
    assert abs(z) < 5.0


@pytest.mark.parametrize("resample", [False, True])
def test_both_modes_are_unbiased_on_the_two_token_document(resample):
    """Two copies of word 4: the first topic is drawn from its exact posterior and resampling leaves it there, so
    exp(ll) is unbiased at R = 1 in both modes.  z = 0.45 without resampling, -0.53 with."""
    z = lf.z_score(np.exp(_estimates(lf.TWO, resample)), _exact(lf.TWO))
    print("z", round(z, 2))
    assert abs(z) < 5.0


def test_the_enumeration_test_sees_a_token_left_in_its_counts():
    """The two-token test with the own token left in the counts while it is drawn again: z = 7.89."""
    z = lf.z_score(np.exp(_estimates(lf.TWO, True, remove_own=False)), _exact(lf.TWO))
    print("z", round(z, 2))
    assert abs(z) > 5.0


@pytest.mark.parametrize("words,resample", [(lf.SEVEN, False), (lf.TWO, False), (lf.TWO, True)])
def test_the_enumeration_test_sees_a_scaled_alpha(words, resample):
    """The chains run with 1.5 alpha, the exact value with alpha: z = 6.56 (seven tokens), -11.73 and -12.74 (two tokens)."""
    z = lf.z_score(np.exp(_estimates(words, resample, alpha=1.5 * fx.ALPHA)), _exact(words))
    print("z", round(z, 2))
    assert abs(z) > 5.0


# ---------------------------------------------------------------- against the paper
def _joint_z(values, reference):
    return float((values.mean() - reference.mean()) / np.sqrt(values.var(ddof=1) / len(values) + reference.var(ddof=1) / len(reference)))


@pytest.fixture(scope="module")
def paper():
    """6000 runs of Algorithm 3 as printed (R = 8, the seven-token document), numpy's own generator."""
    return lf.paper_algorithm_3(lf.SEVEN, fx.table(), fx.ALPHA, 8, PAPER_REPLICAS, np.random.default_rng(5))


def test_resampling_agrees_with_the_algorithm_as_printed(paper):
    """resample=True, R = 8, 6000 replicas each: the mean ll within 5 joint standard errors.  z = 0.49 (both means are
    about -13.153, log p(w) = -13.1541)."""
    z = _joint_z(_estimates(lf.SEVEN, True, 8, PAPER_REPLICAS), paper)
    print("z", round(z, 2))
    assert abs(z) < 5.0


def test_the_paper_test_sees_a_token_left_in_its_counts(paper):
    """z = 10.46 with the own token left in the counts while it is drawn again (3000 replicas each gave 5.1 to 7.8 over two
    seeds, hence 6000)."""
    own = _joint_z(_estimates(lf.SEVEN, True, 8, PAPER_REPLICAS, remove_own=False), paper)
    print("z", round(own, 2))
    assert abs(own) > 5.0


# ---------------------------------------------------------------- closed forms
def _table(rng, V, K):
    P = rng.gamma(0.3, size=(K, V)) + 1e-6
    return (P / P.sum(axis=1, keepdims=True)).T.copy()


def _within_bar(out, want, K, R):
    bar = spec.bar(K, R, out["doc_tok"], want, out["abs_logs"])
    assert np.all(np.abs(out["doc_ll"] - want) <= bar), (out["doc_ll"] - want, bar)


@pytest.mark.parametrize("resample", [0, 1])
def test_one_topic(resample):
    """K = 1: every topic is topic 0 and ll = sum_n c_n log P[w_n][0]."""
    rng = np.random.default_rng(1)
    P = _table(rng, 9, 1)
    ptr, ids, cts = [0, 3, 4], [2, 8, 0, 5], [4, 1, 2, 3]
    out = spec.left_to_right(ptr, ids, cts, P, [0.7], 3, resample, SEED, STREAM)
    want = np.array([np.sum(np.array(cts[:3]) * np.log(P[ids[:3], 0])), cts[3] * np.log(P[5, 0])])
    assert np.all(out["z"] == 0)
    _within_bar(out, want, 1, 3)


def test_one_token():
    """A one-token document: log(sum_k alpha_k P[w][k] / alpha_sum), whatever the mode or the draws."""
    rng = np.random.default_rng(2)
    P, alpha = _table(rng, 7, 10), rng.gamma(1.0, size=10)
    for resample in (0, 1):
        out = spec.left_to_right([0, 1, 2], [6, 3], [1, 1], P, alpha, 5, resample, SEED, STREAM)
        want = np.log(np.array([np.sum(alpha * P[6]), np.sum(alpha * P[3])]) / alpha.sum())
        _within_bar(out, want, 10, 5)


@pytest.mark.parametrize("resample", [0, 1])
def test_rows_constant_over_the_topics(resample):
    """P[w][k] = c_w for every k: p_n = c_w (n + alpha_sum) / (n + alpha_sum), so ll = sum_n c_n log P[w_n][0] whatever is drawn."""
    rng = np.random.default_rng(3)
    P = np.repeat(rng.dirichlet(np.ones(6))[:, np.newaxis], 65, axis=1)
    alpha = rng.gamma(0.5, size=65)
    ptr, ids, cts = [0, 2, 2, 5], [1, 4, 0, 5, 3], [2, 3, 1, 1, 7]
    out = spec.left_to_right(ptr, ids, cts, P, alpha, 4, resample, SEED, STREAM)
    per_term = np.array(cts) * np.log(P[ids, 0])
    want = np.array([per_term[:2].sum(), 0.0, per_term[2:].sum()])
    assert out["doc_ll"][1] == 0.0 and out["tokens"] == 14
    _within_bar(out, want, 65, 4)


def test_draws_are_named_by_the_global_document_and_the_particle():
    """The same documents dealt to two corpora with first_document offsets, and a particle taken as a call of its own on
    its own stream: the same bits."""
    rng = np.random.default_rng(4)
    P, alpha = _table(rng, 12, 10), rng.gamma(0.5, size=10)
    ptr, ids, cts = np.array([0, 2, 3, 6]), np.array([1, 4, 0, 5, 3, 11]), np.array([2, 3, 1, 1, 2, 1])
    whole = spec.left_to_right(ptr, ids, cts, P, alpha, 2, 1, SEED, STREAM)
    tail = spec.left_to_right(ptr[1:] - ptr[1], ids[2:], cts[2:], P, alpha, 2, 1, SEED, STREAM, first_document=1)
    assert np.array_equal(whole["doc_ll"][1:], tail["doc_ll"])
    second = spec.left_to_right(ptr, ids, cts, P, alpha, 1, 1, SEED, STREAM + 1)
    assert np.array_equal(whole["p"].reshape(-1, 2)[:, 1], second["p"])


# ---------------------------------------------------------------- plumbing
def test_header_and_binding_carry_the_two_entry_points_inside_version_10():
    from pylda_amd import _capi
    header = open(os.path.join(ROOT, "include", "pylda_hip.h")).read()
    assert re.search(r"#define PYLDA_ABI_VERSION (\d+)", header).group(1) == str(_capi.ABI_VERSION) == "10"
    changelog = header[header.index(" *  10  additions only"):header.index("A host compiled against another version")]
    for name in ("pylda_left_to_right", "pylda_test_left_to_right_state"):
        assert re.search(r"\bint %s\(" % name, header) and name in _capi.SIGNATURES and name in changelog
    assert len(_capi.SIGNATURES["pylda_left_to_right"][1]) == 11 and len(_capi.SIGNATURES["pylda_test_left_to_right_state"][1]) == 5
    assert callable(_capi.Context.left_to_right) and callable(_capi.Context.test_left_to_right_state)
    assert "ltr_chunk_tokens" in header


def test_engines_offer_the_method_with_the_stated_defaults():
    from pylda_amd.hybrid import Hybrid
    from pylda_amd.monte_carlo import MonteCarlo
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    assert OnlineVariationalBayes.left_to_right is VariationalBayes.left_to_right is Hybrid.left_to_right
    assert MonteCarlo.left_to_right is not VariationalBayes.left_to_right
    for engine in (VariationalBayes, MonteCarlo):
        parameters = inspect.signature(engine.left_to_right).parameters
        assert list(parameters) == ["self", "corpus", "particles", "resample"]
        assert parameters["particles"].default == 20 and parameters["resample"].default is True


def test_streams_of_their_own():
    from pylda_amd import hybrid, monte_carlo, variational_bayes
    base, step = variational_bayes.LEFT_TO_RIGHT_STREAM_BASE, variational_bayes.LEFT_TO_RIGHT_STREAM_STEP
    assert base == 3 << 30 and step == 256
    assert base > hybrid.HELDOUT_STREAM_BASE == monte_carlo.FOLD_IN_STREAM_BASE == 1 << 31
    assert base + step * (1 << 20) + 256 <= 1 << 32        # a million calls stay below 2^32


class _TwoRanks(object):
    """What pylda_amd.distributed.world_of asks of a process group."""
    def size(self):
        return 2


def test_bad_arguments_and_process_groups_are_refused(monkeypatch):
    from pylda_amd import distributed
    from pylda_amd.monte_carlo import MonteCarlo
    from pylda_amd.variational_bayes import VariationalBayes
    monkeypatch.setattr(distributed, "world_of", lambda group: group.size())
    for engine in (VariationalBayes(), MonteCarlo(seed=1)):
        for particles in (0, -1, 257, 2.5):
            with pytest.raises(ValueError, match="particles"):
                engine.left_to_right(["a b"], particles)
        engine._process_group = _TwoRanks()
        with pytest.raises(NotImplementedError, match="process group of 2 ranks"):
            engine.left_to_right(["a b"])


def test_command_line_flags():
    from pylda_amd import cli
    base = ["--input_directory=a", "--model_directory=b"]
    off = cli._parse(cli.TEST_FLAGS, base, "launch_test")
    assert off.left_to_right == 0 and off.left_to_right_resample == 1
    on = cli._parse(cli.TEST_FLAGS, base + ["--left_to_right=8", "--left_to_right_resample=0"], "launch_test")
    assert on.left_to_right == 8 and on.left_to_right_resample == 0
    for bad in (["--left_to_right=257"], ["--left_to_right=4", "--left_to_right_resample=2"], ["--left_to_right=4", "--document_completion=1"]):
        with pytest.raises(SystemExit):
            cli.test_main(base + bad)


def test_left_to_right_kernels_use_no_scratch():
    """Every ltr_* kernel the library ships, from the compiler's own metadata: no scratch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    lines = open(kr.compile_to_asm(os.path.join(ROOT, "pylda_amd", "csrc", "launch_left_to_right.hip"))).read().splitlines()
    res = kr.resources(lines, "ltr_")
    names = kr.demangle(list(res))
    shipped = sorted(names[m] for m in res)
    for kernel in ("ltr_reduce_kernel", "ltr_sum_kernel"):
        assert sum(kernel in n for n in shipped) == 1, shipped
    slots = sorted(int(re.search(r"ltr_particle_kernel<(\d+)", n).group(1)) for n in shipped if "ltr_particle_kernel" in n)
    assert slots == [1, 2, 4, 8, 16], shipped
    for mangled, info in res.items():
        print(names[mangled], info)
        assert info["ScratchSize"] == 0, (names[mangled], info)

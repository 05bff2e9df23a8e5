"""Topic distances without a GPU: the numpy restatement (tests/topic_distance_restatement.py) against
the mpmath golden within the derived bounds (tests/topic_distance_bounds.py), its symmetries, TopicDistances.nearest and
.matching, the new entry point in header and binding, the engines' method, the command line's refusals, and the kernels'
resources from the compiler's own metadata."""
import inspect
import math
import os
import pickle
import re
import sys

import numpy as np
import pytest

import topic_distance_bounds as bounds
import topic_distance_restatement as spec
from conftest import ROOT, load_golden

METRIC_KEYS = (("hellinger", "bc"), ("jensen_shannon", "js"))


@pytest.fixture(scope="module")
def golden():
    return load_golden("topic_distance_mp.npz")


def test_golden_cases_are_the_ones_the_issue_names_and_their_inputs_hash(golden):
    shapes = {name: (len(a), len(b), a.shape[1]) for name, (a, b) in ((n, spec.case(n)) for n in spec.CASES)}
    for shape in ((1, 1, 1), (3, 3, 2), (5, 4, 17), (65, 2, spec.SEGMENT + 1)):
        assert shape in shapes.values(), shape
    assert sum(ka * kb * v for ka, kb, v in shapes.values()) <= 10 ** 6
    assert int(golden["digits"]) == 50
    for name in spec.CASES:
        assert np.array_equal(golden[name + "_sha256"], spec.digest(*spec.case(name))), name
    a, b = spec.case("zeros")
    assert (a == 0).sum() > 20 and (b == 0).sum() > 20
    a, b = spec.case("peaked")
    assert (a[:, 7] == 1.0 - 1e-12).all() and abs(spec.row_sums(a)[0] - 1.0) < 1e-15


@pytest.mark.parametrize("name", spec.CASES)
def test_restatement_is_within_the_bound_of_mpmath(golden, name):
    a, b = spec.case(name)
    for metric, key in METRIC_KEYS:
        got = spec.values(a, b, metric)
        error = np.abs((got - golden["%s_%s_hi" % (name, key)]) - golden["%s_%s_lo" % (name, key)])
        bound = bounds.bound(a, b, metric)
        print(name, metric, "largest error %.3g, largest bound %.3g" % (error.max(), bound.max()))
        assert bound.max() < 1e-12          # (a bound that cannot hide a wrong formula)
        assert (error <= bound).all(), (name, metric, error.max(), bound.max())


def test_golden_hand_values(golden):
    assert golden["one_bc_hi"].tolist() == [[1.0]] and golden["one_js_hi"].tolist() == [[0.0]]
    assert np.array_equal(golden["disjoint_bc_hi"], np.zeros((2, 2)))
    assert np.array_equal(golden["disjoint_js_hi"], np.full((2, 2), math.log(2.0)))
    assert np.array_equal(np.diag(golden["identical_js_hi"]), np.zeros(3)) and np.array_equal(np.diag(golden["identical_bc_hi"]), np.ones(3))
    assert (np.abs(np.diag(golden["scaled_js_hi"])) < 1e-30).all()      # (a scaled row is the same distribution, up to the scaling's rounding)


def test_wrong_formulas_and_wrong_orders_miss(golden):
    """What the tests above are worth: the mutations of LABNOTES, applied to the restatement."""
    a, b = spec.case("odd")
    want = golden["odd_js_hi"]
    bound = bounds.jensen_shannon_bound(a, b)
    p, lp = spec.transform(a, "jensen_shannon")
    q, lq = spec.transform(b, "jensen_shannon")
    no_half = sum(p[:, v, None] * (lp[:, v, None] - np.log(p[:, v, None] + q[None, :, v]))
                  + q[None, :, v] * (lq[None, :, v] - np.log(p[:, v, None] + q[None, :, v])) for v in range(a.shape[1]))
    assert (np.abs(0.5 * no_half - want) > 1e3 * bound).all()           # (log(p + q) without the half: off by ln 2)
    # a dropped last segment, a dropped last chunk: a word is missing from the sum
    a, b = spec.case("segment_edge")
    for metric, key in METRIC_KEYS:
        want = golden["segment_edge_%s_hi" % key]
        for kept in (spec.SEGMENT, spec.SEGMENT + 1 - spec.CHUNK):
            ta = spec.transform(a, metric)
            tb = spec.transform(b, metric)
            short = sum(spec._terms(ta, tb, metric, v) for v in range(kept)) * (0.5 if metric == "jensen_shannon" else 1.0)
            assert (np.abs(short - want) > bounds.bound(a, b, metric)).any(), (metric, kept)
    # segments combined out of order, or of another length: other bits (the Hellinger path is tested for equality)
    rng = np.random.RandomState(5)
    t = rng.gamma(0.4, size=(6, 3 * spec.SEGMENT + 5))
    in_order = spec.values(t, None, "hellinger")
    assert not np.array_equal(spec.values(t, None, "hellinger", segment_order=[3, 2, 1, 0]), in_order)
    assert not np.array_equal(spec.values(t, None, "hellinger", segment=2 * spec.SEGMENT), in_order)
    assert np.array_equal(spec.values(t, None, "hellinger", segment_order=[0, 1, 2, 3]), in_order)


@pytest.mark.parametrize("metric", ["hellinger", "jensen_shannon"])
def test_restatement_is_bit_symmetric_with_an_exactly_zero_js_diagonal(metric):
    rng = np.random.RandomState(11)
    t = rng.gamma(0.3, size=(7, 2 * spec.SEGMENT + 3))
    t[rng.random_sample(t.shape) < 0.3] = 0.0
    t[:, 0] = 1.0
    own = spec.values(t, None, metric)
    assert np.array_equal(own, own.T)
    assert np.array_equal(own, spec.values(t, t.copy(), metric))
    other = rng.gamma(0.3, size=(4, t.shape[1]))
    assert np.array_equal(spec.values(t, other, metric), spec.values(other, t, metric).T)
    if metric == "jensen_shannon":
        assert np.array_equal(np.diag(own), np.zeros(len(t)))
        assert (own <= math.log(2.0) + bounds.jensen_shannon_bound(t)).all() and (own >= -bounds.jensen_shannon_bound(t)).all()
    else:
        assert (np.abs(np.diag(own) - 1.0) <= np.diag(bounds.hellinger_bound(t))).all()


def test_row_sum_order_is_the_lanes_then_the_tree():
    rng = np.random.RandomState(3)
    t = rng.gamma(0.4, size=(3, 200)) * 10.0 ** rng.randint(-8, 8, size=(3, 200))
    for row, s in zip(t, spec.row_sums(t)):
        lanes = [0.0] * 64
        for v, x in enumerate(row):
            lanes[v % 64] = lanes[v % 64] + float(x)
        for m in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ m] for l in range(64)]
        assert len(set(lanes)) == 1 and lanes[0] == s
    assert spec.row_sums(np.array([[3.0]])).tolist() == [3.0]


def test_nearest_orders_by_distance_then_index():
    from pylda_amd.topics import TopicDistances
    js = np.array([[0.0, 0.25, 0.25, 0.04], [0.25, 0.0, 0.25, 0.25], [0.25, 0.25, 0.0, 0.0], [0.04, 0.25, 0.0, 0.0]])
    own = TopicDistances(js, "jensen_shannon", against_itself=True)
    ids, distances = own.nearest(3)
    assert ids.tolist() == [[3, 1, 2], [0, 2, 3], [3, 0, 1], [2, 0, 1]]
    assert distances.tolist() == [[0.2, 0.5, 0.5], [0.5, 0.5, 0.5], [0.0, 0.5, 0.5], [0.0, 0.2, 0.5]]
    assert own.nearest(10)[0].shape == (4, 3)                            # (the topic itself is left out)
    other = TopicDistances(js, "jensen_shannon")
    ids, distances = other.nearest(2)
    assert ids.tolist() == [[0, 3], [1, 0], [2, 3], [2, 3]] and distances[2].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        own.nearest(0)
    one = TopicDistances(np.zeros((1, 1)), "jensen_shannon", against_itself=True)
    assert one.nearest(1)[0].shape == (1, 0)


def test_distance_from_values_and_the_diagonal():
    from pylda_amd.topics import TopicDistances
    bc = np.array([[1.0 + 2.0 ** -52, 0.75], [0.75, 1.0 - 2.0 ** -50]])
    result = TopicDistances(bc, "hellinger", against_itself=True)
    assert result.distance.tolist() == [[0.0, 0.5], [0.5, 0.0]]          # (clamped at 0; the diagonal of a self comparison exactly 0)
    assert TopicDistances(bc, "hellinger").distance[1, 1] == 2.0 ** -25
    js = np.array([[-1e-17, 0.25]])
    assert TopicDistances(js, "jensen_shannon").distance.tolist() == [[0.0, 0.5]]
    assert np.array_equal(result.distance, np.where(np.eye(2) == 1, 0.0, spec.distance(bc, "hellinger")))
    with pytest.raises(ValueError):
        TopicDistances(bc, "cosine")
    assert sorted(result.as_dict()) == ["against_itself", "distance", "metric", "values"]


@pytest.mark.parametrize("metric", ["hellinger", "jensen_shannon"])
def test_matching_recovers_a_row_permutation_at_distance_zero(metric):
    from pylda_amd.topics import TopicDistances
    rng = np.random.RandomState(17)
    t = rng.gamma(0.3, size=(9, 40))
    order = rng.permutation(9)
    result = TopicDistances(spec.values(t, t[order], metric), metric)
    pairs, distances = result.matching()
    assert pairs[:, 0].tolist() == list(range(9)) and order[pairs[:, 1]].tolist() == list(range(9))
    if metric == "jensen_shannon":
        assert distances.tolist() == [0.0] * 9
    else:
        assert (distances <= np.sqrt(np.diag(bounds.hellinger_bound(t)))).all()


def test_matching_on_a_rectangular_case():
    from pylda_amd.topics import TopicDistances
    js = np.array([[0.09, 0.01], [0.04, 0.16], [0.25, 0.0]])            # distances 0.3 0.1 / 0.2 0.4 / 0.5 0
    pairs, distances = TopicDistances(js, "jensen_shannon").matching()
    assert pairs.tolist() == [[1, 0], [2, 1]] and distances.tolist() == [0.2, 0.0]     # (0.2 in all, the only minimum; topic 0 of a stays alone)
    pairs, distances = TopicDistances(js.T.copy(), "jensen_shannon").matching()
    assert pairs.tolist() == [[0, 1], [1, 2]] and distances.tolist() == [0.2, 0.0]


def test_header_and_binding_carry_the_entry_point_at_abi_10():
    from pylda_amd import _capi
    header = open(os.path.join(ROOT, "include", "pylda_hip.h")).read()
    assert re.search(r"#define PYLDA_ABI_VERSION (\d+)", header).group(1) == str(_capi.ABI_VERSION) == "10"
    assert re.search(r"\bint pylda_topic_distances\(", header) and "pylda_topic_distances" in _capi.SIGNATURES
    changelog = header[header.index(" *  10  additions only"):header.index("A host compiled against another version")]
    assert "pylda_topic_distances" in changelog
    assert len(_capi.SIGNATURES["pylda_topic_distances"][1]) == 7
    assert callable(_capi.Context.topic_distances)
    assert "topic_distance_segment_groups" in header
    internal = open(os.path.join(ROOT, "pylda_amd", "csrc", "host_internal.h")).read()
    assert "launch_topic_distance.hip" in internal
    from pylda_amd import build
    assert any(s.endswith("launch_topic_distance.hip") for s in build.sources())


def test_engines_offer_the_method():
    from pylda_amd.hybrid import Hybrid
    from pylda_amd.monte_carlo import MonteCarlo
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    assert Hybrid.topic_distances is VariationalBayes.topic_distances is OnlineVariationalBayes.topic_distances
    # one definition for every engine (pylda_amd/analysis.py); what differs is the table an engine puts under it
    assert callable(MonteCarlo.topic_distances) and MonteCarlo.topic_distances is VariationalBayes.topic_distances
    assert MonteCarlo._device_topic_table is not VariationalBayes._device_topic_table
    for engine in (VariationalBayes, MonteCarlo):
        parameters = inspect.signature(engine.topic_distances).parameters
        assert [(n, p.default) for n, p in parameters.items()][1:] == [("other", None), ("metric", "jensen_shannon")]


class Engine(object):
    """What topics.topic_distances reads of an engine, without a device."""
    _process_group = None

    def __init__(self, words, table=None):
        self._type_to_index = {word: index for index, word in enumerate(words)}
        self._index_to_type = dict(enumerate(words))
        self._number_of_types = len(words)
        self._table = table

    def _topic_table(self):
        return self._table

    def _context(self):
        raise AssertionError("refused before the device is touched")


def test_engines_refuse_bad_arguments_a_process_group_and_another_vocabulary(monkeypatch):
    from pylda_amd import distributed, topics
    words = ["a", "b", "c"]
    mine = Engine(words)
    with pytest.raises(ValueError, match="cosine"):
        topics.topic_distances(mine, None, None, "cosine")
    with pytest.raises(ValueError, match="shape"):
        topics.topic_distances(mine, None, np.ones((2, 4)), "hellinger")
    with pytest.raises(ValueError, match="word 1 is 'b' here and 'x' there"):
        topics.topic_distances(mine, None, Engine(["a", "x", "c"], np.ones((2, 3))), "hellinger")
    with pytest.raises(ValueError, match="word 3, 'd', exists only there"):
        topics.topic_distances(mine, None, Engine(words + ["d"], np.ones((2, 4))), "hellinger")
    assert topics.first_differing_word(mine._type_to_index, dict(mine._type_to_index)) is None
    sharded = Engine(words)
    sharded.__dict__["_process_group"] = object()
    monkeypatch.setattr(distributed, "world_of", lambda group=None: 2)
    with pytest.raises(NotImplementedError):
        topics.topic_distances(sharded, None, None, "hellinger")
    with pytest.raises(NotImplementedError):
        topics.topic_distances(mine, None, sharded, "hellinger")


def _run_directories(tmp_path, other_words):
    """input c/, a run out/c/run1 with snapshot model-5, and another run out/c/run2 (with model-5 where other_words)."""
    source = tmp_path / "c"
    source.mkdir()
    (source / "test.dat").write_text("a b\n")
    run1, run2 = tmp_path / "out" / "c" / "run1", tmp_path / "out" / "c" / "run2"
    run1.mkdir(parents=True)
    run2.mkdir()
    with open(run1 / "model-5", "wb") as out:
        pickle.dump(Engine(["a", "b"]), out)
    if other_words:
        with open(run2 / "model-5", "wb") as out:
            pickle.dump(Engine(other_words), out)
    return ["--input_directory=%s" % source, "--model_directory=%s" % run1], run2


def test_command_line_refusals(tmp_path, capsys):
    from pylda_amd import cli
    base = ["--input_directory=a", "--model_directory=b"]
    opt = cli._parse(cli.TEST_FLAGS, base, "launch_test")
    assert opt.similar_topics == 0 and opt.topic_match is None
    assert cli._parse(cli.TEST_FLAGS, base + ["--similar_topics=5", "--topic_match=x"], "launch_test").topic_match == "x"
    parameters = inspect.signature(cli.evaluate_snapshot).parameters
    assert parameters["similar_topics"].default == 0 and parameters["topic_match"].default is None
    for bad in ("-1", "65"):
        with pytest.raises(SystemExit):
            cli.test_main(base + ["--similar_topics=" + bad])
    # a DIR that does not exist, a DIR under another corpus name, a DIR without the snapshot, a snapshot over another vocabulary
    flags, run2 = _run_directories(tmp_path, None)
    assert cli.test_main(flags + ["--topic_match=%s" % (tmp_path / "nowhere")]) == 2
    assert "does not exist" in capsys.readouterr().err
    elsewhere = tmp_path / "out" / "d" / "run"
    elsewhere.mkdir(parents=True)
    assert cli.test_main(flags + ["--topic_match=%s" % elsewhere]) == 2
    assert "corpus name does not match" in capsys.readouterr().err
    assert cli.test_main(flags + ["--topic_match=%s" % run2]) == 2
    assert "holds no snapshot model-5" in capsys.readouterr().err
    with open(run2 / "model-5", "wb") as out:
        pickle.dump(Engine(["a", "z"]), out)
    assert cli.test_main(flags + ["--topic_match=%s" % run2]) == 2
    assert "another vocabulary: word 1 is 'b' here and 'z' there" in capsys.readouterr().err
    assert not os.path.exists(os.path.join(os.path.dirname(flags[1].split("=")[1]), "run1", "match-5"))


def test_topic_distance_kernels_use_no_scratch():
    """Every topic_distance_* kernel the library ships, from the compiler's own metadata: no scratch, the LDS of its chunks."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    lines = open(kr.compile_to_asm(os.path.join(ROOT, "pylda_amd", "csrc", "launch_topic_distance.hip"))).read().splitlines()
    res = kr.resources(lines, "topic_distance_")
    names = kr.demangle(list(res))
    shipped = sorted(names[m] for m in res)
    for kernel in ("topic_distance_transform_kernel", "topic_distance_pair_kernel<false>", "topic_distance_pair_kernel<true>",
                   "topic_distance_combine_kernel"):
        assert sum(kernel in n for n in shipped) == 1, shipped
    assert len(shipped) == 4, shipped
    for mangled, info in res.items():
        print(names[mangled], info)
        assert info["ScratchSize"] == 0, (names[mangled], info)

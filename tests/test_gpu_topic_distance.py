"""Topic distances on the GPU (pylda_topic_distances, topic_distance_kernels.h) against the numpy restatement
(tests/topic_distance_restatement.py) and the mpmath golden, and the engines' topic_distances() and launch_test
--similar_topics / --topic_match built on them.

The Hellinger numbers are exact: array_equal by their bits.  The Jensen-Shannon numbers carry the device's log: within the
derived bound (tests/topic_distance_bounds.py) of mpmath on the golden's cases, within twice the bound of the restatement
elsewhere (the restatement and the device are each within one bound of the exact value).  The shapes are the small ones at
which tiles (32 x 32 rows), chunks (32 words) and segments (1024 words) have their edges.

Worst error over bound measured on one MI355X: see DESIGN.md section 20."""
import ctypes
import math
import os
import pickle

import numpy as np
import pytest

import topic_distance_bounds as bounds
import topic_distance_restatement as spec
from conftest import load_golden

pytestmark = pytest.mark.gpu

T, C, S = spec.TILE, spec.CHUNK, spec.SEGMENT
# every Ka, Kb of {1, 2, T - 1, T, T + 1, 2 T + 2} and every V of {1, C - 1, C, C + 1, S - 1, S, S + 1, 3 S + 5}; the large V with small K
SHAPES = [(1, 1, 1), (2, T - 1, C - 1), (T - 1, 2, C), (T, T + 1, C + 1), (T + 1, T, S - 1), (2 * T + 2, 1, S), (1, 2 * T + 2, S + 1),
          (2 * T + 1, 3, 3 * S + 5), (2 * T + 2, T + 1, C + 1)]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _same(x, y):
    return x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


def _tables(Ka, Kb, V, seed=0):
    rng = np.random.RandomState(Ka * 1000003 + Kb * 1009 + V + seed)
    a, b = rng.gamma(0.4, size=(Ka, V)) + 2.0 ** -40, rng.gamma(0.4, size=(Kb, V)) + 2.0 ** -40
    if V > 4:                                                            # (rows with zeros)
        a[rng.random_sample(a.shape) < 0.2] = 0.0
        b[rng.random_sample(b.shape) < 0.2] = 0.0
        a[:, 0], b[:, 1] = 1.0, 1.0
    return a, b


@pytest.fixture(scope="module")
def restated():
    """The restatement's answers per (shape, metric, against itself), computed once."""
    memo = {}

    def answer(Ka, Kb, V, metric, own=False):
        key = (Ka, Kb, V, metric, own)
        if key not in memo:
            a, b = _tables(Ka, Kb, V)
            memo[key] = spec.values(a, None if own else b, metric)
        return memo[key]
    return answer


@pytest.mark.parametrize("Ka,Kb,V", SHAPES)
def test_hellinger_equals_the_restatement_by_bits(Ka, Kb, V, restated):
    from pylda_amd import _capi
    a, b = _tables(Ka, Kb, V)
    ctx = _capi.Context(2, V)
    try:
        got = ctx.topic_distances(a, b, 0)
        assert got.dtype == np.float64 and _same(got, restated(Ka, Kb, V, "hellinger"))
        assert _same(ctx.topic_distances(b, a, 0), got.T)
        own = ctx.topic_distances(a, None, 0)                           # b = NULL against b = a
        assert _same(own, restated(Ka, Kb, V, "hellinger", True)) and _same(own, own.T)
        assert _same(ctx.topic_distances(a, a.copy(), 0), own)
        assert _same(ctx.topic_distances(a, b, 0), got)                  # a repeated call
    finally:
        ctx.close()


@pytest.mark.parametrize("Ka,Kb,V", [(T + 1, 3, S + 1), (2, 2 * T + 2, C - 1)])
def test_null_a_is_the_uploaded_eta(Ka, Kb, V):
    from pylda_amd import _capi
    a, b = _tables(Ka, Kb, V, seed=1)
    ctx = _capi.Context(Ka, V)
    try:
        ctx.set_eta(a)
        for metric in (0, 1):
            assert _same(ctx.topic_distances(None, b, metric), ctx.topic_distances(a, b, metric))
            assert _same(ctx.topic_distances(None, None, metric), ctx.topic_distances(a, None, metric))
        assert _same(ctx.topic_distances(None, b, 0), spec.values(a, b, "hellinger"))
        assert _same(ctx.get_eta(), a)                                   # read, never written
    finally:
        ctx.close()


@pytest.mark.parametrize("name", spec.CASES)
def test_golden_cases_are_within_the_bound_of_mpmath(name):
    from pylda_amd import _capi
    golden = load_golden("topic_distance_mp.npz")
    a, b = spec.case(name)
    assert np.array_equal(golden[name + "_sha256"], spec.digest(a, b))
    ctx = _capi.Context(2, a.shape[1])
    try:
        for metric, key in (("hellinger", "bc"), ("jensen_shannon", "js")):
            got = ctx.topic_distances(a, b, spec.METRICS[metric])
            error = np.abs((got - golden["%s_%s_hi" % (name, key)]) - golden["%s_%s_lo" % (name, key)])
            bound = bounds.bound(a, b, metric)
            ratio = float(np.max(np.where(error == 0.0, 0.0, error / np.where(bound > 0, bound, 1.0))))
            print("%s %s: largest error %.3g, largest bound %.3g, worst error over bound %.3g" % (name, metric, error.max(), bound.max(), ratio))
            assert (error <= bound).all(), (name, metric, error.max(), bound.max())
            if metric == "hellinger":
                assert _same(got, spec.values(a, b, metric))
        if name == "identical":
            assert np.array_equal(np.diag(ctx.topic_distances(a, b, 1)), np.zeros(len(a)))
        if name == "disjoint":
            assert np.array_equal(ctx.topic_distances(a, b, 0), np.zeros((2, 2)))
            assert np.abs(ctx.topic_distances(a, b, 1) - math.log(2.0)).max() <= bounds.jensen_shannon_bound(a, b).max()
    finally:
        ctx.close()


@pytest.mark.parametrize("Ka,Kb,V", SHAPES)
def test_jensen_shannon_is_within_twice_the_bound_of_the_restatement(Ka, Kb, V, restated):
    from pylda_amd import _capi
    a, b = _tables(Ka, Kb, V)
    ctx = _capi.Context(2, V)
    try:
        got = ctx.topic_distances(a, b, 1)
        bound = bounds.jensen_shannon_bound(a, b)
        error = np.abs(got - restated(Ka, Kb, V, "jensen_shannon"))
        print("(%d, %d, %d): largest error %.3g, largest bound %.3g, worst error over twice the bound %.3g"
              % (Ka, Kb, V, error.max(), bound.max(), (error / (2 * bound)).max()))
        assert (error <= 2 * bound).all()
        assert (got <= math.log(2.0) + bound).all() and (got >= -bound).all()
        assert _same(ctx.topic_distances(b, a, 1), got.T)
        own = ctx.topic_distances(a, None, 1)
        own_bound = bounds.jensen_shannon_bound(a)
        assert np.array_equal(np.diag(own), np.zeros(Ka))                # exactly 0: m == p, and the same log
        assert _same(own, own.T) and _same(ctx.topic_distances(a, a.copy(), 1), own)
        assert (np.abs(own - restated(Ka, Kb, V, "jensen_shannon", True)) <= 2 * own_bound).all()
        assert (own <= math.log(2.0) + own_bound).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("Ka,Kb", [(T + 1, 3), (2 * T + 2, None)])
def test_the_bits_depend_on_neither_the_segment_groups_nor_the_call(Ka, Kb):
    from pylda_amd import _capi
    V = 8 * S + 5                                                        # 9 segments
    a, b = _tables(Ka, Kb or 2, V, seed=2)
    b = None if Kb is None else b
    ctx = _capi.Context(2, V)
    try:
        for metric in (0, 1):
            first = ctx.topic_distances(a, b, metric)
            for groups in (1, 2, 7, 9, 64, 0):
                ctx.set_option("topic_distance_segment_groups", groups)
                assert _same(ctx.topic_distances(a, b, metric), first), (metric, groups)
                assert _same(ctx.topic_distances(a, b, metric), first), (metric, groups, "again")
            if metric == 0:
                assert _same(first, spec.values(a, b, "hellinger"))
        for bad in (-1, 65536):
            with pytest.raises(_capi.PyldaError):
                ctx.set_option("topic_distance_segment_groups", bad)
    finally:
        ctx.close()


def test_error_codes_come_before_any_launch_and_leave_the_context_usable():
    from pylda_amd import _capi
    Ka, Kb, V = 5, 4, 70
    a, b = _tables(Ka, Kb, V, seed=3)
    want = spec.values(a, b, "hellinger")
    ctx = _capi.Context(Ka, V)
    f64p = ctypes.POINTER(ctypes.c_double)
    try:
        ctx.set_profiling(True)
        ctx.kernel_time()

        def refused(status, text, a_rows, n_a, b_rows, n_b, metric=0, out=True):
            result = np.full((max(n_a, 1), max(n_b, 1)), np.nan)
            rc = ctx._lib.pylda_topic_distances(ctx._h, None if a_rows is None else a_rows.ctypes.data_as(f64p), n_a,
                                                None if b_rows is None else b_rows.ctypes.data_as(f64p), n_b, metric,
                                                result.ctypes.data_as(f64p) if out else None)
            assert rc == status and text in ctx._lib.pylda_last_error(ctx._h), (rc, ctx._lib.pylda_last_error(ctx._h))
            assert np.isnan(result).all()
            assert ctx.kernel_time()[:2] == (0.0, 0.0)                   # nothing was launched
            assert _same(ctx.topic_distances(a, b, 0), want)             # the context is usable
            assert ctx.kernel_time()[0] > 0

        refused(-4, b"eta was never set", None, Ka, b, Kb)               # NULL a without eta
        for entry, word in ((-1e-300, b"1 of 5 rows of a"), (np.nan, b"1 of 5 rows of a"), (np.inf, b"1 of 5 rows of a")):
            bad = a.copy()
            bad[3, 17] = entry
            refused(-1, word, bad, Ka, b, Kb)
            refused(-1, b"1 of 5 rows of b", a, Ka, bad, Ka)
        zero = b.copy()
        zero[1], zero[2] = 0.0, 0.0
        refused(-1, b"2 of 4 rows of b", a, Ka, zero, Kb, 1)             # zero rows
        refused(-1, b"Ka=0", a, 0, b, Kb)
        refused(-1, b"Kb=0", a, Ka, b, 0)
        refused(-1, b"Ka=32769", a, 32769, b, Kb)
        refused(-1, b"out_ab is NULL", a, Ka, b, Kb, out=False)
        refused(-1, b"metric=2", a, Ka, b, Kb, metric=2)
        refused(-1, b"Kb=4 is not Ka=5", a, Ka, None, Kb)
        ctx.set_eta(a)
        refused(-1, b"Ka=4 is not K=5", None, 4, b, Kb)
        with pytest.raises(ValueError):
            ctx.topic_distances(a[:, :-1], b, 0)
    finally:
        ctx.close()


# ---- the engines ----
def _documents(words, ptr, ids, cts, docs):
    return [" ".join(" ".join([words[t]] * int(c)) for t, c in zip(ids[ptr[d]:ptr[d + 1]], cts[ptr[d]:ptr[d + 1]])) for d in docs]


def _train(m, ap_train, documents=200, topics=10):
    words = [str(w) for w in ap_train["words"]]
    m._verbose = False
    np.random.seed(0)
    m._initialize(_documents(words, ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"], range(documents)), words, topics, 0.1,
                  1.0 / len(words))
    m.learning()
    m.learning()
    return m


def _engines():
    from pylda_amd.hybrid import Hybrid
    from pylda_amd.monte_carlo import MonteCarlo
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    return {"vb": lambda: VariationalBayes(), "hybrid": lambda: Hybrid(seed=5), "online": lambda: OnlineVariationalBayes(4),
            "gibbs": lambda: MonteCarlo(hyper_parameter_optimize_interval=1000, seed=21, blocks=16)}


def _table(m):
    from pylda_amd.monte_carlo import MonteCarlo
    return np.array(m._n_kv + m._alpha_beta[np.newaxis, :]) if isinstance(m, MonteCarlo) else np.array(m._eta)


def _assert_result(result, a, b, metric, what):
    assert result.metric == metric and result.against_itself == (b is None), what
    want = spec.values(a, b, metric)
    if metric == "hellinger":
        assert _same(result.values, want), what
    else:
        assert (np.abs(result.values - want) <= 2 * bounds.jensen_shannon_bound(a, b)).all(), what
    distance = spec.distance(result.values, metric)
    if b is None:
        np.fill_diagonal(distance, 0.0)
        assert np.array_equal(np.diag(result.distance), np.zeros(len(a))), what
    assert np.array_equal(result.distance, distance), what


@pytest.mark.parametrize("kind", ["vb", "hybrid", "online", "gibbs"])
def test_engine_against_itself_its_permuted_table_and_its_snapshot(kind, ap_train):
    m = _train(_engines()[kind](), ap_train)
    table = _table(m)
    assert table.shape == (10, len(ap_train["words"]))
    own = m.topic_distances()
    _assert_result(own, table, None, "jensen_shannon", kind)
    hellinger = m.topic_distances(metric="hellinger")
    _assert_result(hellinger, table, None, "hellinger", kind)
    ids, distances = own.nearest(3)
    assert ids.shape == (10, 3) and not np.any(ids == np.arange(10)[:, None]) and np.all(np.diff(distances, axis=1) >= 0)
    # against its own row-permuted table: the matching is the permutation, at distance 0
    order = np.random.RandomState(4).permutation(10)
    for metric in ("jensen_shannon", "hellinger"):
        permuted = m.topic_distances(table[order], metric)
        _assert_result(permuted, table, table[order], metric, kind)
        pairs, matched = permuted.matching()
        assert pairs[:, 0].tolist() == list(range(10)) and order[pairs[:, 1]].tolist() == list(range(10))
        if metric == "jensen_shannon":
            assert matched.tolist() == [0.0] * 10
        else:
            assert (matched <= np.sqrt(np.diag(bounds.hellinger_bound(table)))).all()
    assert np.array_equal(_table(m), table)                              # read, never written
    restored = pickle.loads(pickle.dumps(m))
    restored._verbose = False
    assert _same(restored.topic_distances().values, own.values)
    assert _same(restored.topic_distances(metric="hellinger").values, hellinger.values)
    assert _same(restored.topic_distances(m).values, own.values)         # an engine as the other side: its table


def test_a_gibbs_model_against_a_variational_one(ap_train):
    gibbs, vb = _train(_engines()["gibbs"](), ap_train), _train(_engines()["vb"](), ap_train, topics=7)
    result = gibbs.topic_distances(vb)
    assert result.values.shape == (10, 7) and not result.against_itself
    _assert_result(result, _table(gibbs), _table(vb), "jensen_shannon", "gibbs against vb")
    back = vb.topic_distances(gibbs, "hellinger")
    _assert_result(back, _table(vb), _table(gibbs), "hellinger", "vb against gibbs")
    assert _same(back.values, gibbs.topic_distances(vb, "hellinger").values.T)
    pairs, distances = result.matching()
    assert pairs.shape == (7, 2) and sorted(pairs[:, 1].tolist()) == list(range(7)) and np.all(np.diff(pairs[:, 0]) > 0)
    vb._type_to_index = dict(vb._type_to_index, **{vb._index_to_type[3]: 4, vb._index_to_type[4]: 3})
    with pytest.raises(ValueError, match="word 3 is"):
        gibbs.topic_distances(vb)


# ---- the command line ----
def test_launch_test_with_the_flags(ap_train, tmp_path, capsys):
    from pylda_amd import cli
    words = [str(w) for w in ap_train["words"]]
    ptr, ids, cts = ap_train["doc_ptr"], ap_train["term_id"], ap_train["term_ct"]
    source = tmp_path / "in" / "ap120"
    source.mkdir(parents=True)
    (source / "train.dat").write_text("\n".join(_documents(words, ptr, ids, cts, range(120))) + "\n")
    (source / "test.dat").write_text("\n".join(_documents(words, ptr, ids, cts, range(300, 320))) + "\n")
    (source / "voc.dat").write_text("\n".join(words) + "\n")
    train = ["--input_directory=%s" % source, "--training_iterations=2", "--snapshot_interval=2"]
    assert cli.train_main(train + ["--number_of_topics=5", "--output_directory=%s" % (tmp_path / "vb")]) == 0
    assert cli.train_main(train + ["--number_of_topics=6", "--output_directory=%s" % (tmp_path / "gibbs"), "--inference_mode=1",
                                   "--sampler_seed=3", "--gibbs_blocks=8"]) == 0
    run = tmp_path / "vb" / "ap120" / os.listdir(tmp_path / "vb" / "ap120")[0]
    other = tmp_path / "gibbs" / "ap120" / os.listdir(tmp_path / "gibbs" / "ap120")[0]
    trained = sorted(os.listdir(run))
    capsys.readouterr()
    test = ["--input_directory=%s" % source, "--model_directory=%s" % run]
    assert cli.test_main(test) == 0
    plain = capsys.readouterr().out
    assert sorted(os.listdir(run)) == sorted(trained + ["test-2"])
    assert cli.test_main(test + ["--similar_topics=3", "--topic_match=%s" % other]) == 0
    out = capsys.readouterr().out
    assert sorted(os.listdir(run)) == sorted(trained + ["test-2", "similar-topics-2", "match-2"])
    added = [l for l in out.splitlines() if l.startswith(("similar topics of snapshot", "topic match of snapshot"))]
    assert len(added) == 2 and [l for l in out.splitlines() if l not in added] == plain.splitlines()
    with open(run / "model-2", "rb") as stream:
        engine = pickle.load(stream)
    with open(other / "model-2", "rb") as stream:
        gibbs = pickle.load(stream)
    # similar-topics-2 parses back to the API's numbers
    ids, distances = engine.topic_distances().nearest(3)
    rows = (run / "similar-topics-2").read_text().splitlines()
    assert len(rows) == 5
    for k, row in enumerate(rows):
        fields = [field.split(":") for field in row.split("\t")]
        assert [int(i) for i, _ in fields] == ids[k].tolist() and [float(x) for _, x in fields] == distances[k].tolist()
    k = int(np.argmin(distances[:, 0]))
    assert "the closest pair is topics %d and %d at distance %.17g" % (k, ids[k, 0], distances[k, 0]) in added[0]
    # match-2 too
    pairs, matched = engine.topic_distances(gibbs).matching()
    mine, theirs = engine.top_words(5), gibbs.top_words(5)
    rows = [row.split("\t") for row in (run / "match-2").read_text().splitlines()]
    assert len(rows) == 5 and pairs.shape == (5, 2)
    for k, fields in enumerate(rows):
        assert [int(fields[0]), int(fields[1])] == pairs[k].tolist() and float(fields[2]) == matched[k]
        assert fields[3].split(" ") == [w for w, _ in mine[k]] and fields[4].split(" ") == [w for w, _ in theirs[pairs[k, 1]]]
    assert added[1].endswith("distance mean %g, median %g, maximum %g" % (np.mean(matched), np.median(matched), np.max(matched)))
    # the other way round there are more topics than partners: -1; and both run before --left_to_right returns
    for name in ("similar-topics-2", "match-2"):
        os.remove(run / name)
    cli.evaluate_snapshot(str(other / "model-2"), (source / "test.dat").read_text().splitlines(), str(other / "test-2"),
                          left_to_right=2, similar_topics=2, topic_match=str(run))
    out = capsys.readouterr().out
    assert "left-to-right likelihood" in out and out.index("topic match of snapshot") < out.index("left-to-right likelihood")
    rows = [row.split("\t") for row in (other / "match-2").read_text().splitlines()]
    assert len(rows) == 6 and sorted(int(f[1]) for f in rows) == [-1, 0, 1, 2, 3, 4]
    alone = [f for f in rows if f[1] == "-1"][0]
    assert alone[2] == "nan" and alone[4] == ""
    assert len((other / "similar-topics-2").read_text().splitlines()) == 6 and not (other / "test-2").exists()
    # a snapshot that DIR does not hold
    os.rename(other / "model-2", other / "model-3")
    assert cli.test_main(test + ["--topic_match=%s" % other]) == 2
    assert "holds no snapshot model-2" in capsys.readouterr().err and not (run / "match-2").exists()

"""The engines' surface without a GPU: which calls every public method makes on the device context, in which order, under
which stream numbers, with arguments of which shapes, and what it leaves in the engine's counters.  (A float array is
logged as its shape and sum and the stand-in returns zeros, so the values inside a table are not pinned here: the GPU
tests compare those bit for bit.)

A recording stand-in for pylda_amd._capi.Context logs every call with its arguments (bound to the real method's signature,
so a keyword and a positional spelling of the same call read the same) and returns zeros of the right shapes.  Each engine
is initialised on a three-document, five-word corpus with K = 2 and driven through one script: a learning step, the
read-only queries, the held-out entries, the exports, a snapshot of the trained engine, and the same again on the engine
restored from it.  The sequences in tests/engine_surface_recorded.py were recorded before the engines were given their
common bases (pylda_amd/analysis.py, pylda_amd/count_engine.py) and are literals: code that moves between the classes
must leave them as they are.  (`python tests/test_engine_surface_host.py` prints that module.)"""
import inspect
import pickle
import pprint

import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (the repository root goes on sys.path)
from pylda_amd import _capi

REAL_CONTEXT = _capi.Context            # (its methods' signatures name the arguments of the recorded calls)

VOCABULARY = ["a", "b", "c", "d", "e"]
TRAINING = ["a b a c", "d", "e e b zz"]
HELDOUT = ["a c c", "zz", "b d"]
K = 2
COUNTERS = ("_counter", "_step", "_fold_in_calls", "_inference_calls", "_heldout_calls", "_left_to_right_calls")


# ---------------------------------------------------------------- the recording context
def _render(value):
    if isinstance(value, RecordingCorpus):
        return value.label
    if isinstance(value, (list, tuple)):
        value = np.asarray(value)
    if isinstance(value, np.ndarray):
        if value.dtype.kind in "iu" and value.size <= 16:
            return "i%s" % (value.tolist(),)
        return "%s%s=%.6g" % (value.dtype.kind, list(value.shape), float(value.sum()))
    if isinstance(value, (np.integer, np.bool_)):
        return repr(value.item())
    if isinstance(value, np.floating):
        return repr(float(value))
    return repr(value)


class RecordingCorpus(object):
    def __init__(self, ctx, doc_ptr, term_id, term_ct):
        self._ctx = ctx
        self.D, self.nnz, self.tokens = len(doc_ptr) - 1, len(term_id), int(np.sum(term_ct))
        ctx.trace.corpora += 1
        self.label = "corpus%d" % ctx.trace.corpora

    def close(self):
        self._ctx.trace.calls.append("%s.close()" % self.label)


class Trace(object):
    """The log the contexts of one engine's script share (a restored engine opens a context of its own)."""

    def __init__(self):
        self.calls, self.corpora = [], 0

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def _returns(ctx, name, a):
    """Zeros of the shapes pylda_amd._capi.Context returns."""
    K, V = ctx.K, ctx.V
    corpus = a.get("corpus")
    if name == "corpus":
        return RecordingCorpus(ctx, a["doc_ptr"], a["term_id"], a["term_ct"])
    if name in ("get_eta", "get_sstats"):
        return np.zeros((K, V))
    if name == "get_gamma":
        return np.zeros((corpus.D, K))
    if name == "get_doc_values":
        return np.zeros(corpus.D), np.zeros(corpus.D), np.zeros(corpus.D, np.int32)
    if name == "estep_results":
        return 0.0, 0.0, 0
    if name == "outer_fetch":
        return 0.0, 3, 0, 0.0, np.zeros(K), np.full(K, 0.5)
    if name == "mstep":
        return 0.0, np.zeros(K) if a["want_alpha_ss"] else None
    if name == "gibbs_get_counts":
        return (np.zeros((K, V), np.int32) if a["want_n_kv"] else None, np.zeros(K, np.int32),
                np.zeros(corpus.tokens, np.int32) if a["want_topics"] else None)
    if name == "cvb0_get_state":
        return (np.zeros((K, V)) if a["want_n_kv"] else None, np.zeros(K), np.zeros((corpus.D, K)),
                np.zeros((corpus.nnz, K)) if a["want_g"] else None)
    if name == "scvb_get_state":
        return np.zeros((K, V)) if a["want_n_kv"] else None, np.zeros(K), np.zeros((corpus.D, K)), np.zeros(corpus.D)
    if name in ("gibbs_log_posterior", "foldin", "cvb0_foldin", "elapsed_ms"):
        return 0.0
    if name in ("cvb0_log_likelihood", "completion_score", "left_to_right"):
        return 0.0, 0
    if name == "top_words":
        return np.zeros((K, a["M"]), np.int32), np.zeros((K, a["M"]))
    if name == "codocument_counts":
        M = np.asarray(a["ids"]).shape[1]
        return np.zeros((K, M), np.int64), np.zeros((K, M, M), np.int64)
    if name == "similar_documents":
        Q = len(a["rows"])
        return np.zeros((Q, a["N"]), np.int32), np.zeros((Q, a["N"]))
    if name == "topic_distances":
        Ka = K if a["a"] is None else len(a["a"])
        return np.zeros((Ka, Ka if a["b"] is None else len(a["b"])))
    return None


class RecordingContext(object):
    trace = None            # set by the script that drives an engine

    def __init__(self, number_of_topics, number_of_types, device=0):
        self.K, self.V, self.device = int(number_of_topics), int(number_of_types), int(device)
        self.trace.calls.append("Context(%d, %d, %d)" % (self.K, self.V, self.device))

    def __getattr__(self, name):
        real = getattr(REAL_CONTEXT, name)          # AttributeError for what the real context does not have
        signature = inspect.signature(real)

        def call(*args, **kwargs):
            bound = signature.bind(self, *args, **kwargs)
            bound.apply_defaults()
            arguments = dict(bound.arguments)
            arguments.pop("self")
            self.trace.calls.append("%s(%s)" % (name, ", ".join(_render(v) for v in arguments.values())))
            return _returns(self, name, arguments)
        return call


@pytest.fixture
def recording(monkeypatch):
    """pylda_amd._capi.Context, which every engine class opens by that name, replaced by the recording stand-in."""
    from pylda_amd import build
    build.build(verbose=False)              # (VariationalBayes parses its corpus in the native library)
    monkeypatch.setattr(_capi, "Context", RecordingContext)
    monkeypatch.setattr(RecordingContext, "trace", Trace())
    return RecordingContext.trace


# ---------------------------------------------------------------- the engines and their script
def _engine(name):
    from pylda_amd.cvb0 import CollapsedVariationalBayes
    from pylda_amd.hybrid import Hybrid
    from pylda_amd.monte_carlo import MonteCarlo
    from pylda_amd.scvb0 import StochasticCollapsedVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    m = {"MonteCarlo": lambda: MonteCarlo(seed=7, blocks=2),
         "CollapsedVariationalBayes": lambda: CollapsedVariationalBayes(seed=7, blocks=2),
         "StochasticCollapsedVariationalBayes": lambda: StochasticCollapsedVariationalBayes(2, seed=7),
         "VariationalBayes": lambda: VariationalBayes(),
         "Hybrid": lambda: Hybrid(seed=7)}[name]()
    m._verbose = False
    return m


def _counters(m):
    return ", ".join("%s=%d" % (key, m.__dict__[key]) for key in COUNTERS if key in m.__dict__)


def _queries(m, tmp_path, fold_in):
    """(step, what it does) for the read-only surface and the held-out entries"""
    return [
        ("top_words", lambda: m.top_words(3)),
        ("topic_coherence", lambda: m.topic_coherence(top_words=3)),
        ("topic_coherence(documents)", lambda: m.topic_coherence(HELDOUT, top_words=3)),
        ("top_documents", lambda: m.top_documents(2)),
        ("similar_documents", lambda: m.similar_documents(top=2)),
        ("similar_documents(documents)", lambda: m.similar_documents(HELDOUT, top=2)),
        ("similar_documents(rows)", lambda: m.similar_documents(np.ones((1, K)), top=2, metric="dot")),
        ("topic_distances", lambda: m.topic_distances()),
        ("topic_distances(table)", lambda: m.topic_distances(np.ones((3, len(VOCABULARY))), metric="hellinger")),
        (fold_in, lambda: getattr(m, fold_in)(HELDOUT)),
        ("document_completion", lambda: m.document_completion(HELDOUT)),
        ("document_completion(nothing left)", lambda: m.document_completion(["zz"])),
        ("left_to_right", lambda: m.left_to_right(HELDOUT, particles=2)),
        ("export_beta", lambda: quietly(m.export_beta, str(tmp_path / "beta"), 2)),
        ("export_gamma", lambda: quietly(m.export_gamma, str(tmp_path / "gamma"))),
    ]


def quietly(export, *arguments):
    with np.errstate(all="ignore"):         # (the stand-in's counts are zeros: the exports normalise 0 / 0)
        export(*arguments)


def run_script(name, trace, tmp_path):
    """[(step, the context's calls during it, the engine's counters after it)]"""
    m = _engine(name)
    fold_in = "fold_in" if hasattr(m, "fold_in") else "inference"
    steps = []

    def step(label, action, engine):
        action()
        steps.append((label, trace.take(), _counters(engine)))

    def initialise():
        m._initialize(TRAINING, VOCABULARY, K, 0.5, 0.1)
        if name in ("VariationalBayes", "Hybrid"):
            m._eta = np.full((K, len(VOCABULARY)), 0.25)            # (in place of the random start)
    step("_initialize", initialise, m)
    step("learning", m.learning, m)
    for label, action in _queries(m, tmp_path, fold_in):
        step(label, action, m)
    snapshot = []
    step("pickle", lambda: snapshot.append(pickle.dumps(m)), m)
    restored = pickle.loads(snapshot[0])
    for label, action in _queries(restored, tmp_path, fold_in):
        step("restored: " + label, action, restored)
    step("restored: pickle", lambda: pickle.dumps(restored), restored)
    step("restored: learning", restored.learning, restored)
    step("restored: pickle after learning", lambda: pickle.dumps(restored), restored)
    return steps, sorted(pickle.loads(snapshot[0]).__dict__)


ENGINES = ["MonteCarlo", "CollapsedVariationalBayes", "StochasticCollapsedVariationalBayes", "VariationalBayes", "Hybrid"]


@pytest.mark.parametrize("name", ENGINES)
def test_every_method_asks_the_device_what_it_asked_before(name, recording, tmp_path):
    import engine_surface_recorded as recorded
    steps, keys = run_script(name, recording, tmp_path)
    want_steps, want_keys = recorded.STEPS[name], recorded.SNAPSHOT_KEYS[name]
    assert [label for label, _, _ in steps] == [label for label, _, _ in want_steps]
    for (label, calls, counters), (_, want_calls, want_counters) in zip(steps, want_steps):
        assert calls == want_calls, "%s.%s" % (name, label)
        assert counters == want_counters, "%s.%s" % (name, label)
    assert keys == want_keys                 # a snapshot's dictionary: the same keys, so old pickles and new ones interchange


def test_only_the_gibbs_engine_has_fold_in():
    """launch_test (pylda_amd/cli.py) branches on hasattr(engine, "fold_in")"""
    for name in ENGINES:
        assert hasattr(_engine(name), "fold_in") == (name == "MonteCarlo"), name


@pytest.mark.parametrize("name, counter, fold_in, entry", [
    ("MonteCarlo", "_fold_in_calls", "fold_in", "foldin("),
    ("CollapsedVariationalBayes", "_inference_calls", "inference", "cvb0_foldin("),
    ("StochasticCollapsedVariationalBayes", "_inference_calls", "inference", "cvb0_foldin(")])
def test_a_snapshot_without_the_counter_counts_from_stream_2_to_the_31(name, counter, fold_in, entry, recording):
    """A dictionary shaped like an older __getstate__(), the held-out counter absent: it restores, and its first held-out
    call draws from stream 2^31, the next from 2^31 + 1."""
    m = _engine(name)
    m._initialize(TRAINING, VOCABULARY, K, 0.5, 0.1)
    state = m.__getstate__()
    assert state[counter] == 0
    del state[counter]
    restored = type(m).__new__(type(m))
    restored.__setstate__(state)
    assert counter not in restored.__dict__
    recording.take()
    for n in range(2):
        getattr(restored, fold_in)(HELDOUT)
        calls = [call for call in recording.take() if call.startswith(entry)]
        assert len(calls) == 1 and ", %d, 0)" % (2 ** 31 + n) in calls[0], calls
        assert restored.__dict__[counter] == n + 1
    restored.document_completion(HELDOUT)
    calls = [call for call in recording.take() if call.startswith(entry)]
    assert len(calls) == 1 and ", %d, 0)" % (2 ** 31 + 2) in calls[0] and restored.__dict__[counter] == 3


def test_class_paths_and_stream_bases_stay_where_they_are():
    from pylda_amd import cvb0, hybrid, monte_carlo, scvb0
    assert monte_carlo.MonteCarlo.__module__ == "pylda_amd.monte_carlo"
    assert cvb0.CollapsedVariationalBayes.__module__ == "pylda_amd.cvb0"
    assert scvb0.StochasticCollapsedVariationalBayes.__module__ == "pylda_amd.scvb0"
    assert monte_carlo.FOLD_IN_STREAM_BASE == cvb0.INFERENCE_STREAM_BASE == hybrid.HELDOUT_STREAM_BASE == 1 << 31


if __name__ == "__main__":
    import pathlib
    import tempfile
    _capi.Context = RecordingContext
    all_steps, all_keys = {}, {}
    for engine_name in ENGINES:
        RecordingContext.trace = Trace()
        with tempfile.TemporaryDirectory() as folder:
            all_steps[engine_name], all_keys[engine_name] = run_script(engine_name, RecordingContext.trace, pathlib.Path(folder))
    print('"""What tests/test_engine_surface_host.py recorded: per engine the steps of its script as (step, the device context\'s\n'
          'calls during it, the engine\'s counters after it), and the keys of a snapshot\'s dictionary."""')
    print("STEPS = " + pprint.pformat(all_steps, width=150))
    print("SNAPSHOT_KEYS = " + pprint.pformat(all_keys, width=150, compact=True))

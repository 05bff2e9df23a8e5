"""Nearest documents without a GPU: the numpy restatement (tests/similarity_restatement.py) against its brute-force form and
hand cases, SimilarDocuments.distance, the new entry points in header and binding, the engines' methods, the command line's
flag, the kernels' resources from the compiler's own metadata, and the benchmark's kernel-source hash."""
import hashlib
import math
import os
import re
import sys

import numpy as np
import pytest

import similarity_restatement as spec
from conftest import ROOT

CASES = [(1, 1, 1, 1, 0), (3, 7, 3, 1, 0), (5, 9, 4, 12, 0), (4, 30, 10, 5, 1), (6, 20, 17, 20, 2), (2, 64, 1, 64, 2)]


def _rows(rng, n, K, t):
    return rng.standard_normal((n, K)) if t == 0 else rng.gamma(0.3, size=(n, K)) + 1e-9


@pytest.mark.parametrize("Q,D,K,N,t", CASES)
def test_restatement_equals_brute_force(Q, D, K, N, t):
    rng = np.random.default_rng(Q * 1000 + D + K + N)
    a, b = _rows(rng, Q, K, t), _rows(rng, D, K, t)
    b[D // 2] = b[0]                                                     # (a tie, where D > 1)
    self_ids = np.where(np.arange(Q) % 2 == 0, np.arange(Q) % D, -1)
    ta, tb = spec.transform(a, t), spec.transform(b, t)
    assert np.array_equal(ta, np.array(spec.brute_transform(a, t))) and np.array_equal(tb, np.array(spec.brute_transform(b, t)))
    score = spec.scores(ta, tb)
    assert np.array_equal(score, np.array(spec.brute_scores(ta, tb)))
    for selfs in (None, self_ids):
        ids, values = spec.top(score, N, selfs)
        assert ids.dtype == np.int32 and ids.shape == values.shape == (Q, N)
        want = spec.brute_top(score.tolist(), N, None if selfs is None else [int(s) if s >= 0 else None for s in selfs])
        assert ids.tolist() == [[d for d, _ in row] for row in want]
        assert values.tolist() == [[x for _, x in row] for row in want]
        again = spec.nearest(b, t, a, t, N, selfs)
        assert np.array_equal(again[0], ids) and np.array_equal(again[1], values)


def test_restatement_on_the_hand_case():
    """3 documents over 2 topics, gamma rows (1, 3), (2, 2), (3, 1); the query (1, 3).
    transform 1: theta = (1/4, 3/4), (1/2, 1/2), (3/4, 1/4); the scores of the query are 1/16 + 9/16 = 5/8,
    1/8 + 3/8 = 1/2 and 3/16 + 3/16 = 3/8 - all exact in binary: documents 0, 1, 2.  Leaving out document 0: 1, 2, and a
    third entry (-1, -inf).
    transform 2: sqrt(theta); with itself the query scores (1/2)^2 + (sqrt(3)/2)^2, 1 to the last bit or two, and the
    Hellinger distance to itself is 0 within sqrt(2^-52); to document 2 the coefficient is 2 sqrt(3)/4 = 0.8660..."""
    base = np.array([[1.0, 3.0], [2.0, 2.0], [3.0, 1.0]])
    query = base[:1]
    assert spec.transform(base, 1).tolist() == [[0.25, 0.75], [0.5, 0.5], [0.75, 0.25]]
    ids, values = spec.nearest(base, 1, query, 1, 3)
    assert ids.tolist() == [[0, 1, 2]] and values.tolist() == [[0.625, 0.5, 0.375]]
    ids, values = spec.nearest(base, 1, query, 1, 3, np.array([0]))
    assert ids.tolist() == [[1, 2, -1]] and values.tolist() == [[0.5, 0.375, -math.inf]]
    ids, values = spec.nearest(base, 2, query, 2, 3)
    assert ids.tolist() == [[0, 1, 2]]
    assert values[0, 0] == pytest.approx(1.0, abs=4e-16) and values[0, 2] == pytest.approx(math.sqrt(3) / 2, rel=1e-15)
    distance = spec.hellinger(values, ids)
    assert distance[0, 0] <= 2.0 ** -26 and distance[0, 2] == pytest.approx(math.sqrt(1 - math.sqrt(3) / 2), rel=1e-14)
    # one-hot queries under transform 0 against theta: the score is theta_dk itself
    ids, values = spec.nearest(base, 1, np.eye(2), 0, 2)
    assert ids.tolist() == [[2, 1], [0, 1]] and values.tolist() == [[0.75, 0.5], [0.75, 0.5]]


def test_ties_and_padding_by_hand():
    score = np.array([[1.0, 2.0, 2.0, 0.5, 2.0], [0.0, -0.0, 0.0, 0.0, 0.0]])
    ids, values = spec.top(score, 4)
    assert ids.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]] and values[0].tolist() == [2.0, 2.0, 2.0, 1.0]
    ids, values = spec.top(score, 7, np.array([2, -1]))
    assert ids.tolist() == [[1, 4, 0, 3, -1, -1, -1], [0, 1, 2, 3, 4, -1, -1]]
    assert values[0].tolist() == [2.0, 2.0, 1.0, 0.5, -math.inf, -math.inf, -math.inf]
    assert spec.brute_top(score.tolist(), 7, [2, None])[0] == [(1, 2.0), (4, 2.0), (0, 1.0), (3, 0.5)] + [(-1, -math.inf)] * 3


def test_similar_documents_distance():
    from pylda_amd.similarity import SimilarDocuments, hellinger_distance
    ids = np.array([[4, 0, -1], [2, -1, -1]], dtype=np.int32)
    affinity = np.array([[1.0 + 2.0 ** -52, 0.75, -np.inf], [0.0, -np.inf, -np.inf]])
    result = SimilarDocuments(ids, affinity, "hellinger", 5)
    assert result.distance.tolist() == [[0.0, 0.5, math.inf], [1.0, math.inf, math.inf]]      # (1 - BC clamped at 0)
    assert np.array_equal(result.distance, spec.hellinger(affinity, ids)) and np.array_equal(hellinger_distance(affinity, ids), result.distance)
    assert result.metric == "hellinger" and result.documents == 5 and result.ids is ids and result.affinity is affinity
    assert SimilarDocuments(ids, affinity, "dot", 5).distance is None
    assert sorted(result.as_dict()) == ["affinity", "distance", "documents", "ids", "metric", "query_rows"]


def test_header_and_binding_carry_the_two_entry_points_at_abi_10():
    from pylda_amd import _capi
    header = open(os.path.join(ROOT, "include", "pylda_hip.h")).read()
    assert re.search(r"#define PYLDA_ABI_VERSION (\d+)", header).group(1) == str(_capi.ABI_VERSION) == "10"
    for name in ("pylda_similarity_set_base", "pylda_similar_documents"):
        assert re.search(r"\bint %s\(" % name, header) and name in _capi.SIGNATURES
    changelog = header[header.index(" *  10  additions only"):header.index("A host compiled against another version")]
    assert "pylda_similarity_set_base" in changelog and "pylda_similar_documents" in changelog
    assert len(_capi.SIGNATURES["pylda_similarity_set_base"][1]) == 4 and len(_capi.SIGNATURES["pylda_similar_documents"][1]) == 8
    assert callable(_capi.Context.similarity_set_base) and callable(_capi.Context.similar_documents)
    assert "similarity_doc_slices" in header


def test_engines_offer_the_methods():
    import inspect
    from pylda_amd.hybrid import Hybrid
    from pylda_amd.monte_carlo import MonteCarlo
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    for method in ("similar_documents", "top_documents"):
        assert getattr(Hybrid, method) is getattr(VariationalBayes, method)
        assert getattr(OnlineVariationalBayes, method) is getattr(VariationalBayes, method)
        assert callable(getattr(MonteCarlo, method))
    # one body for every engine (pylda_amd/analysis.py): the engines differ in their rows and, for similar_documents, in
    # the fit options their signature names
    assert MonteCarlo.top_documents is VariationalBayes.top_documents
    assert MonteCarlo.similar_documents is not VariationalBayes.similar_documents
    assert MonteCarlo._similar_documents is VariationalBayes._similar_documents
    assert MonteCarlo._document_rows is not VariationalBayes._document_rows
    parameters = inspect.signature(VariationalBayes.similar_documents).parameters
    assert [(n, p.default) for n, p in parameters.items()][1:] == [("queries", None), ("top", 10), ("metric", "hellinger")]
    parameters = inspect.signature(MonteCarlo.similar_documents).parameters
    assert list(parameters)[1:] == ["queries", "top", "metric", "number_of_samples", "burn_in_samples"]
    assert inspect.signature(VariationalBayes.top_documents).parameters["top"].default == 10


def test_engines_refuse_bad_arguments_and_a_process_group(monkeypatch):
    from pylda_amd import distributed, similarity

    class Engine(object):
        _process_group = None

    rows = np.ones((3, 2))
    sharded = Engine()
    sharded.__dict__["_process_group"] = object()
    monkeypatch.setattr(distributed, "world_of", lambda group=None: 2)
    with pytest.raises(NotImplementedError):
        similarity.similar_documents(sharded, rows, None, 10, "hellinger", None)
    with pytest.raises(NotImplementedError):
        similarity.top_documents(sharded, rows, 10)
    with pytest.raises(ValueError):
        similarity.similar_documents(Engine(), rows, None, 10, "cosine", None)
    for top in (0, 65):
        with pytest.raises(ValueError):
            similarity.similar_documents(Engine(), rows, None, top, "hellinger", None)
        with pytest.raises(ValueError):
            similarity.top_documents(Engine(), rows, top)
    with pytest.raises(RuntimeError):
        similarity.similar_documents(Engine(), None, None, 10, "hellinger", None)
    with pytest.raises(ValueError):
        similarity.similar_documents(Engine(), rows, np.ones((2, 3)), 10, "hellinger", None)


def test_command_line_flag_defaults_to_off():
    import inspect
    from pylda_amd import cli
    base = ["--input_directory=a", "--model_directory=b"]
    assert cli._parse(cli.TEST_FLAGS, base, "launch_test").similar_documents == 0
    assert cli._parse(cli.TEST_FLAGS, base + ["--similar_documents=5"], "launch_test").similar_documents == 5
    assert inspect.signature(cli.evaluate_snapshot).parameters["similar_documents"].default == 0
    for bad in ("-1", "65"):
        with pytest.raises(SystemExit):
            cli.test_main(base + ["--similar_documents=" + bad])


def test_similarity_kernels_use_no_scratch():
    """Every similarity_* kernel the library ships, from the compiler's own metadata: no scratch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    lines = open(kr.compile_to_asm(os.path.join(ROOT, "pylda_amd", "csrc", "launch_similarity.hip"))).read().splitlines()
    res = kr.resources(lines, "similarity_")
    names = kr.demangle(list(res))
    shipped = sorted(names[m] for m in res)
    for kernel in ("similarity_transform_kernel", "similarity_topn_kernel", "similarity_merge_kernel"):
        assert sum(kernel in n for n in shipped) == 1, shipped
    assert len(shipped) == 3, shipped
    for mangled, info in res.items():
        print(names[mangled], info)
        assert info["ScratchSize"] == 0, (names[mangled], info)


def test_kernel_source_hash_is_what_it_was_without_the_new_files():
    """bench.kernel_source_hash() over csrc/ equals the hash of the file list that leaves this feature's files out."""
    import bench
    csrc = os.path.join(ROOT, "pylda_amd", "csrc")
    new_files = ("similarity_kernels.h", "launch_similarity.hip", "topn_list.h")
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

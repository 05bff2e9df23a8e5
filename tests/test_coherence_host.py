"""Topic coherence without a GPU: the numpy restatement (tests/coherence_restatement.py) against its brute-force form and a
hand case, pylda_amd.coherence.scores_from_counts against the restatement, the new entry points in header and binding, the
engines' methods, the command line's flag, the binding helper's rebuild message, the kernels' resources from the compiler's
own metadata, and the benchmark's kernel-source hash."""
import hashlib
import math
import os
import re
import sys

import numpy as np
import pytest

import coherence_restatement as spec
from conftest import ROOT

CASES = [(1, 5, 5, 1, None), (2, 9, 1, 7, None), (3, 40, 8, 64, None), (4, 30, 6, 65, 3), (5, 12, 12, 130, 2), (2, 70, 64, 20, 3)]


def _hand_case():
    doc_ptr = np.array([0, 2, 4, 5, 7], dtype=np.int64)
    term_id = np.array([0, 1, 0, 2, 2, 0, 1], dtype=np.int32)
    table = np.array([[5, 3, 3, 1, 0], [1, 0, 7, 2, 0]], dtype=np.float64)
    return table, doc_ptr, term_id


@pytest.mark.parametrize("K,V,M,D,levels", CASES)
def test_restatement_equals_brute_force(K, V, M, D, levels):
    rng = np.random.default_rng(K * 1000 + V + M + D)
    table, doc_ptr, term_id, _ = spec.random_case(rng, K, V, M, D, levels=levels)
    got = spec.coherence(table, M, doc_ptr, term_id)
    ids = spec.brute_top_words(table, M)
    assert got["top_ids"].tolist() == ids
    assert np.array_equal(got["top_values"], np.array([[table[k][v] for v in ids[k]] for k in range(K)]))
    doc_freq, co = spec.brute_counts(doc_ptr, term_id, ids)
    assert got["doc_freq"].tolist() == doc_freq and got["co_doc_freq"].tolist() == co
    for k, (umass, npmi, undefined) in enumerate(spec.brute_scores(doc_freq, co, D)):
        assert got["umass"][k] == pytest.approx(umass, rel=1e-12, abs=1e-13)
        assert got["npmi"][k] == pytest.approx(npmi, rel=1e-12, abs=1e-13)
        assert got["undefined_pairs"][k] == undefined


def test_restatement_on_the_hand_case():
    """4 documents over 5 words: {0, 1}, {0, 2}, {2}, {0, 1}; words 3 and 4 occur nowhere.
    D = 4; D(0) = 3, D(1) = 2, D(2) = 2, D(3) = 0; D(0, 1) = 2, D(0, 2) = 1, D(1, 2) = 0.

    Topic 0, row (5, 3, 3, 1, 0): word 0, then the tie of words 1 and 2 at 3, which the smaller id wins: (0, 1, 2).
      pair (v_m, v_l)   D(v_m, v_l)  D(v_l)   UMass term        NPMI term
      (1, 0)            2            3        log(3 / 3) = 0    log((2/4) / ((2/4)(3/4))) / -log(2/4) = log(4/3) / log 2
      (2, 0)            1            3        log(2 / 3)        log((1/4) / ((2/4)(3/4))) / -log(1/4) = log(2/3) / log 4
      (2, 1)            0            2        log(1 / 2)        -1: the two never share a document
      UMass = log(1/3), NPMI = (log(4/3) / log 2 + log(2/3) / log 4 - 1) / 3, no undefined pair.
    Topic 1, row (1, 0, 7, 2, 0): (2, 3, 0); word 3 occurs nowhere.
      (3, 2)            0            2        log(1 / 2)        -1
      (0, 2)            1            2        log(2 / 2) = 0    log(2/3) / log 4
      (0, 3)            0            0        undefined: 0      -1
      UMass = log(1/2), NPMI = (log(2/3) / log 4 - 2) / 3, one undefined pair."""
    table, doc_ptr, term_id = _hand_case()
    got = spec.coherence(table, 3, doc_ptr, term_id)
    assert got["top_ids"].tolist() == [[0, 1, 2], [2, 3, 0]] and got["top_values"].tolist() == [[5, 3, 3], [7, 2, 1]]
    assert got["doc_freq"].tolist() == [[3, 2, 2], [2, 0, 3]]
    assert got["co_doc_freq"].tolist() == [[[3, 2, 1], [2, 2, 0], [1, 0, 2]], [[2, 0, 1], [0, 0, 0], [1, 0, 3]]]
    assert got["documents"] == 4 and got["undefined_pairs"].tolist() == [0, 1]
    assert got["umass"][0] == pytest.approx(math.log(1 / 3), rel=1e-15) and got["umass"][1] == pytest.approx(math.log(1 / 2), rel=1e-15)
    assert got["npmi"][0] == pytest.approx((math.log(4 / 3) / math.log(2) + math.log(2 / 3) / math.log(4) - 1) / 3, rel=1e-15)
    assert got["npmi"][1] == pytest.approx((math.log(2 / 3) / math.log(4) - 2) / 3, rel=1e-15)
    assert got["umass_mean"] == pytest.approx((math.log(1 / 3) + math.log(1 / 2)) / 2, rel=1e-15)
    # one top word: nothing to pair
    one = spec.coherence(table, 1, doc_ptr, term_id)
    assert one["umass"].tolist() == [0, 0] and one["npmi"].tolist() == [0, 0] and one["undefined_pairs"].tolist() == [0, 0]
    # a pair that every document holds scores 0
    every = spec.scores(np.array([[4, 4]]), np.array([[[4, 4], [4, 4]]]), 4)
    assert every[1].tolist() == [0.0] and every[0][0] == math.log(5 / 4)


@pytest.mark.parametrize("K,V,M,D,levels", CASES + [(None, 5, 3, 4, None)])       # (K None: the hand case)
def test_scores_from_counts_equal_the_restatement(K, V, M, D, levels):
    from pylda_amd.coherence import TopicCoherence, scores_from_counts
    if K is None:
        table, doc_ptr, term_id = _hand_case()
    else:
        table, doc_ptr, term_id, _ = spec.random_case(np.random.default_rng(K * 1000 + V + M + D), K, V, M, D, levels=levels)
    want = spec.coherence(table, M, doc_ptr, term_id)
    umass, npmi, undefined = scores_from_counts(want["doc_freq"], want["co_doc_freq"], D)
    assert umass.shape == npmi.shape == undefined.shape == (len(table),)
    np.testing.assert_allclose(umass, want["umass"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(npmi, want["npmi"], rtol=1e-12, atol=1e-13)
    assert np.array_equal(undefined, want["undefined_pairs"])
    result = TopicCoherence(want["top_ids"], want["top_values"], want["doc_freq"], want["co_doc_freq"], D)
    assert sorted(result.as_dict()) == sorted(want)
    assert result.documents == D and result.top_words_count == M
    assert result.umass_mean == pytest.approx(want["umass_mean"], rel=1e-12, abs=1e-13)
    assert result.npmi_mean == pytest.approx(want["npmi_mean"], rel=1e-12, abs=1e-13)


def test_header_and_binding_carry_the_two_entry_points_at_abi_10():
    from pylda_amd import _capi
    header = open(os.path.join(ROOT, "include", "pylda_hip.h")).read()
    assert re.search(r"#define PYLDA_ABI_VERSION (\d+)", header).group(1) == str(_capi.ABI_VERSION) == "10"
    for name in ("pylda_top_words", "pylda_codocument_counts"):
        assert re.search(r"\bint %s\(" % name, header) and name in _capi.SIGNATURES
    changelog = header[header.index(" *  10  additions only"):header.index("A host compiled against another version")]
    assert "pylda_top_words" in changelog and "pylda_codocument_counts" in changelog
    assert len(_capi.SIGNATURES["pylda_top_words"][1]) == 5 and len(_capi.SIGNATURES["pylda_codocument_counts"][1]) == 6
    assert callable(_capi.Context.top_words) and callable(_capi.Context.codocument_counts)
    assert "coherence_chunk_docs" in header


def test_engines_offer_the_methods():
    from pylda_amd.hybrid import Hybrid
    from pylda_amd.monte_carlo import MonteCarlo
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    for method in ("topic_coherence", "top_words"):
        assert getattr(Hybrid, method) is getattr(VariationalBayes, method)
        assert getattr(OnlineVariationalBayes, method) is getattr(VariationalBayes, method)
        # one definition for every engine (pylda_amd/analysis.py); what differs is the table an engine puts under it
        assert callable(getattr(MonteCarlo, method)) and getattr(MonteCarlo, method) is getattr(VariationalBayes, method)
    assert MonteCarlo._device_topic_table is not VariationalBayes._device_topic_table


def test_command_line_flag_defaults_to_off():
    import inspect
    from pylda_amd import cli
    base = ["--input_directory=a", "--model_directory=b"]
    assert cli._parse(cli.TEST_FLAGS, base, "launch_test").topic_coherence == 0
    assert cli._parse(cli.TEST_FLAGS, base + ["--topic_coherence=5"], "launch_test").topic_coherence == 5
    assert inspect.signature(cli.evaluate_snapshot).parameters["topic_coherence"].default == 0


def test_binding_helper_gives_the_rebuild_message_for_a_missing_symbol():
    from pylda_amd import _capi

    class Function(object):
        restype = argtypes = None

    class Stub(object):
        """A library built before pylda_codocument_counts existed."""
        def __getattr__(self, name):
            if name == "pylda_codocument_counts" or name not in _capi.SIGNATURES:
                raise AttributeError(name)
            function = Function()
            setattr(self, name, function)
            return function

    with pytest.raises(RuntimeError) as e:
        _capi._bind(Stub(), "/somewhere/libpylda_hip.so")
    message = str(e.value)
    assert "pylda_codocument_counts" in message and "python -m pylda_amd.build --force" in message and "/somewhere/libpylda_hip.so" in message

    class Whole(Stub):
        def __getattr__(self, name):
            if name not in _capi.SIGNATURES:
                raise AttributeError(name)
            function = Function()
            setattr(self, name, function)
            return function
    whole = Whole()
    assert _capi._bind(whole) is whole
    assert whole.pylda_top_words.argtypes == _capi.SIGNATURES["pylda_top_words"][1]


def test_coherence_kernels_use_no_scratch():
    """Every coherence_* kernel the library ships, from the compiler's own metadata: no scratch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    lines = open(kr.compile_to_asm(os.path.join(ROOT, "pylda_amd", "csrc", "launch_coherence.hip"))).read().splitlines()
    res = kr.resources(lines, "coherence_")
    names = kr.demangle(list(res))
    shipped = sorted(names[m] for m in res)
    for kernel in ("coherence_select_kernel", "coherence_mark_kernel", "coherence_pair_kernel"):
        assert sum(kernel in n for n in shipped) == 1, shipped
    assert len(shipped) == 3, shipped
    for mangled, info in res.items():
        print(names[mangled], info)
        assert info["ScratchSize"] == 0, (names[mangled], info)


def test_kernel_source_hash_is_what_it_was_without_the_new_files():
    """bench.kernel_source_hash() over csrc/ equals the hash of the file list that leaves this feature's files out."""
    import bench
    csrc = os.path.join(ROOT, "pylda_amd", "csrc")
    new_files = ("coherence_kernels.h", "launch_coherence.hip")
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

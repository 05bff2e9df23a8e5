"""Document completion without a GPU: the split of pylda_amd.corpus against its token-by-token restatement
(tests/completion_restatement.py), the estimator on a hand case in exact binary fractions, the new entry points in header and
binding, the command line's flag, and the kernels' resources from the compiler's own assembly."""
import math
import os
import re
import sys

import numpy as np

import completion_restatement as spec
from conftest import ROOT


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_split_of_the_example():
    from pylda_amd.corpus import split_for_completion
    observed, held = split_for_completion([0, 3], [10, 11, 12], [3, 1, 2])           # (a:3, b:1, c:2)
    assert observed[0].tolist() == [0, 2] and observed[1].tolist() == [10, 12] and observed[2].tolist() == [2, 1]
    assert held[0].tolist() == [0, 3] and held[1].tolist() == [10, 11, 12] and held[2].tolist() == [1, 1, 1]
    assert _same(observed, spec.split([0, 3], [10, 11, 12], [3, 1, 2])[0]) and _same(held, spec.split([0, 3], [10, 11, 12], [3, 1, 2])[1])


def test_split_of_the_associated_press_test_documents(ap_test):
    from pylda_amd.corpus import split_for_completion
    ptr, ids, cts = ap_test["doc_ptr"], ap_test["term_id"], ap_test["term_ct"]
    observed, held = split_for_completion(ptr, ids, cts)
    want = spec.split(ptr, ids, cts)
    assert _same(observed, want[0]) and _same(held, want[1])
    D, V = len(ptr) - 1, int(ids.max()) + 1
    assert len(observed[0]) == len(held[0]) == D + 1

    def dense(csr):
        out = np.zeros((D, V), dtype=np.int64)
        np.add.at(out, (np.repeat(np.arange(D), np.diff(csr[0])), csr[1]), csr[2])
        return out
    assert np.array_equal(dense(observed) + dense(held), dense((ptr, ids, cts)))
    tokens_observed, tokens_held = dense(observed).sum(axis=1), dense(held).sum(axis=1)
    assert np.all(tokens_observed - tokens_held >= 0) and np.all(tokens_observed - tokens_held <= 1)
    assert np.all(observed[2] > 0) and np.all(held[2] > 0)
    assert np.all(np.diff(observed[0])[np.diff(ptr) > 0] > 0)
    # the terms keep their order: each half's ids are a subsequence of the document's
    for d in (0, 7, D - 1):
        whole = ids[ptr[d]:ptr[d + 1]].tolist()
        for half in (observed, held):
            it = iter(whole)
            assert all(t in it for t in half[1][half[0][d]:half[0][d + 1]].tolist())


def test_split_of_a_single_token_an_empty_document_and_a_300_fold_term():
    from pylda_amd.corpus import split_for_completion
    csr = ([0, 1, 1, 3, 5], [4, 9, 2, 1, 9], [1, 300, 1, 1, 300])
    observed, held = split_for_completion(*csr)
    assert _same(observed, spec.split(*csr)[0]) and _same(held, spec.split(*csr)[1])
    assert observed[0].tolist() == [0, 1, 1, 3, 5] and observed[1].tolist() == [4, 9, 2, 1, 9] and observed[2].tolist() == [1, 150, 1, 1, 150]
    assert held[0].tolist() == [0, 0, 0, 1, 2] and held[1].tolist() == [9, 9] and held[2].tolist() == [150, 150]
    empty = split_for_completion([0], [], [])
    assert empty[0][0].tolist() == [0] and empty[1][0].tolist() == [0] and len(empty[0][1]) == len(empty[1][2]) == 0


def test_hand_case_in_exact_binary_fractions():
    """P[0] = (1/4, 3/4), theta = (1/4, 3/4): p = 1/16 + 9/16 = 0.625, every step exact."""
    P = spec.predictive_table([[1, 2, 1], [3, .5, .5]])
    assert P.tolist() == [[0.25, 0.75], [0.5, 0.125], [0.25, 0.125]]
    doc_ll, tokens, terms = spec.score([0, 1], [0], [2], P, [[1.0, 3.0]])
    assert doc_ll[0] == 2 * math.log(0.625) and tokens.tolist() == [2] and terms.tolist() == [1]
    empty = spec.score([0, 0], [], [], P, [[1.0, 3.0]])
    assert empty[0].tolist() == [0.0] and empty[1].tolist() == [0]
    assert spec.bar(3, 2, tokens, terms, doc_ll)[0] == (3 + 4 + 64) * 2.0 ** -53 * 2 + 2.0 ** -53 * abs(doc_ll[0])


def test_header_and_binding_carry_the_two_entry_points_at_abi_9():
    from pylda_amd import _capi
    header = open(os.path.join(ROOT, "include", "pylda_hip.h")).read()
    assert re.search(r"#define PYLDA_ABI_VERSION (\d+)", header).group(1) == str(_capi.ABI_VERSION) == "10"
    for name in ("pylda_completion_set_model", "pylda_completion_score"):
        assert re.search(r"\bint %s\(" % name, header) and name in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["pylda_completion_score"][1]) == 6
    assert callable(_capi.Context.completion_set_model) and callable(_capi.Context.completion_score)


def test_engines_offer_the_method():
    from pylda_amd.hybrid import Hybrid
    from pylda_amd.monte_carlo import MonteCarlo
    from pylda_amd.online_vb import OnlineVariationalBayes
    from pylda_amd.variational_bayes import VariationalBayes
    assert OnlineVariationalBayes.document_completion is VariationalBayes.document_completion
    assert Hybrid.document_completion is not VariationalBayes.document_completion
    assert callable(MonteCarlo.document_completion)


def test_command_line_flag_defaults_to_off():
    from pylda_amd import cli
    base = ["--input_directory=a", "--model_directory=b"]
    assert cli._parse(cli.TEST_FLAGS, base, "launch_test").document_completion == 0
    assert cli._parse(cli.TEST_FLAGS, base + ["--document_completion=1"], "launch_test").document_completion == 1


def test_completion_kernels_use_no_scratch():
    """Every completion_* kernel the library ships, from the compiler's own metadata: no scratch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    lines = open(kr.compile_to_asm(os.path.join(ROOT, "pylda_amd", "csrc", "launch_completion.hip"))).read().splitlines()
    res = kr.resources(lines, "completion_")
    names = kr.demangle(list(res))
    shipped = sorted(names[m] for m in res)
    for kernel in ("completion_rowsum_kernel", "completion_table_kernel", "completion_sum_kernel"):
        assert sum(kernel in n for n in shipped) == 1, shipped
    slots = sorted(int(re.search(r"completion_score_kernel<(\d+)", n).group(1)) for n in shipped if "completion_score_kernel" in n)
    assert slots == [1, 2, 4, 8, 16], shipped
    for mangled, info in res.items():
        print(names[mangled], info)
        assert info["ScratchSize"] == 0, (names[mangled], info)

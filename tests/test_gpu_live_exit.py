"""The live-topic kernel (estep_compact.h) without the per-iteration work no result needs (estep_limits.h
live_stop_shortcut, live_guard_once, live_raw_extremes): not a bit of a result may move.

The cases of tests/live_exit_cases.py - K = 256 (pair stage and single stage) and K = 128, 96 documents whose term
counts sit at the slot boundaries of two, three and four term slots per lane, thresholds 1e-2 .. 1e-6 at hand-over
counts 4, 20 and 56 - against what the commit before gave on an MI355X (tests/golden/live_exit_k256.npz, recorded by
tests/golden/make_live_exit_golden.py): SHA-256 of gamma, the iteration counts, the statistics, the joint value and the
executed work on the training fast path (document terms by doc_terms_kernel) and with per-document values (the
kernel's own epilogue; there the per-document log-likelihood too), and against the C oracle at the suite's bars.

The stop test is exercised on both sides.  Hand-over is not reported per document, so the documents that stop INSIDE
the live-topic kernel are bounded from below: of H documents handed over at most `at cap` (all documents that ran to
the iteration cap) did not stop there, so at least H - at cap did.  That bound must reach a quarter of H at hand-over
counts 20 and 56 in every case, and per threshold over the three hand-over counts together (a test of its own; at
count 4 a handful of these documents is handed over at all: 0 .. 6 on the recorded commit).  The model was chosen on the
CPU so that the oracle alone leaves room for it (test_the_oracle_alone_stops_documents_before_the_cap).  The work
counters show which way the stop test was taken: the full sum in every case that hands documents over (the iteration a
document stops in forms it), the shortcut too in every case at thresholds of 1e-3 and below (at 1e-2 a document stops as
soon as no topic moves by more than the threshold on its own: there is next to nothing to skip).

The range check (estep_compact.h compact_range_check): option compact_underflow_doc scales, between the dense kernel
and the live-topic kernel, the hand-over tile's entries of the LAST term of a 65-term document by 1e-288 - a scale
per term cancels in everything but the term's normaliser, which is then below the kernel's 1e-280 from the first
iteration run there.  alpha = 1e-3 makes t of a dead topic an exact zero, so the exactness guard's two bounds hold and
the range check is the only thing that can flag; the failing term sits on lane 0 of the second slot beside 63 padded
slots.  The document must end flagged (status 1) and redone by the log-space kernel, alone, as on the parent commit's
kernels run with the same hook (recorded in the golden file); without the hook nothing is flagged.  The exit the check
shares with the exactness guard is also driven for every document (option compact_guard_fail).  The log-space kernel adds
its statistics with atomics in no fixed order: they, and the joint value that holds their corpus term, are held to the
oracle, everything else to the recorded bits.  Needs an MI355X."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
import live_exit_cases as cases

GAMMA_RTOL_ORACLE, LL_RTOL, SSTATS_ATOL = 1e-7, 1e-9, 1e-8          # tests/test_gpu_live_topics.py


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def recorded():
    return load_golden("live_exit_k256.npz")


@pytest.mark.parametrize("name", list(cases.MODELS))
def test_the_oracle_alone_stops_documents_before_the_cap(name):
    """CPU: at every threshold at most a third of the documents run to the iteration cap in the C oracle, so with every
    document handed over two thirds of them stop inside the live-topic kernel - and the lengths are the slot boundaries."""
    ptr = cases.inputs(name)[0]
    assert {65, 128, 129, 192, 193, 208, 256} <= set(np.diff(ptr).tolist()) and len(ptr) - 1 == cases.D
    for tol in cases.TOLS:
        assert cases.stops_before_the_cap(cases.reference(name, tol)["iters"]) >= 2 * cases.D // 3, tol


_runs = {}


def result(capi, name, cap, tol, fast):
    """An E-step of the sweep: run once, shared among the tests, never modified."""
    key = (name, cap, tol, fast)
    if key not in _runs:
        _runs[key] = cases.run(capi, name, tol, (("compact_cap", cap),), fast)
    return _runs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", cases.CAPS)
@pytest.mark.parametrize("name", list(cases.MODELS))
def test_results_keep_their_bits_and_the_stop_test_works_on_both_sides(capi, recorded, name, cap):
    for tol in cases.TOLS:
        ref = cases.reference(name, tol)
        for fast in (True, False):
            what = "%s compact_cap=%d tol=%g %s" % (name, cap, tol, "fast path" if fast else "per-document values")
            out = result(capi, name, cap, tol, fast)
            handed, at_cap = out["handed_over"], cases.D - cases.stops_before_the_cap(out["iters"])
            skipped, formed = out["stop_sums"]
            print("%s: handed over %d, at the cap %d, stop sums skipped %d formed %d" % (what, handed, at_cap, skipped, formed))
            assert out["flagged"] == 0, what
            assert handed == float(recorded[cases.key_of(name, cap, tol, fast, "handed_over")]), what
            for field, d in cases.digests(out, fast).items():
                assert d.encode() == bytes(recorded[cases.key_of(name, cap, tol, fast, field)]), (what, field)
            assert np.array_equal(out["iters"], ref["iters"]), what
            assert rel_err(out["gamma"], ref["gamma"]) < GAMMA_RTOL_ORACLE, what
            assert np.max(np.abs(out["sstats"] - ref["sstats"])) < SSTATS_ATOL, what
            assert rel_err(out["joint"], ref["document_log_likelihood"]) < LL_RTOL, what
            if not fast:
                assert rel_err(out["doc_ll"], ref["doc_ll"]) < LL_RTOL, what
            # both sides of the stop test, and both ways of taking it
            if cap >= 20:
                assert handed > 0 and handed - at_cap >= handed / 4.0, what
                assert formed > 0, what
                if tol <= 1e-3:
                    assert skipped > 0, what


@pytest.mark.gpu
@pytest.mark.parametrize("tol", cases.TOLS)
@pytest.mark.parametrize("name", list(cases.MODELS))
def test_a_quarter_of_the_documents_handed_over_stop_inside_the_kernel(capi, name, tol):
    """Per threshold, over the three hand-over counts together (the bound of the module's docstring)."""
    handed = inside = 0.0
    for cap in cases.CAPS:
        out = result(capi, name, cap, tol, True)
        handed += out["handed_over"]
        inside += max(0.0, out["handed_over"] - (cases.D - cases.stops_before_the_cap(out["iters"])))
    assert handed > 0 and inside >= handed / 4.0, (name, tol, handed, inside)


@pytest.mark.gpu
def test_a_normaliser_that_underflows_inside_the_kernel_sends_its_document_to_the_log_space_kernel(capi, recorded):
    ref = cases.underflow_reference()
    (ptr, _, _, _, _), doc = cases.underflow_inputs()
    assert ptr[doc + 1] - ptr[doc] == cases.UNDERFLOW_N == 65
    for fast in (True, False):
        plain, out = cases.run_underflow(capi, False, fast), cases.run_underflow(capi, True, fast)
        key = lambda field: cases.key_of("underflow", cases.UNDERFLOW_CAP, 1e-6, fast, field)      # noqa: E731
        assert plain["flagged"] == 0 and plain["handed_over"] == out["handed_over"] == float(recorded[key("handed_over")]) > 0
        assert out["flagged"] == int(recorded[key("flagged")]) == 1
        for field, d in cases.digests(out, fast).items():
            if field not in ("sstats", "joint"):
                assert d.encode() == bytes(recorded[key(field)]), (fast, field)
        # the other documents are untouched by the hook, the flagged one is the oracle's (redone from the table)
        others = np.arange(cases.D) != doc
        assert np.array_equal(out["gamma"][others], plain["gamma"][others])
        for o in (plain, out):
            assert np.array_equal(o["iters"], ref["iters"])
            assert rel_err(o["gamma"], ref["gamma"]) < GAMMA_RTOL_ORACLE
            assert np.max(np.abs(o["sstats"] - ref["sstats"])) < SSTATS_ATOL
            assert rel_err(o["joint"], ref["document_log_likelihood"]) < LL_RTOL
            if not fast:
                assert rel_err(o["doc_ll"], ref["doc_ll"]) < LL_RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cases.MODELS))
def test_the_flagged_exit_hands_the_same_documents_to_the_log_space_kernel(capi, recorded, name):
    ref = cases.reference(name, 1e-6)
    for fast in (True, False):
        out = cases.run(capi, name, 1e-6, (("compact_guard_fail", 1),), fast)
        assert out["handed_over"] == float(recorded[cases.key_of(name, 0, 1e-6, fast, "guard_fail/handed_over")]) == cases.D
        assert out["flagged"] == int(recorded[cases.key_of(name, 0, 1e-6, fast, "guard_fail/flagged")]) == cases.D
        for field, d in cases.digests(out, fast).items():
            if field not in ("sstats", "joint"):
                assert d.encode() == bytes(recorded[cases.key_of(name, 0, 1e-6, fast, "guard_fail/" + field)]), (fast, field)
        assert np.array_equal(out["iters"], ref["iters"])
        assert rel_err(out["gamma"], ref["gamma"]) < 1e-8 and np.max(np.abs(out["sstats"] - ref["sstats"])) < SSTATS_ATOL
        assert rel_err(out["joint"], ref["document_log_likelihood"]) < LL_RTOL

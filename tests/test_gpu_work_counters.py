"""The profiling counters of an E-step (doc_terms.h: work_count_partial_kernel over many workgroups, then
work_count_kernel's one) against what the single-workgroup kernel of the parent commit summed - recorded on an MI355X in
tests/golden/work_counters_single_workgroup.json by tests/golden/make_work_counters_golden.py.  Every summand is an
integer far below 2^53 held in a double, so the totals do not depend on the order of summation: they must be EQUAL.
Cases: tests/work_counter_cases.py (one row of partial sums, a single document, two rows).  Needs an MI355X."""
import json
import os

import pytest

import work_counter_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "work_counters_single_workgroup.json")


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    _capi.load()
    assert _capi.device_count() >= 1, "no HIP device visible"
    return _capi


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", cases.CASES)
def test_counters_equal_the_single_workgroup_sums(capi, recorded, case):
    out = cases.run(capi, case)
    want = recorded[case]
    for field in cases.FIELDS:
        print("%s %s: %r (recorded %r from %s)" % (case, field, out[field], want[field], recorded["recorded_from"]))
    for field in cases.FIELDS:
        assert float(out[field]).is_integer() and out[field] == want[field], (case, field, out[field], want[field])
    assert out["inner_iterations"] > 0 and out["inner_iteration_terms"] > 0 and out["tile_entries"] > 0
    if case == "K256x96":           # the case that reaches every counter
        assert out["handed_over"] > 0 and out["stop_sums_skipped"] > 0 and out["stop_sums_formed"] > 0
    # the two clock spans: both stages' workgroups time themselves in both clocks
    shader, wall, hz = out["clock_spans"]
    print("%s clock spans: %r shader cycles, %r ticks at %r Hz" % (case, shader, wall, hz))
    assert shader > 0 and wall > 0 and hz > 0

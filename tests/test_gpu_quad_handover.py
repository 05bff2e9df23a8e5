"""The hand-over of the stride-256 quad kernels decided at the bottom of an inner iteration (estep_quad.h,
estep_limits.h quad_early_handoff), where the live count is read, instead of behind the first chunk of the next
iteration's pass A: the same inner iteration, the same bits.

K = 256, the 96 boundary-length documents of tests/test_gpu_quad_slots.py (most topics of a document die), inner-iteration
caps 1 .. 12 x four stop thresholds at hand-over counts 4 and 56 (option compact_cap), against the values the commit
before the early exit gave on an MI355X (tests/golden/quad_handover_k256.npz, recorded by
tests/golden/make_quad_handover_golden.py): iteration counts, executed work (tile entries, documents handed over -
Context.executed_work) and gamma's bits.  That pins the hand-over to the same inner iteration, and a document that meets
the stop test and the hand-over count in the same iteration to finishing in the dense kernel.  Gamma is also held
against the dense kernels alone (compact = 0) at the suite's bar.  Needs an MI355X."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
import quad_handover_cases as cases
import test_gpu_quad_slots as slots

pytestmark = pytest.mark.gpu

GAMMA_RTOL = 1e-9          # live-topic kernel against the dense kernels (tests/test_gpu_live_topics.py)


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def recorded():
    return load_golden("quad_handover_k256.npz")


_dense = {}


@pytest.mark.parametrize("tol", cases.TOLS)
@pytest.mark.parametrize("cap", cases.CAPS)
def test_hand_over_happens_in_the_same_inner_iteration(capi, recorded, cap, tol):
    inputs = slots.inputs_and_reference(cases.K, "hand-over")[0]
    a, b = cases.CAPS.index(cap), cases.TOLS.index(tol)
    if tol not in _dense:
        _dense[tol] = cases.sweep(capi, inputs, slots.V, (("compact", 0),), tol)
    live = cases.sweep(capi, inputs, slots.V, (("compact_cap", cap),), tol)
    # (the sweep does hand documents over - and at the loosest threshold every document stops first)
    assert recorded["handed_over"][:, 2:].max(axis=2).min() > 0 and recorded["handed_over"][:, 0].max() == 0
    for c, (out, dense) in enumerate(zip(live, _dense[tol])):
        what = "compact_cap=%d tol=%g max_iter=%d" % (cap, tol, cases.MAX_ITERS[c])
        assert out["flagged"] == 0 and dense["handed_over"] == 0, what
        assert np.array_equal(out["iters"], recorded["iters"][a, b, c]), what
        assert out["handed_over"] == recorded["handed_over"][a, b, c], what
        assert out["tile_entries"] == recorded["tile_entries"][a, b, c], what
        assert cases.gamma_digest(out["gamma"]).encode() == bytes(recorded["gamma_sha256"][a, b, c]), what
        assert np.array_equal(out["iters"], dense["iters"]), what
        assert rel_err(out["gamma"], dense["gamma"]) < GAMMA_RTOL, what

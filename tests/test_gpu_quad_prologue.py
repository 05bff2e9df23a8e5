"""The packed prologue of the stride-256 quad kernels with its loads requested at once (estep_quad.h, estep_limits.h
quad_prologue_at_once: ids, alpha and sum alpha in front of the record; the two counts requested in front of the row
gather and stored behind it; all rows of the LDS slots requested before the first is stored) must compute what the
prologue before it computed - bit for bit - and what the oracle computes.

The corpora, modes and bars of tests/test_gpu_quad_slots.py at K = 129 / 256 (every slot boundary 159 .. 256 of the quad
classes: one to four LDS slots, the streamed classes, lanes with no count to load): gamma, per-document
log-likelihood, iteration counts and statistics against their SHA-256 as the commit before the change computed them on an
MI355X (tests/golden/quad_handover_k256.npz, keys boundary/..., recorded by tests/golden/make_quad_handover_golden.py -
equality of the digests is np.array_equal of the arrays), against the chain through order / doc_ptr / term_id
(quad_packed = 0, which has no counts to defer) with np.array_equal, and against the C oracle.  Needs an MI355X."""
import numpy as np
import pytest

from conftest import load_golden
import quad_handover_cases as cases
import test_gpu_quad_slots as slots

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return load_golden("quad_handover_k256.npz")


@pytest.mark.parametrize("mode", list(slots.MODES))
@pytest.mark.parametrize("K", cases.BOUNDARY_KS)
def test_prologue_at_once_changes_no_bit_at_the_boundary_lengths(recorded, K, mode):
    from pylda_amd import _capi
    inputs, ref = slots.inputs_and_reference(K, mode)
    kw = slots.MODES[mode]
    heldout = bool(kw.get("heldout"))
    outs = {packed: slots.run(_capi, K, inputs, packed, **kw) for packed in (1, 0)}
    for packed, out in outs.items():
        assert out["flagged"] == 0 and (out["quad_slot_bytes"] > 0)
        # every lane shape with LDS slots ran, the streamed ones included
        assert {c["geometry"] for c in out["plan"] if c["kernel"] == "quad"} >= {321001, 321002, 321003, 321004, 3320804, 4320804}
        slots.check_against(out, ref, heldout, "quad_packed=%d K=%d %s" % (packed, K, mode))
    for name, digest in cases.boundary_digests(outs[1], heldout).items():
        assert digest.encode() == bytes(recorded["boundary/%d/%s/%s" % (K, mode, name)]), (name, bytes(recorded["recorded_from"]))
        assert np.array_equal(outs[1][name], outs[0][name]), name

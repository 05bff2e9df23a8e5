"""The hand-over tile of the stride-256 quad kernels written in slot pairs (estep_quad.h quad_hand_over, estep_limits.h
quad_handover_pairs): 16-byte stores of two adjacent terms after a swap between the half-waves - the same bytes at the
same addresses as the 8-byte stores before, so everything an E-step gives stays bit for bit what it was.

One document of every length 161 .. 256 (both parities, every class boundary 176 / 192 / 208 / 224 / 240, last slots
filled by one word group only, the streamed classes), K = 256 and 129 (padding topics), hand-over counts 4, the default
and 56 (option compact_cap), on the training fast path and with per-document values, against what the commit before the
change gave on an MI355X (tests/golden/quad_handover_pairs.npz, recorded by
tests/golden/make_quad_handover_pairs_golden.py): SHA-256 of gamma, of the iteration counts and of the statistics, the
joint value, and the executed work (Context.executed_work).  At the default count and at 56 at least 80 of the 96
documents are handed over - with documents that stay dense the test would say nothing about the tile (at count 4 none
is on this corpus: its documents keep 7 - 25 topics alive, those four cases pin the dense path only).  The tile region
that lies last in the buffer is that of the 161 terms, an odd length; a second test hands it over at the count its live
topics meet exactly, so that its last column is in use - the place where a 16-byte store reaching past N would leave
the allocation.

There is no hook that reads the tile back: the live-topic kernel forms every normaliser from all live columns of a term,
so a wrong or missing tile element changes a normaliser and with it gamma's digest (shown once with a copy of the tree
that skipped one paired store: LABNOTES).  Gamma is also held against the C oracle at the suite's bars.
Needs an MI355X."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
import quad_handover_pairs_cases as cases

pytestmark = pytest.mark.gpu

GAMMA_RTOL_ORACLE, SSTATS_ATOL = 1e-7, 1e-8          # tests/test_gpu_quad_slots.py

_inputs, _reference = {}, {}


def inputs_of(K):
    if K not in _inputs:
        _inputs[K] = cases.corpus(K)
    return _inputs[K]


def reference_of(K):
    """The C oracle's E-step on the corpus of K: computed once, shared, never modified."""
    from oracle import c_oracle
    if K not in _reference:
        ptr, ids, cts, eta, alpha = inputs_of(K)
        ref = c_oracle.e_step(alpha, eta, ptr, ids, cts, max_iter=50)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _reference[K] = ref
    return _reference[K]


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    return _capi


@pytest.fixture(scope="module")
def recorded():
    return load_golden("quad_handover_pairs.npz")


@pytest.mark.parametrize("path", cases.PATHS)
@pytest.mark.parametrize("cap", cases.CAPS)
@pytest.mark.parametrize("K", cases.KS)
def test_paired_tile_stores_give_the_bits_of_the_single_stores(capi, recorded, K, cap, path):
    inputs = inputs_of(K)
    out = cases.run(capi, K, inputs, cap, path)
    what = "K=%d compact_cap=%d %s" % (K, cap, path)
    print(what, "handed over", out["work"][1], "tile entries", out["work"][0])
    assert out["flagged"] == 0, what
    if cap != 4:
        assert recorded[cases.key(K, cap, path, "work")][1] >= 80, what           # the condition of the corpus
    for field in ("gamma", "iters", "sstats"):
        assert cases.digest(out[field]).encode() == bytes(recorded[cases.key(K, cap, path, field)]), (what, field)
    assert np.array_equal(out["joint"], recorded[cases.key(K, cap, path, "joint")]), what
    assert np.array_equal(out["work"], recorded[cases.key(K, cap, path, "work")]), what
    ref = reference_of(K)
    assert np.array_equal(out["iters"], ref["iters"]), what
    assert rel_err(out["gamma"], ref["gamma"]) < GAMMA_RTOL_ORACLE, what
    assert np.max(np.abs(out["sstats"] - ref["sstats"])) < SSTATS_ATOL, what


def capacities(plan):
    """Terms a document of each launch class can have at most, in the order of the plan: 16 per word slot."""
    return [16 * (c["geometry"] % 10000 // 100 + c["geometry"] % 100 + c["geometry"] // 1000000) for c in plan if c["kernel"] == "quad"]


@pytest.mark.parametrize("K", cases.KS)
def test_the_last_tile_region_is_an_odd_length_handed_over_with_its_last_column_in_use(capi, recorded, K):
    """The one place where a 16-byte store reaching past N would leave the allocation: the last column of the tile
    region that lies last in the buffer.  That region is the 161-term document's - the schedule sorts by length, longest
    first, the launch classes follow it (checked on the plan: capacities strictly falling), and prepare_compact hands out
    the regions in that order.  Its live count per iteration is read off the dense kernels (cases.live_counts); with the
    first count that fits its 56 columns as option compact_cap the document has N x that many doubles, the count of the
    iteration before was larger, so it is handed over in that iteration with ALL its columns live: with the iteration
    cap at that iteration it finishes dense, with one more it is handed over.  At that count the whole corpus gives the
    parent's bits on both paths, and the document's own rows are those it gives alone."""
    inputs = inputs_of(K)
    ptr, alpha = inputs[0], inputs[4]
    lengths = np.diff(ptr)
    assert lengths[-1] == lengths.min() == 161 and np.all(np.diff(lengths) < 0)
    alone = cases.last_document(inputs)
    counts = cases.live_counts(capi, K, alone)
    cap = cases.cap_met_exactly(counts)
    at = counts.index(cap) + 1                                       # the inner iteration that ends with `cap` live topics
    print("K", K, "live topics per iteration", counts, "-> compact_cap", cap, "met at iteration", at)
    assert cap == int(recorded["last_cap/%d" % K]) and at >= 2 and counts[at - 2] > cap
    assert cases.run(capi, K, alone, cap, "values", max_iter=at)["work"][1] == 0
    assert cases.run(capi, K, alone, cap, "values", max_iter=at + 1)["work"][1] == 1
    single = cases.run(capi, K, alone, cap, "values")
    assert single["work"][1] == 1 and single["flagged"] == 0
    assert np.count_nonzero(single["gamma"][0] != alpha) <= cap
    for path in cases.PATHS:
        out = cases.run(capi, K, inputs, cap, path)
        what = "K=%d compact_cap=%d %s" % (K, cap, path)
        falling = capacities(out["plan"])
        assert all(a > b for a, b in zip(falling, falling[1:])) and falling[-1] == 176, out["plan"]
        assert sum(c["documents"] for c in out["plan"] if c["kernel"] == "quad") == cases.D
        assert out["flagged"] == 0 and out["work"][1] >= 1, what
        for field in ("gamma", "iters", "sstats"):
            assert cases.digest(out[field]).encode() == bytes(recorded[cases.key(K, cap, path, field)]), (what, field)
        assert np.array_equal(out["joint"], recorded[cases.key(K, cap, path, "joint")]), what
        assert np.array_equal(out["work"], recorded[cases.key(K, cap, path, "work")]), what
        assert np.array_equal(out["gamma"][-1], single["gamma"][0]) and out["iters"][-1] == single["iters"][0], what

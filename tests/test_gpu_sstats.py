"""The sufficient-statistics pass (pylda_amd/csrc/sstats_kernels.h, sstats_sweep.h, sstats_live.h, the planner behind
them in host_plan.cpp, sstats_gather.hip) on INJECTED inputs, exact to the last bit.  Needs an MI355X.

pylda_test_statistics runs the production pass - tables, postings, segment cut, rounds or sweep or lists, finalize,
entropy sum - on a given t, r and lists of live topics.  sstats[w][k] = B[w][k] * sum_d r_dw t'_d[k]: with the small
integers of tests/sstats_reference.py every partial sum is exact in fp64 in any order, so

    get_sstats() == (B_dev * s).T[:K]          bit for bit (array_equal),

with B_dev the expElog table as pylda_test_tables reads it back and s the int64 reference; the product is one fp64
multiply in numpy as on the device.  A posting that is lost, doubled, read from another document's row or credited to
another term changes an integer: nothing is too small to see.  Eta ~ gamma(100, 0.01), so every B[w][k] is distinct.

The entropy sum is compared with math.fsum(G_dev * s) over all V x stride entries (G_dev: expElog_elog as read back)
within n * 2^-53 * sum|G s|, n the longest chain of roundings a value passes through on the device (the terms of second
order, n 2^-54 of the bound, are covered by the exact first addition onto 0 that every chain below counts as a rounding):
  * finalize route (every gather kernel, the pass over the lists; sstats_finalize_kernel, then vector_sum3_kernel):
    the product G s is rounded on the device as in numpy - the same addends; block_sum<256> = wave_sum's 6 levels + 4
    additions of the wavefronts' sums; vector_sum3_kernel: ceil(E / 1024) additions per thread over the E = ceil(V
    stride / 256) partials, 6 levels, 16 additions.  n = 6 + 4 + ceil(E / 1024) + 6 + 16.
  * sweep (sstats_sweep_kernel): a lane's fma chain over its T terms x stride / 64 values (one rounding each; + 1 for the
    product numpy rounds and the fma does not), wave_sum's 6 levels, then vector_sum3_kernel over passes x wavefronts
    partials.  n = T stride / 64 + 1 + 6 + ceil(passes wavefronts / 1024) + 6 + 16.
Both are far below V x stride.

The real-valued cases (t in (0, 1), r in (0, 4), every addend positive) hold every statistic to
(postings of the term + its segments + 2) * 2^-53 relative to a correctly rounded sum times B: a posting costs one
rounding (an fma; in the pass over the lists a product and an addition, whose first per segment is onto 0 and exact; the
tree that joins a gather kernel's accumulators is never deeper than the segment has postings), joining the segments one
less than there are, B one, and the reference two (the sum's rounding, the multiply).

Runs share a context and a case, so an earlier run's statistics would be the right answer of the next: the entry fills
the statistics, the partial rows, the entropy partials and their sum with NaN before the pass, and every run - each
variant of positions, blocks, rounds, sub-steps and rendezvous - is held against the reference in full.  What a launch
leaves unwritten is a NaN in the result.

Every run prints the kernel family it reached, its geometry and the entropy error over its bound.
"""
import functools
import math

import numpy as np
import pytest

import sstats_reference as sr
from conftest import csr_slice

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SSTATS_ATOL = 1e-8        # the whole-E-step case: test_gpu_estep.py's bar against the oracle
BASE = {"gather_rows": 2, "gather_blocks": 0, "gather_sweep": 0, "gather_round_mb": 0, "wide_postings": 0, "gather_live": 0,
        "sweep_sub": 4, "sweep_xcd": 1}
LAYOUT = ("gather_blocks", "gather_segments", "gather_rounds", "gather_partial_rows", "gather_sweep_passes", "gather_sweep_terms",
          "gather_sweep_wpb", "gather_live")


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    _capi.load()
    assert _capi.device_count() >= 1, "no HIP device visible"
    return _capi


corpus_of = functools.lru_cache(maxsize=None)(sr.build_corpus)


@functools.lru_cache(maxsize=None)
def integer_case(V, K, mix=None):
    case = sr.integer_inputs(corpus_of(V), K, seed=V + K, mix=mix)
    return case, sr.reference_sums(corpus_of(V), case)


@functools.lru_cache(maxsize=None)
def real_case(V, K, mix=None):
    case = sr.real_inputs(corpus_of(V), K, seed=V + K, mix=mix)
    return case, sr.real_reference(corpus_of(V), case)


class Model(object):
    """A context whose eta is set, and its tables B = expElog and G = expElog_elog as the device holds them."""

    def __init__(self, capi, K, V):
        self.K, self.V = K, V
        self.ctx = capi.Context(K, V)
        self.ctx.set_eta(np.random.default_rng(1000 * K + V).gamma(100.0, 0.01, (K, V)))
        tables = self.ctx.test_tables(only=("expElog", "expElog_elog"))
        self.B, self.G = tables["expElog"], tables["expElog_elog"]
        self.ldk = self.B.shape[1]
        self.expected = {}
        assert self.ldk == sr.table_stride(K)
        if V <= 1000:       # every B distinct but the rows' maxima, which are exactly 1: a sum credited to another entry shows
            assert np.unique(self.B[:, :K]).size >= K * V - V - 8

    def run(self, case, **options):
        """The production pass on the case's inputs: (statistics (K, V), entropy sum, layout)."""
        corpus_host = corpus_of(self.V)
        opts = dict(BASE, **options)
        for name, value in opts.items():
            self.ctx.set_option(name, value)
        corpus = self.ctx.corpus(corpus_host.doc_ptr, corpus_host.term_id, corpus_host.term_ct)
        try:
            entropy = self.ctx.test_statistics(corpus, case["t"], case["r"], case["live_n"], case["live_topic"], case["live_t"])
            sstats = np.array(self.ctx.get_sstats())
            layout = {name: corpus.layout(name) for name in LAYOUT}
            layout["compute_units"] = self.ctx.compute_units()
        finally:
            corpus.close()
        layout["family"] = family(self.ldk, opts, layout)
        return sstats, entropy, layout

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def models(capi):
    """One model per (K, V) of the small vocabularies: eta drawn, uploaded and its tables read back once."""
    cache = {}

    def get(K, V):
        if (K, V) not in cache:
            cache[(K, V)] = Model(capi, K, V)
        return cache[(K, V)]
    yield get
    for model in cache.values():
        model.close()


@pytest.fixture(scope="module")
def compute_units(capi):
    ctx = capi.Context(2, 4)
    cus = ctx.compute_units()
    ctx.close()
    assert cus >= 8
    return cus


def family(ldk, opts, layout):
    """The kernel enqueue_sstats_gather launches for this layout (sstats_gather.hip)."""
    pos = "int64" if opts["wide_postings"] else "int32"
    if layout["gather_live"]:
        return "live<4, %s> lds %d" % (pos, 4 * ldk * 8)
    if layout["gather_sweep_passes"]:
        return "sweep<%d, %d, %d, %s> passes %d" % (ldk // 64, layout["gather_sweep_terms"], layout["gather_sweep_wpb"], pos,
                                                    layout["gather_sweep_passes"])
    if ldk in (16, 32):
        return "gather<%d, %s>" % (ldk, pos)
    if opts["gather_rows"] and ldk in (64, 128, 256):
        if opts["gather_rows"] == 2 and ldk != 64:
            return "bulk<%d, 4, %s>" % (ldk // 64, pos)
        return "rows<%d, %s>" % (ldk // 64, pos)
    return "gather<64, %s> grid.y %d" % (pos, (ldk + 63) // 64)


def finalize_chain(V, ldk):
    # (E does not depend on the rounds: a round starts on a multiple of 16 terms, so on a multiple of 256 statistics, and
    #  takes the blocks of 256 of the WHOLE table from there - plan_rounds' ent_first - so the rounds' blocks tile the
    #  ceil(V stride / 256) of the single round; the entry fills exactly that many partials with NaN beforehand)
    return 6 + 4 + ((V * ldk + 255) // 256 + 1023) // 1024 + 6 + 16


def sweep_chain(ldk, layout):
    waves = layout["compute_units"] * layout["gather_sweep_wpb"]
    return layout["gather_sweep_terms"] * (ldk // 64) + 1 + 6 + (layout["gather_sweep_passes"] * waves + 1023) // 1024 + 6 + 16


def check_exact(model, s, got, what):
    """Statistics bit for bit, the entropy sum within its derived bound; prints the family and the entropy figure."""
    sstats, entropy, layout = got
    K, V, ldk = model.K, model.V, model.ldk
    n = sweep_chain(ldk, layout) if layout["gather_sweep_passes"] else finalize_chain(V, ldk)
    assert n <= V * ldk
    if id(s) not in model.expected:         # once per case: every run of it is held against the same reference
        addends = model.G * s
        addends = addends[addends != 0.0]
        model.expected[id(s)] = (s, (model.B * s).T[:K], math.fsum(addends.tolist()), math.fsum(np.abs(addends).tolist()))
    _, want, want_entropy, scale = model.expected[id(s)]
    bound = n * U * scale
    print("sstats %-28s K %4d V %5d %-44s blocks %2d segments %6d rounds %d | entropy chain %3d error / bound %.4f"
          % (what, K, V, layout["family"], layout["gather_blocks"], layout["gather_segments"], layout["gather_rounds"], n,
             abs(entropy - want_entropy) / bound))
    differ = np.argwhere(sstats != want)
    assert differ.size == 0, "%s (%s): %d statistics differ, first: topic %d of term %d (%d postings) is %r, expected %r" % (
        what, layout["family"], len(differ), differ[0][0], differ[0][1], corpus_of(V).postings[differ[0][1]],
        sstats[tuple(differ[0])], want[tuple(differ[0])])
    assert np.array_equal(sstats, want)
    for v in sr.empty_terms(V):
        assert not sstats[:, v].any()
    assert abs(entropy - want_entropy) <= bound, (what, entropy, want_entropy, bound)


# ---- plain gather: no document blocks ------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,rows,wide", [
    (10, 2, 0), (10, 2, 1), (20, 2, 0), (20, 2, 1), (50, 0, 0), (50, 0, 1), (50, 1, 0), (50, 1, 1),
    (100, 0, 0), (100, 1, 0), (100, 1, 1), (100, 2, 0), (100, 2, 1), (130, 0, 0), (130, 1, 0), (130, 1, 1), (130, 2, 0), (130, 2, 1)])
def test_plain_gather(models, K, rows, wide):
    """Strides 16, 32 (sstats_gather_kernel's 4 x 64 / LR unroll and tail), 64, 128, 256 by 64-topic chunks, whole rows
    (the pair loop and its odd tail) and postings in bulk (chunks of 63, 64, 65; trips that run past n % 4 != 0); the
    plain cut at 256 postings."""
    model = models(K, 700)
    case, s = integer_case(700, K)
    got = model.run(case, gather_rows=rows, wide_postings=wide)
    layout = got[2]
    want_family = {16: "gather<16", 32: "gather<32"}.get(model.ldk) or (
        "gather<64" if rows == 0 else "bulk<%d" % (model.ldk // 64) if rows == 2 and model.ldk > 64 else "rows<%d" % (model.ldk // 64))
    assert layout["family"].startswith(want_family) and ("int64" in layout["family"]) == bool(wide)
    assert layout["gather_blocks"] == 1 and layout["gather_rounds"] == 1 and not layout["gather_live"] and not layout["gather_sweep_passes"]
    assert layout["gather_segments"] == corpus_of(700).segments().sum() == layout["gather_partial_rows"]
    check_exact(model, s, got, "plain rows=%d" % rows)


@pytest.mark.parametrize("K,stride,wide", [(300, 384, 0), (300, 384, 1), (1025, 1088, 0)])
def test_plain_gather_generic_strides(models, K, stride, wide):
    """Strides the row kernels are not built for: 64-topic chunks, grid.y = stride / 64 (17 at stride 1088, beyond the
    1024 mark where the stride is a multiple of 64, not of 128)."""
    model = models(K, 300)
    assert model.ldk == stride
    case, s = integer_case(300, K)
    got = model.run(case, wide_postings=wide)
    assert got[2]["family"].startswith("gather<64") and got[2]["family"].endswith("grid.y %d" % (stride // 64))
    check_exact(model, s, got, "plain generic")


# ---- document blocks, paced by the dispatch order -------------------------------------------------------------------------

@pytest.mark.parametrize("K", [50, 100, 130])
@pytest.mark.parametrize("blocks", [8, 24, 40])
def test_blocked_gather(models, K, blocks):
    """Segments cut at the boundaries of 8, 24 and 40 document blocks of 643 documents (at 40 the last two hold none)
    and run in XCD order through exec_order (-1 slots, blocks that start on multiples of 4 slots): whole rows and bulk."""
    model = models(K, 700)
    case, s = integer_case(700, K)
    for rows in (1, 2):
        got = model.run(case, gather_rows=rows, gather_blocks=blocks)
        layout = got[2]
        assert layout["gather_blocks"] == blocks and layout["gather_rounds"] == 1 and not layout["gather_sweep_passes"]
        assert layout["gather_segments"] == corpus_of(700).segments(blocks, 256).sum()
        assert layout["family"].startswith("bulk" if rows == 2 and model.ldk > 64 else "rows")
        check_exact(model, s, got, "blocked rows=%d" % rows)


def test_blocked_gather_in_rounds(capi):
    """A 1 MiB budget of partial rows (512 rows at stride 256) at V = 20000: several rounds over term ranges that start on
    multiples of 16 terms and share the rows; exact, and bitwise the single round."""
    K, V = 130, 20000
    model = Model(capi, K, V)
    try:
        case, s = integer_case(V, K)
        single = model.run(case, gather_blocks=24)
        rounds = model.run(case, gather_blocks=24, gather_round_mb=1)
        assert single[2]["gather_rounds"] == 1 and single[2]["gather_partial_rows"] == single[2]["gather_segments"]
        assert rounds[2]["gather_rounds"] >= 3 and rounds[2]["gather_partial_rows"] < single[2]["gather_partial_rows"]
        check_exact(model, s, single, "blocked, one round")
        check_exact(model, s, rounds, "blocked, %d rounds" % rounds[2]["gather_rounds"])
        assert np.array_equal(single[0], rounds[0])
    finally:
        model.close()


# ---- the persistent sweep ------------------------------------------------------------------------------------------------

def sweep_geometry(ldk, V, cus):
    """host_plan.cpp sweep_geometry: (terms per wavefront, wavefronts per workgroup, passes)."""
    passes = lambda T, wpb: (V + cus * wpb * T - 1) // (cus * wpb * T)
    if ldk == 128:
        return (12, 16, 1) if passes(12, 16) == 1 else (16, 16, passes(16, 16))
    a, b = passes(8, 16), passes(12, 12)
    return (12, 12, b) if b < a else (8, 16, a)


# (K, terms per compute unit, one more?, the geometry that vocabulary reaches): on 256 compute units the vocabularies are
# 49152, 49153, 65537 at stride 128 and 32768, 32769, 36865, 65537 at stride 256
SWEEP_CASES = [
    (100, 16 * 12, 0, (12, 16, 1)),      # every slot of every wavefront holds a term
    (100, 16 * 12, 1, (16, 16, 1)),
    (100, 16 * 16, 1, (16, 16, 2)),      # the second pass holds one term
    (130, 16 * 8, 0, (8, 16, 1)),
    (130, 16 * 8, 1, (12, 12, 1)),
    (130, 12 * 12, 1, (8, 16, 2)),
    (130, 16 * 16, 1, (12, 12, 2)),
]


@pytest.mark.parametrize("K,per_cu,more,geometry", SWEEP_CASES)
def test_sweep(capi, compute_units, K, per_cu, more, geometry):
    """Every slot of a wavefront's T terms (the groups of four, both halves of a group), one and two passes (the pass
    offset into term_of and the entropy partials, the rendezvous across passes), all four kernels of the dispatch; 8
    blocks (81 postings of one term in a block: the loop behind the batch) and 40 (blocks without documents); the sub-steps
    of a block and both rendezvous."""
    V = compute_units * per_cu + more
    ldk = sr.table_stride(K)
    assert sweep_geometry(ldk, V, compute_units) == geometry
    model = Model(capi, K, V)
    try:
        case, s = integer_case(V, K)
        runs = [dict(gather_blocks=nb, sweep_sub=sub, sweep_xcd=xcd) for nb in (8, 40) for sub in (1, 7) for xcd in (0, 1)]
        if geometry[2] == 2:
            runs.append(dict(gather_blocks=8, wide_postings=1))
        first = None
        for options in runs:
            what = "sweep " + " ".join("%s=%d" % kv for kv in sorted(options.items()))
            got = model.run(case, gather_sweep=2, **options)
            layout = got[2]
            assert (layout["gather_sweep_terms"], layout["gather_sweep_wpb"], layout["gather_sweep_passes"]) == geometry, layout
            assert layout["gather_blocks"] == options["gather_blocks"] and layout["gather_partial_rows"] == 0
            assert layout["gather_segments"] == corpus_of(V).segments(options["gather_blocks"], 64).sum()
            check_exact(model, s, got, what)
            if first is None:
                first = got
            else:       # (the entropy sum keeps its order: the same bits whatever the blocks, the pacing, the positions)
                assert got[1] == first[1], options
    finally:
        model.close()
        integer_case.cache_clear()
        corpus_of.cache_clear()


# ---- the pass over the lists of live topics ---------------------------------------------------------------------------------

@pytest.mark.parametrize("K,wide", [(10, 0), (50, 0), (100, 0), (256, 0), (256, 1), (300, 0), (2000, 0)])
def test_live_lists(models, K, wide):
    """All documents listed, none, every third without a list (mixed and uniform chunks in one segment); lists of 1, 11,
    12, 13, 24, 25, 59 and 60 entries, topics 0 and K - 1 among them; the dense rows of listed documents are NaN.  Stride
    2048 asks for exactly 64 KiB of LDS."""
    model = models(K, 700)
    for mix in sr.MIXES:
        case, s = integer_case(700, K, mix)
        got = model.run(case, gather_live=1, wide_postings=wide)
        layout = got[2]
        assert layout["gather_live"] == 1 and layout["gather_blocks"] == 1 and layout["family"].startswith("live")
        assert layout["gather_segments"] == corpus_of(700).segments().sum()
        check_exact(model, s, got, "lists: " + mix)
    integer_case.cache_clear()


def test_live_lists_beyond_the_lds_limit(models, capi):
    """Stride 2112 (K = 2049): four rows no longer fit 64 KiB, the corpus reports gather_live = 0 and the row route is exact;
    a listed document is then refused, not silently read as a row."""
    K = 2049
    model = models(K, 700)
    case, s = integer_case(700, K, "none")
    got = model.run(case, gather_live=1)
    assert got[2]["gather_live"] == 0 and got[2]["family"].startswith("gather<64") and model.ldk == 2112
    check_exact(model, s, got, "lists: beyond LDS")
    listed, _ = integer_case(700, K, "third")
    with pytest.raises(capi.PyldaError) as e:
        model.run(listed, gather_live=1)
    assert e.value.status == -4 and "gather_live" in str(e.value)
    integer_case.cache_clear()


# ---- real values: one case per route --------------------------------------------------------------------------------------

@pytest.mark.parametrize("route,K,options,cut,mix", [
    ("plain rows", 33, dict(gather_rows=1), (1, 256), None),
    ("plain chunks", 20, dict(), (1, 256), None),
    ("bulk", 65, dict(gather_rows=2), (1, 256), None),
    ("blocked", 65, dict(gather_rows=2, gather_blocks=24), (24, 256), None),
    ("sweep", 65, dict(gather_sweep=2, gather_blocks=8), (8, 64), None),
    ("lists", 65, dict(gather_live=1), (1, 256), "third"),
])
def test_real_values(models, route, K, options, cut, mix):
    model = models(K, 700)
    corpus = corpus_of(700)
    case, sums = real_case(700, K, mix)
    sstats, entropy, layout = model.run(case, **options)
    assert layout["gather_segments"] == corpus.segments(*cut).sum()
    assert bool(layout["gather_live"]) == (route == "lists") and bool(layout["gather_sweep_passes"]) == (route == "sweep")
    want = (model.B * sums).T[:K]
    n = (corpus.postings + corpus.segments(*cut) + 2).astype(np.float64)
    error = np.abs(sstats - want)
    bound = n[None, :] * U * want
    worst = np.max(np.divide(error, bound, out=np.zeros_like(error), where=bound > 0))
    print("sstats real values, %-12s K %3d %-40s worst error / bound %.4f" % (route, K, layout["family"], worst))
    assert np.all(np.isfinite(sstats)) and np.all(error <= bound)
    assert not sstats[:, list(sr.empty_terms(700))].any()


# ---- a whole E-step: what injected inputs cannot cover -----------------------------------------------------------------------

@pytest.mark.parametrize("options", [dict(gather_rows=2, gather_sweep=0), dict(gather_sweep=2)], ids=["bulk", "sweep"])
def test_whole_estep_with_empty_first_and_last_document(capi, ap_train, options):
    """Document 0 (and the last one) empty: the bulk and sweep kernels read row 0 of t with factor 0 for the lanes past a
    chunk, so whatever the dense kernels leave in an empty document's row must be finite (they write it)."""
    from oracle import c_oracle
    g = ap_train
    K, V = 128, 6806
    ptr, tid, tct = csr_slice(g["doc_ptr"], g["term_id"], g["term_ct"], range(300))
    ptr = np.concatenate(([0], ptr, [ptr[-1]]))
    assert ptr[1] == 0 and ptr[-1] == ptr[-2] and ptr.size == 303
    rng = np.random.default_rng(128)
    eta, alpha = rng.gamma(100.0, 0.01, (K, V)), rng.uniform(0.05, 1.0, K)
    ctx = capi.Context(K, V)
    for name, value in dict(gather_live=0, gather_blocks=8, **options).items():
        ctx.set_option(name, value)
    corpus = ctx.corpus(ptr, tid, tct)
    out = ctx.estep_host(corpus, alpha, eta)
    assert corpus.layout("gather_blocks") == 8 and (corpus.layout("gather_sweep_passes") >= 1) == (options["gather_sweep"] == 2)
    corpus.close()
    ctx.close()
    ref = c_oracle.e_step(alpha, eta, ptr, tid, tct)
    worst = np.max(np.abs(out["sstats"] - ref["sstats"]))
    print("sstats whole E-step, documents 0 and %d empty: largest difference from the oracle %.3g" % (ptr.size - 2, worst))
    assert np.all(np.isfinite(out["sstats"])) and worst < SSTATS_ATOL
    assert np.array_equal(out["iters"], ref["iters"]) and out["iters"][0] == 1 and out["iters"][-1] == 1

"""The E-step's safety net where documents really reach it: the `bad` exit of the dense kernels (status 1, rfinal / tfinal
zeroed), estep_logspace_kernel finding and redoing the flagged documents, their statistics added behind the gather - through
the C ABI, against the C oracle and the mpmath golden.  The cases and the prediction of which documents a dense kernel flags
are tests/safety_net_cases.py; tests/test_safety_net_host.py checks them on the CPU.  Needs an MI355X.

Bars (tests/test_gpu_estep.py): the oracle's inner-iteration count on EVERY document, gamma 1e-9 relative,
per-document likelihood 1e-9 relative + 1e-11, statistics 1e-8 absolute, corpus likelihood of the fast path 1e-11 relative."""
import functools

import numpy as np
import pytest

import safety_net_cases as sc
from conftest import load_golden

pytestmark = pytest.mark.gpu

GAMMA_RTOL, LL_RTOL, LL_ATOL, SSTATS_ATOL, FAST_RTOL = 1e-9, 1e-9, 1e-11, 1e-8, 1e-11


def EMPTY_DOC_FLOOR(alpha):
    """The likelihood of an empty document is analytically 0: lnG(sum alpha) - sum lnG(alpha_k), summed term after term on
    the host, against the same terms of gamma = alpha summed as a tree on the device.  Nothing relative is left to compare,
    and the two sums cancel at M = sum |lnG(alpha_k)| - 9431 at K = 1024, alpha = 1e-4, 26970 at K = 3325, alpha = 3e-4 -
    where all K terms are equal and their rounding errors add up instead of averaging out.  Two bounds of the formats, none
    measured: recursive summation of K terms errs by up to (K - 1) 2^-53 M, and the device's lnG is pinned to 5e-14 relative
    (tests/special_bounds.py LGAMMA_SCALED).  The floor of this one document is the suite's 1e-11 plus their sum, 1.5e-9 and
    1.1e-8 in the two cases above and 6e-11 at K = 1024, alpha ~ 1; every other document keeps 1e-11."""
    from scipy.special import gammaln
    return (5e-14 + (alpha.size - 1) * 2.0 ** -53) * float(np.sum(np.abs(gammaln(alpha))))


@pytest.fixture(scope="module")
def capi():
    from pylda_amd import _capi
    _capi.load()
    assert _capi.device_count() >= 1, "no HIP device visible"
    return _capi


_CASES = {"branch": sc.branch_case, "natural": sc.natural_case, "chunk": lambda _: sc.chunk_case(),
          "boundary": sc.boundary_case, "guard": functools.lru_cache(maxsize=None)(sc.guard_case), "mp": sc.mp_inputs}


@functools.lru_cache(maxsize=None)
def oracle(kind, key, max_iter=50, tol=1e-6, heldout=False):
    """The C oracle on a case, computed once and shared (nobody writes into it)."""
    from oracle import c_oracle
    alpha, eta, ptr, ids, cts = _CASES[kind](key)
    return c_oracle.e_step(alpha, eta, ptr, ids, cts, max_iter=max_iter, tol=tol, heldout=heldout)


def estep(capi, case, max_iter=50, tol=1e-6, heldout=False, options=()):
    alpha, eta, ptr, ids, cts = case
    K, V = eta.shape
    ctx = capi.Context(K, V)
    for name, value in options:
        ctx.set_option(name, value)
    corpus = ctx.corpus(ptr, ids, cts)
    out = ctx.estep_host(corpus, alpha, eta, max_iter, tol, heldout)
    out["logspace_docs"] = ctx.estep_results(corpus)[2]
    corpus.close()
    ctx.close()
    return out


def check(out, ref, case, heldout, what="", exact_reference=False):
    """Every document against the reference: no document is left out of a comparison."""
    alpha, eta, ptr, ids, cts = case
    assert np.array_equal(out["iters"], ref["iters"]), (what, np.nonzero(out["iters"] != ref["iters"])[0], out["iters"], ref["iters"])
    gamma_err = np.max(np.abs(out["gamma"] - ref["gamma"]) / np.abs(ref["gamma"])) if ref["gamma"].size else 0.0
    key = "doc_words_ll" if heldout else "doc_ll"
    ll_err = np.abs(out[key] - ref[key]) - LL_RTOL * np.abs(ref[key])
    floor = np.full(len(ptr) - 1, LL_ATOL)
    empty = np.nonzero(np.diff(ptr) == 0)[0]
    if not heldout:
        floor[empty] += EMPTY_DOC_FLOOR(alpha)
    print("%s gamma %.2e  %s over the relative bar by %.2e" % (what, gamma_err, key, ll_err.max() if ll_err.size else 0.0), end="")
    assert np.all(np.isfinite(out["gamma"])) and gamma_err < GAMMA_RTOL, (what, gamma_err)
    assert np.all(ll_err <= floor), (what, ll_err.max())
    for d in empty:                                             # gamma = alpha after one iteration (its likelihood: the floor above)
        assert out["iters"][d] == 1 and np.array_equal(out["gamma"][d], alpha)
    if heldout:
        assert out["sstats"] is None
        print()
        return
    sstats_err = np.abs(out["sstats"] - ref["sstats"])
    # 1e-8; against an fp64 oracle the column of the word with the count of 10^6 gets the oracles' own gap on top (see there)
    bar = SSTATS_ATOL if exact_reference else sc.statistics_bar(eta.shape[1], ids, cts)
    print("  statistics %.2e, worst error / bar %.3f" % (sstats_err.max(), np.max(sstats_err / bar)))
    assert np.all(sstats_err < bar), (what, sstats_err.max())
    assert abs(out["sstats"].sum() - cts.sum()) < 1e-7 * max(1, cts.sum())              # tokens conserved


def fast_path_agrees(capi, case, options=(), max_iter=50, tol=1e-6):
    """doc_values = 0 (what learning() runs: `sc[0] -= sc[2]`, doc_terms_kernel skipping the flagged documents) gives the
    corpus likelihood of doc_values = 1, the same statistics to the order of the net's atomics and the same count."""
    alpha, eta, ptr, ids, cts = case
    ctx = capi.Context(*eta.shape)
    for name, value in options:
        ctx.set_option(name, value)
    corpus = ctx.corpus(ptr, ids, cts)
    full = ctx.estep_host(corpus, alpha, eta, max_iter, tol)
    flagged = ctx.estep_results(corpus)[2]
    ctx.set_option("doc_values", 0)
    ctx.estep(corpus, max_iter, tol)
    fast_ll, _, fast_flagged = ctx.estep_results(corpus)
    fast_sstats = ctx.get_sstats()
    fast_gamma = ctx.get_gamma(corpus)
    corpus.close()
    ctx.close()
    assert fast_flagged == flagged
    assert abs(fast_ll - full["document_log_likelihood"]) <= FAST_RTOL * abs(full["document_log_likelihood"])
    assert abs(full["doc_ll"].sum() - full["document_log_likelihood"]) <= FAST_RTOL * abs(full["document_log_likelihood"])
    # (the net's atomics are unordered: an entry may round differently, by an ulp of its own size)
    assert np.all(np.abs(fast_sstats - full["sstats"]) <= 1e-11 * np.maximum(1.0, full["sstats"]))
    assert np.max(np.abs(fast_gamma - full["gamma"]) / full["gamma"]) < 1e-12
    return flagged


# ---- 1. the log-space kernel at its own branch points ----
@pytest.mark.parametrize("setting", range(len(sc.SETTINGS)))
@pytest.mark.parametrize("K", sc.BRANCH_K)
def test_logspace_kernel_at_its_strides(capi, K, setting):
    """force_logspace: every document through estep_logspace_kernel.  K around the lane stride (64) and the thread stride
    (256) and beyond both; documents around the wavefront stride (4 words) and the thread stride (256 terms), an empty one, a
    count of 10^6; an iteration cap of 1 (the final pass reuses psi of the start gamma), 2, early stops, threshold 0."""
    max_iter, tol = sc.SETTINGS[setting]
    case = sc.branch_case(K)
    D = len(case[2]) - 1
    for heldout in (False, True):
        out = estep(capi, case, max_iter, tol, heldout, [("force_logspace", 1)])
        assert out["logspace_docs"] == D
        check(out, oracle("branch", K, max_iter, tol, heldout), case, heldout, "K=%d %s heldout=%d:" % (K, sc.SETTINGS[setting], heldout))
    assert fast_path_agrees(capi, case, [("force_logspace", 1)], max_iter, tol) == D         # doc_values = 0 against 1


@pytest.mark.parametrize("max_iter", sc.MP_MAX_ITER)
@pytest.mark.parametrize("name", [c[0] for c in sc.MP_CASES])
def test_logspace_kernel_against_mpmath(capi, name, max_iter):
    """The same bars against the reference's E-step in mpmath at 50 digits (tests/golden/make_logspace_mp.py): K = 1024 at
    alpha = 1e-4 is the regime the net exists for, psi(gamma) ~ -1e3 .. -1e4.  At K = 1024 the documents also run without the
    hook: estep_qfusek flags the one of one token itself."""
    g = load_golden("logspace_mp.npz")
    case = sc.mp_inputs(name)
    ref = {key: g["%s_m%d_%s" % (name, max_iter, key)] for key in ("gamma", "doc_ll", "words_ll", "sstats", "iters")}
    ref["doc_words_ll"] = ref["words_ll"]
    D = len(case[2]) - 1
    for options in ([("force_logspace", 1)], []) if name == "K1024" else ([("force_logspace", 1)],):
        for heldout in (False, True):
            out = estep(capi, case, max_iter, 1e-6, heldout, options)
            assert out["logspace_docs"] == (D if options else 1)          # (the document of one token: test_safety_net_host.py)
            check(out, ref, case, heldout, "%s max_iter=%d heldout=%d %s:" % (name, max_iter, heldout, options), exact_reference=True)


# ---- 2. documents the dense kernels flag themselves ----
@pytest.mark.parametrize("setting", range(len(sc.SETTINGS)))
@pytest.mark.parametrize("name", list(sc.NATURAL))
def test_dense_kernels_flag_the_predicted_documents(capi, name, setting):
    """alpha collapsed to 1e-4 / 3e-4 at K = 1024 (estep_qfusek), 2000 and 3325, the largest K (the generic kernels): the
    documents whose normaliser leaves the fp64 range - predicted by the numpy emulation, with a margin of 1e20 either side of the kernels'
    threshold - are flagged and redone, the others finished by the dense kernel; both kinds share words, so the zeroed rows
    pass through the gather and the net adds behind it.  The ABI exposes no per-document status: the count, and parity of
    every document."""
    max_iter, tol = sc.SETTINGS[setting]
    case = sc.natural_case(name)
    predicted = sc.natural_flagged(name, max_iter, tol)
    for heldout in (False, True):
        out = estep(capi, case, max_iter, tol, heldout)
        print("%s %s: %d flagged, predicted %s" % (name, sc.SETTINGS[setting], out["logspace_docs"], predicted.tolist()))
        assert out["logspace_docs"] == len(predicted)
        check(out, oracle("natural", name, max_iter, tol, heldout), case, heldout, "%s %s heldout=%d:" % (name, sc.SETTINGS[setting], heldout))


@pytest.mark.parametrize("name", list(sc.NATURAL))
def test_flagged_documents_through_every_statistics_pass(capi, name):
    """The zeroed rows of the flagged documents through the blocked gather, the rounds, the sweep and the 64-bit postings,
    the net's atomics behind each; two runs agree to 1e-11 (the atomics are unordered: not bit for bit); the fast path."""
    case = sc.natural_case(name)
    alpha, eta, ptr, ids, cts = case
    predicted = sc.natural_flagged(name)
    assert 0 < len(predicted) < len(ptr) - 1
    ctx = capi.Context(*eta.shape)
    corpus = ctx.corpus(ptr, ids, cts)
    kernels = {c["kernel"] for c in corpus.plan()}
    corpus.close()
    ctx.close()
    assert kernels and kernels <= sc.NATURAL[name][3], kernels
    ref = oracle("natural", name)
    first = None
    for options in ([], [("gather_blocks", 0)], [("gather_blocks", 8)], [("gather_blocks", 8), ("gather_sweep", 2)],
                    [("gather_blocks", 8), ("gather_sweep", 0), ("gather_round_mb", 1)], [("wide_postings", 1)], []):
        out = estep(capi, case, options=options)
        assert out["logspace_docs"] == len(predicted), options
        check(out, ref, case, False, "%s %s:" % (name, options))
        if first is None:
            first = out
        assert np.max(np.abs(out["sstats"] - first["sstats"])) < 1e-11
        assert np.max(np.abs(out["gamma"] - first["gamma"]) / first["gamma"]) < 1e-11
        assert np.all(np.abs(out["doc_ll"] - first["doc_ll"]) <= 1e-11 * np.abs(first["doc_ll"]))
    assert fast_path_agrees(capi, case) == len(predicted)


def test_more_than_one_document_per_workgroup_of_the_net(capi):
    """2100 documents - more than four workgroups on each of 256 CUs - so that estep_logspace_kernel collects several
    documents per chunk: one token (flagged) and ten tokens (not) in turn, K = 1024."""
    case = sc.chunk_case()
    for heldout in (False, True):
        out = estep(capi, case, heldout=heldout)
        assert out["logspace_docs"] == sc.CHUNK_D // 2
        check(out, oracle("chunk", None, 50, 1e-6, heldout), case, heldout, "chunk heldout=%d:" % heldout)


# ---- 3. state between E-steps on one corpus and context ----
def test_flags_and_counters_between_e_steps_on_one_corpus(capi):
    """status / live_n are reset between E-steps: alpha = 1e-4 (set F flagged) -> 0.1 (nothing) -> held-out at 1e-4 (F again,
    statistics untouched) -> training at 1e-4; each against the oracle, and the profiling counter of inner iterations equal
    to the sum of the iteration counts of the same E-step (a flagged document's count is written by the net)."""
    from oracle import c_oracle
    name = "K1024_a1e-4"
    alpha, eta, ptr, ids, cts = case = sc.natural_case(name)
    F = len(sc.natural_flagged(name))
    collapsed, grown = alpha, np.full(alpha.size, 0.1)
    assert not sc.predict_flagged(grown, eta, ptr, ids, cts)[1].any()
    ctx = capi.Context(*eta.shape)
    corpus = ctx.corpus(ptr, ids, cts)
    ctx.set_profiling(True)
    ctx.work_counters()
    kept = None
    for a, heldout, flagged in ((collapsed, False, F), (grown, False, 0), (collapsed, True, F), (collapsed, False, F)):
        ref = oracle("natural", name, 50, 1e-6, heldout) if a is collapsed else c_oracle.e_step(a, eta, ptr, ids, cts)
        out = ctx.estep_host(corpus, a, eta, 50, 1e-6, heldout)
        counted = ctx.work_counters()[0]
        assert ctx.estep_results(corpus)[2] == flagged
        check(out, ref, (a, eta, ptr, ids, cts), heldout, "alpha=%g heldout=%d:" % (a[0], heldout))
        print("inner iterations counted %d, sum of the documents' %d (oracle %d)" % (counted, out["iters"].sum(), ref["iters"].sum()))
        assert counted == out["iters"].sum()
        if heldout:
            assert np.array_equal(ctx.get_sstats(), kept)
        else:
            kept = out["sstats"]
    corpus.close()
    ctx.close()


# ---- 4. the live-topic guard's route into the net ----
@pytest.mark.parametrize("gather_live", (0, 1))
@pytest.mark.parametrize("K", (128, 256, 400))
def test_guard_failures_behind_every_hand_over_kernel(capi, K, gather_live):
    """compact_guard_fail: every document the live-topic kernel takes over fails its exactness guard and is redone by the
    log-space kernel - behind the quad kernel at table strides 128 and 256 and behind the fused streaming kernel (K = 400),
    with the statistics from live lists and from rows, training with and without per-document values, held-out."""
    alpha, eta, ptr, ids, cts = case = _CASES["guard"](K)
    for heldout in (False, True):
        ctx = capi.Context(K, eta.shape[1])
        ctx.set_option("compact_guard_fail", 1)
        ctx.set_option("gather_live", gather_live)
        corpus = ctx.corpus(ptr, ids, cts)
        ctx.set_profiling(True)
        ctx.work_counters()
        out = ctx.estep_host(corpus, alpha, eta, 50, 1e-6, heldout)
        counted = ctx.work_counters()[0]
        handed, flagged = ctx.executed_work()[1], ctx.estep_results(corpus)[2]
        print("K=%d gather_live=%d heldout=%d: handed over %d, flagged %d of %d" % (K, gather_live, heldout, handed, flagged, len(ptr) - 1))
        assert flagged == handed > 0
        assert counted == out["iters"].sum()
        check(out, oracle("guard", K, 50, 1e-6, heldout), case, heldout, "K=%d:" % K)
        if not heldout:
            ctx.set_option("doc_values", 0)
            ctx.estep(corpus)
            fast_ll, _, fast_flagged = ctx.estep_results(corpus)
            assert fast_flagged == flagged
            assert abs(fast_ll - out["document_log_likelihood"]) <= FAST_RTOL * abs(out["document_log_likelihood"])
            assert np.max(np.abs(ctx.get_sstats() - out["sstats"])) < 1e-11
        corpus.close()
        ctx.close()


# ---- 5. the LDS boundary ----
def test_largest_k_runs_and_the_next_is_refused(capi):
    """estep_logspace_kernel is launched in every E-step with its K-sized arrays and its list of flagged documents: the
    creation of a corpus refuses exactly the K whose launch would not fit the 160 KiB less the margin the runtime wants - no
    K is accepted there and then fails in every E-step (3390 .. 3411 were, before the two went by one function)."""
    K = sc.LARGEST_K
    assert sc.logspace_launch_bytes(K) + sc.LDS_MARGIN <= sc.LDS_BYTES < sc.logspace_launch_bytes(K + 1) + sc.LDS_MARGIN
    case = sc.boundary_case(K)
    for heldout in (False, True):
        out = estep(capi, case, heldout=heldout)
        assert out["logspace_docs"] == 4
        check(out, oracle("boundary", K, 50, 1e-6, heldout), case, heldout, "K=%d heldout=%d:" % (K, heldout))
    one = (np.array([0, 1]), np.array([1], np.int32), np.array([2], np.int32))
    for k in (K - 5, K - 1, K, K + 1, 3380, 3389, 3390, 3400, 3411, 3412):
        ctx = capi.Context(k, 4)
        if k <= K:
            corpus = ctx.corpus(*one)
            ctx.set_alpha(np.full(k, 0.1))
            ctx.set_eta(np.ones((k, 4)))
            ctx.estep(corpus)                                   # (raises where a launch fails)
            ll, _, flagged = ctx.estep_results(corpus)
            assert np.isfinite(ll) and flagged == 0 and abs(ctx.get_sstats().sum() - 2.0) < 1e-9
            corpus.close()
        else:
            with pytest.raises(capi.PyldaError) as e:
                ctx.corpus(*one)
            assert e.value.status == -1 and "LDS" in str(e.value), k
        ctx.close()

"""Packed launch slots of the quad kernel (estep_quad.h, estep_limits.h QuadSlot): the prologue that addresses its
document from blockIdx.x alone, reads the token total and sum alpha as scalars and forms the first t while the row gather
is in flight must give what the chain through order / doc_ptr / term_id gives - bit for bit - and what the oracle gives.

Documents with distinct-term counts exactly at every slot boundary of the quad classes (register, LDS and streamed
slots; one term, a full first slot, one over), every length four times and shuffled, counts above 1, a non-uniform alpha
(the order of summation of sum alpha matters) with three topics at 0.05 (the sign-bit path of alpha_sgn); K = 65 / 128
(table stride 128, classes that keep the old addressing) and 129 / 256 (stride 256, packed; padding topics at 65 / 129).
Bars: the suite's (tests/test_gpu_live_topics.py).  The GPU tests need an MI355X; the oracle cross-check runs anywhere."""
import numpy as np
import pytest

from conftest import rel_err

GAMMA_RTOL_ORACLE, LL_RTOL, SSTATS_ATOL = 1e-7, 1e-9, 1e-8
LENGTHS = [1, 15, 16, 17, 159, 160, 161, 175, 176, 177, 191, 192, 193, 207, 208, 209, 223, 224, 225, 239, 240, 241, 255, 256]
KS = [65, 128, 129, 256]
V, D = 2000, 96
MODES = {"hand-over": dict(options=()), "compact=0": dict(options=(("compact", 0),)), "held-out": dict(options=(), heldout=True),
         "max_iter=1": dict(options=(), max_iter=1)}


def boundary_corpus(K):
    """96 documents: every length of LENGTHS four times, shuffled; words drawn from a few topics each (most topics of a
    document die, so the hand-over happens), counts 2 .. 6; eta knows the topics."""
    rng = np.random.default_rng(7000 + K)
    true_topics = 24
    beta = rng.dirichlet(np.full(V, 0.02), size=true_topics)
    lengths = rng.permutation(np.repeat(LENGTHS, D // len(LENGTHS)))
    ptr, ids, cts = [0], [], []
    for n in lengths:
        theta = rng.dirichlet(np.full(true_topics, 0.1))
        p = 0.9 * (theta @ beta) + 0.1 / V
        u = np.sort(rng.choice(V, size=int(n), replace=False, p=p / p.sum()))
        ids.append(u.astype(np.int32))
        cts.append(rng.integers(2, 7, size=int(n)).astype(np.int32))
        ptr.append(ptr[-1] + int(n))
    eta = rng.gamma(100.0, 0.01, (K, V))
    for k in range(K):
        eta[k] += 40.0 * V * beta[k % true_topics] * rng.uniform(0.2, 1.0)
    alpha = rng.uniform(0.5, 1.5, K) / K
    alpha[rng.choice(K, size=3, replace=False)] = 0.05
    return np.array(ptr, np.int64), np.concatenate(ids), np.concatenate(cts), eta, alpha


_cache = {}


def inputs_and_reference(K, mode):
    """The corpus of K and the C oracle's E-step on it in `mode`: computed once, shared, never modified."""
    from oracle import c_oracle
    if K not in _cache:
        _cache[K] = {"inputs": boundary_corpus(K)}
    ptr, ids, cts, eta, alpha = _cache[K]["inputs"]
    key = (bool(MODES[mode].get("heldout")), MODES[mode].get("max_iter", 50))
    if key not in _cache[K]:
        ref = c_oracle.e_step(alpha, eta, ptr, ids, cts, max_iter=key[1], heldout=key[0])
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[K][key] = ref
    return (ptr, ids, cts, eta, alpha), _cache[K][key]


def check_against(out, ref, heldout, what):
    assert np.array_equal(out["iters"], ref["iters"]), what
    assert rel_err(out["gamma"], ref["gamma"]) < GAMMA_RTOL_ORACLE, what
    assert rel_err(out["doc_ll"], ref["doc_ll"]) < LL_RTOL, what
    if not heldout:
        assert np.max(np.abs(out["sstats"] - ref["sstats"])) < SSTATS_ATOL, what


@pytest.mark.parametrize("K", KS)
def test_the_two_oracles_agree_on_these_inputs(K):
    """The reference alone satisfies the bars on these inputs (numpy oracle against the C oracle, CPU): no iteration
    count sits on the stop threshold."""
    from oracle import vb_numpy
    (ptr, ids, cts, eta, alpha), ref = inputs_and_reference(K, "hand-over")
    other = vb_numpy.e_step(alpha, eta, ptr, ids, cts)
    check_against(other, ref, False, "numpy oracle, K=%d" % K)


def run(capi, K, inputs, packed, options=(), heldout=False, max_iter=50):
    ptr, ids, cts, eta, alpha = inputs
    ctx = capi.Context(K, V)
    ctx.set_option("quad_packed", packed)
    for name, value in options:
        ctx.set_option(name, value)
    corpus = ctx.corpus(ptr, ids, cts)
    out = ctx.estep_host(corpus, alpha, eta, max_iter, 1e-6, heldout)
    out["flagged"] = ctx.estep_results(corpus)[2]
    out["plan"] = corpus.plan()
    out["quad_slot_bytes"] = corpus.layout("quad_slot_bytes")
    corpus.close()
    ctx.close()
    return out


def expected_slot_bytes(plan):
    """What host_plan.cpp quad_slot_layout allots: a 32-byte record and 16 word groups x (slots rounded up to 4) ids per
    launch slot of a stride-256 quad class."""
    total = 0
    for c in plan:
        rn = c["geometry"]
        if c["kernel"] == "quad" and rn % 1000000 // 10000 == 32:
            wpg = rn % 10000 // 100 + rn % 100 + rn // 1000000
            total += c["documents"] * (32 + 16 * ((wpg + 3) // 4 * 4) * 4)
    return total


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("K", KS)
def test_packed_prologue_matches_the_oracle_and_the_unpacked_chain_bitwise(K, mode):
    from pylda_amd import _capi
    inputs, ref = inputs_and_reference(K, mode)
    kw = MODES[mode]
    heldout = bool(kw.get("heldout"))
    outs = {packed: run(_capi, K, inputs, packed, **kw) for packed in (1, 0)}
    # every lane shape of the quad kernel ran, the streamed ones included
    tl = 160000 if K <= 128 else 320000
    shapes = {tl + 800, tl + 1000, tl + 1001, tl + 1002, tl + 1003, tl + 1004} | \
        ({2000000 + tl + 904, 3000000 + tl + 904} if K <= 128 else {3000000 + tl + 804, 4000000 + tl + 804})
    for packed, out in outs.items():
        assert {c["geometry"] for c in out["plan"] if c["kernel"] == "quad"} == shapes, out["plan"]
        assert sum(c["documents"] for c in out["plan"] if c["kernel"] == "quad") == D
        assert out["flagged"] == 0
        assert out["quad_slot_bytes"] == expected_slot_bytes(out["plan"])
        assert (out["quad_slot_bytes"] > 0) == (K > 128)
        check_against(out, ref, heldout, "quad_packed=%d K=%d %s" % (packed, K, mode))
    for name in ("gamma", "iters", "doc_ll") + (() if heldout else ("sstats",)):
        assert np.array_equal(outs[1][name], outs[0][name]), name

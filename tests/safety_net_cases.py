"""Cases for the E-step's safety net: the `bad` exit of a dense kernel (status 1), estep_logspace_kernel redoing the flagged
documents, their statistics added behind the gather.  Plain module, no GPU: tests/test_safety_net_host.py checks the cases on
the CPU, tests/test_gpu_safety_net.py runs them on the device.

predict_flagged() is the dense kernels' linear-space iteration in numpy.  The kernels scale t in one of two ways and the
scale decides which documents leave the fp64 range:

  "sum"  t_k = exp(psi(gamma_k) - psi(sum gamma))   estep_qfusek.h (and the register kernels of K <= 512)
  "max"  t_k = exp(psi(gamma_k) - max_j psi(gamma_j))   estep_generic.h (every K > 1024)

With "sum" a document of one token at K >= 1024 and alpha <= 3e-4 starts at gamma ~ 1e-3, psi ~ -900: every t_k is an exact
zero in iteration 1.  With "max" the largest t_k is 1 by construction and the normaliser of word w is at least B[w][k*]: the
generic kernels flag a document only where the topic that holds its mass does not know one of its words at all - B[w][k*] an
exact zero.  anchored_model() builds that: topic 0 knows nothing but a few anchor words and it alone knows them (eta 1e-3
elsewhere: E log eta ~ -1000 below the other entries of the word), so in a document of one anchor word and one ordinary word
topic 0 takes the anchor word's token in iteration 1, the other topics stay at gamma ~ 1e-3, and the ordinary word's
normaliser is an exact zero in iteration 2 - under either scale.

Every case keeps a margin: a document's smallest normaliser is below 1e-300 (in practice exactly 0) or above 1e-250, so a few
ulp between the device's t and numpy's cannot move a document across the kernels' 1e-280 threshold."""
import functools

import numpy as np
from scipy.special import psi

FLAG_BELOW, FLAG_ABOVE = 1e-280, 1e300          # estep_generic.h / estep_qfusek.h: !(nrm > 1e-280 && nrm < 1e300)
MARGIN_LOW, MARGIN_HIGH = 1e-300, 1e-250


def linear_tables(eta):
    """B[w][k] = exp(E log eta[k][w] - max_j E log eta[j][w]) as the kernels read it (V x K)."""
    eta = np.asarray(eta, dtype=np.float64)
    elog = psi(eta) - psi(eta.sum(axis=1))[:, None]
    with np.errstate(under="ignore"):
        return np.exp(elog - elog.max(axis=0)[None, :]).T.copy()


def predict_flagged(alpha, eta, ptr, ids, cts, max_iter=50, tol=1e-6, scale="sum"):
    """Per document: (smallest normaliser over the iterations the document runs, the iteration - from 1 - at which a
    normaliser first leaves (1e-280, 1e300), 0 where none does).  A document stops at its first bad iteration: what the
    kernel computes behind it is discarded."""
    alpha = np.asarray(alpha, dtype=np.float64)
    K = alpha.size
    B = linear_tables(eta)
    D = len(ptr) - 1
    smallest, bad_at = np.full(D, np.inf), np.zeros(D, dtype=np.int64)
    for d in range(D):
        lo, hi = int(ptr[d]), int(ptr[d + 1])
        if hi == lo:
            continue
        b, c = B[ids[lo:hi]], np.asarray(cts[lo:hi], dtype=np.float64)
        gamma = alpha + c.sum() / K
        psi_total = psi(alpha.sum() + c.sum())          # (sum gamma is conserved by the update)
        for it in range(1, max_iter + 1):
            ps = psi(gamma)
            with np.errstate(under="ignore"):
                t = np.exp(ps - (psi_total if scale == "sum" else ps.max()))
                nrm = b @ t
            smallest[d] = min(smallest[d], nrm.min())
            if not np.all((nrm > FLAG_BELOW) & (nrm < FLAG_ABOVE)):
                bad_at[d] = it
                break
            new = alpha + t * ((c / nrm) @ b)
            change = np.mean(np.abs(new - gamma))
            gamma = new
            if change <= tol:
                break
    return smallest, bad_at


def margin_holds(smallest):
    return bool(np.all((smallest < MARGIN_LOW) | (smallest > MARGIN_HIGH)))


def statistics_bar(V, ids, cts):
    """Absolute bar on the sufficient statistics per word against an fp64 ORACLE: the suite's 1e-8 - and for the one word that
    carries a count of 10^5 or more, 1e-13 of its tokens on top (1e-7 at 10^6 tokens).  An entry of that column is up to 10^6
    tokens times phi, and the reference itself is only fp64 there: the C oracle and the numpy oracle, two statements of the
    same lines, differ in that column by up to 3.7e-8 (the count placed in documents of 1 to 65 terms, K = 65 to 1024:
    1.0e-8 to 3.7e-8 in eleven of sixteen placements) - 4e-14 of the word's tokens, rounding of fifty iterations.  The
    allowance is 2.7 times that measured gap; every other column keeps 1e-8, and the flat 1e-8 holds for every column
    wherever the reference is the mpmath golden."""
    bar = np.full(V, 1e-8)
    heavy = np.asarray(cts) >= 10 ** 5
    np.add.at(bar, np.asarray(ids)[heavy], 1e-13 * np.asarray(cts, dtype=np.float64)[heavy])
    return bar[None, :]


def csr(docs):
    """[(ids, cts), ...] -> (ptr int64, ids int32, cts int32), the terms of a document in ascending order."""
    ptr, ids, cts = [0], [], []
    for i, c in docs:
        i, c = np.asarray(i, dtype=np.int64), np.asarray(c, dtype=np.int64)
        at = np.argsort(i, kind="stable")
        assert np.unique(i).size == i.size
        ids.append(i[at])
        cts.append(c[at])
        ptr.append(ptr[-1] + i.size)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return np.array(ptr, dtype=np.int64), cat(ids, np.int32), cat(cts, np.int32)


def documents_of_lengths(rng, V, lengths, first_word=0, heavy_in=None):
    """Documents with exactly the given numbers of distinct terms among the words first_word .. V - 1, counts 1-4; document
    `heavy_in` gets a count of 10^6 on its first term."""
    docs = []
    for d, n in enumerate(lengths):
        i = first_word + rng.choice(V - first_word, size=n, replace=False)
        c = rng.integers(1, 5, size=n)
        if heavy_in is not None and d == heavy_in and n:
            c[0] = 10 ** 6
        docs.append((i, c))
    return docs


# ---- 1. the log-space kernel at its own branch points (force_logspace) ----
BRANCH_K = (1, 2, 63, 64, 65, 255, 256, 257, 700, 1024)
BRANCH_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1030)       # words by 4 (wavefronts), terms by 256 (threads)
BRANCH_V = 1100
SETTINGS = ((50, 1e-6), (1, 1e-6), (2, 1e-6), (50, 1e-1), (7, 0.0))     # (max_iter, tol)


@functools.lru_cache(maxsize=None)
def branch_case(K):
    """alpha, eta, ptr, ids, cts: documents of every boundary length, one term of 10^6 (in the document of 65 terms)."""
    rng = np.random.default_rng(4000 + K)
    lengths = [min(n, 300) if K >= 700 else n for n in BRANCH_LENGTHS]
    ptr, ids, cts = csr(documents_of_lengths(rng, BRANCH_V, lengths, heavy_in=BRANCH_LENGTHS.index(65)))
    eta = rng.gamma(100.0, 0.01, (K, BRANCH_V))
    eta[:, rng.choice(BRANCH_V, BRANCH_V // 4, replace=False)] = 1.0 / BRANCH_V
    alpha = rng.uniform(0.05, 1.5, K)
    return alpha, eta, ptr, ids, cts


# ---- 2. documents the dense kernels flag themselves ----
ANCHORS = 4                       # words 0 .. 3: the only words topic 0 knows
FLAT = 12                         # words 4 .. 15: eta = 0.5 in every topic but 0, so a token of theirs spreads evenly over them
GENERIC = {"generic64", "generic256", "generic512", "generic_global", "generic_huge"}
NATURAL = {                       # name -> (K, alpha, V, kernels of the plan, scale of t)
    "K1024_a1e-4": (1024, 1e-4, 400, {"qfusek"}, "sum"),
    "K1024_a3e-4": (1024, 3e-4, 400, {"qfusek"}, "sum"),
    "K2000_a1e-4": (2000, 1e-4, 400, GENERIC, "max"),
    "K2000_a3e-4": (2000, 3e-4, 400, GENERIC, "max"),
    "K3325_a1e-4": (3325, 1e-4, 400, GENERIC, "max"),       # (LARGEST_K below)
    "K3325_a3e-4": (3325, 3e-4, 400, GENERIC, "max"),
}


def scale_at(name, tol):
    """The scale of t in the kernels that run the case at this threshold: outside 2^-28 <= tol K < 1024 the fixed-point stop
    test of the streaming kernels does not apply and the generic kernels take every document (host_plan.cpp choose_variant)."""
    K, scale = NATURAL[name][0], NATURAL[name][4]
    return scale if 2.0 ** -28 <= tol * K < 1024.0 else "max"


def anchored_model(rng, K, V):
    """eta of an ordinary model, but topic 0 knows the anchor words and nothing else, and no other topic knows them."""
    eta = rng.gamma(100.0, 0.01, (K, V))
    eta[:, ANCHORS:ANCHORS + FLAT] = 0.5
    eta[0, :] = 1e-3
    eta[:, :ANCHORS] = 1e-3
    eta[0, :ANCHORS] = 50.0
    return eta


def natural_documents(rng, K, V):
    """Flagged and unflagged documents over the same words.  In order: an empty document; documents of one token (K = 1024:
    flagged in iteration 1; the generic kernels finish them) and, at the larger K, of 2-5 tokens of one term; an anchor word
    and a flat word, one token each (flagged in iteration 2 by every kernel); 2-12 tokens that stay in range; ordinary
    documents of 40-400 terms (four at K = 1024, two above), every other one with an anchor word."""
    first = ANCHORS + FLAT
    shared = first + rng.choice(V - first, size=24, replace=False)               # the words of the short documents
    docs = [([], [])]
    for j in range(6):
        docs.append(([shared[j]], [1]))
    if K > 1024:
        for j, n in enumerate((2, 3, 5)):
            docs.append(([shared[6 + j]], [n]))
    for j in range(6):
        docs.append(([j % ANCHORS, ANCHORS + j], [1, 1]))
    for j, n in enumerate((6, 8, 12)):                                          # n tokens on four ordinary words
        docs.append((shared[9 + 4 * j:13 + 4 * j], [n - 3, 1, 1, 1]))
    for n, anchor in ((40, True), (90, False), (150, True), (400, False)) if K <= 1024 else ((40, True), (400, False)):
        i = np.concatenate([shared[:12], ANCHORS + np.arange(8), first + rng.permutation(V - first)])
        i = i[np.sort(np.unique(i, return_index=True)[1])][:n - (1 if anchor else 0)]
        if anchor:
            i = np.concatenate([[1], i])
        docs.append((i, rng.integers(1, 5, size=i.size)))
    return docs


@functools.lru_cache(maxsize=None)
def natural_case(name):
    """alpha, eta, ptr, ids, cts of a NATURAL case; the margin is asserted for every (max_iter, tol) of SETTINGS."""
    K, a, V, _, _ = NATURAL[name]
    rng = np.random.default_rng(K)
    eta = anchored_model(rng, K, V)
    ptr, ids, cts = csr(natural_documents(rng, K, V))
    alpha = np.full(K, a)
    for max_iter, tol in SETTINGS:
        smallest, _ = predict_flagged(alpha, eta, ptr, ids, cts, max_iter, tol, scale_at(name, tol))
        assert margin_holds(smallest), (name, max_iter, tol, smallest)
    return alpha, eta, ptr, ids, cts


def natural_flagged(name, max_iter=50, tol=1e-6):
    """Indices of the documents the case's dense kernel flags."""
    alpha, eta, ptr, ids, cts = natural_case(name)
    return np.nonzero(predict_flagged(alpha, eta, ptr, ids, cts, max_iter, tol, scale_at(name, tol))[1])[0]


CHUNK_D = 2100                    # more than 4 workgroups x 256 CUs: estep_logspace_kernel's chunk is 3 documents


@functools.lru_cache(maxsize=None)
def chunk_case():
    """K = 1024, alpha 1e-4: documents of one token (flagged) and of ten tokens (not) in turn."""
    K, V = 1024, 300
    rng = np.random.default_rng(77)
    eta = rng.gamma(100.0, 0.01, (K, V))
    docs = []
    for d in range(CHUNK_D):
        if d % 2 == 0:
            docs.append(([rng.integers(V)], [1]))
        else:
            docs.append((rng.choice(V, size=3, replace=False), [8, 1, 1]))
    ptr, ids, cts = csr(docs)
    alpha = np.full(K, 1e-4)
    smallest, bad_at = predict_flagged(alpha, eta, ptr, ids, cts, 50, 1e-6, "sum")
    assert margin_holds(smallest) and np.array_equal(np.nonzero(bad_at)[0], np.arange(0, CHUNK_D, 2))
    return alpha, eta, ptr, ids, cts


def collapsed_alpha_inputs():
    """The inputs of tests/test_gpu_estep.py::test_collapsed_alpha_triggers_safety_net (max_iter = 3)."""
    rng = np.random.default_rng(5)
    K, V, D = 4, 40, 12
    eta = np.full((K, V), 1e-3)
    for k in range(K):
        eta[k, k * 10:(k + 1) * 10] = 50.0
    alpha = np.array([1e-4, 1e-4, 1e-4, 5.0])
    ptr, ids, cts = [0], [], []
    for d in range(D):
        k = d % 3
        w = rng.choice(np.arange(k * 10, (k + 1) * 10), size=3, replace=False)
        ids += list(w)
        cts += [1, 1, 1]
        ptr.append(len(ids))
    return alpha, eta, np.array(ptr), np.array(ids, np.int32), np.array(cts, np.int32)


# ---- 4. the live-topic guard's route into the net ----
def guard_case(K):
    """A topical corpus (tests/test_gpu_live_topics.py) whose documents the quad / fused streaming kernels hand over."""
    rng = np.random.default_rng(900 + K)
    V, D, true_topics = 600, 40, 24
    beta = rng.dirichlet(np.full(V, 0.02), size=true_topics)
    docs = []
    for _ in range(D):
        theta = rng.dirichlet(np.full(true_topics, 0.1))
        words = rng.choice(V, size=max(1, int(rng.poisson(150))), p=theta @ beta)
        docs.append(np.unique(words, return_counts=True))
    eta = rng.gamma(100.0, 0.01, (K, V))
    for k in range(K):
        eta[k] += 40.0 * V * beta[k % true_topics] * rng.uniform(0.2, 1.0)
    return (np.full(K, 1.0 / K), eta) + csr(docs)


# ---- 5. the LDS boundary ----
LDS_BYTES = 160 * 1024            # gfx950
LDS_MARGIN = 3072                 # estep_limits.h kLdsMargin: the runtime refuses a request within 3 KiB of the limit


def logspace_launch_bytes(K):
    """estep_limits.h logspace_launch_lds_bytes: psi, gamma, four partial gammas and scratch, rounded up to 16 bytes, then the
    list of a chunk's flagged documents (256 + 1 ints)."""
    return (((6 * K + 4) * 8 + 64 + 15) & ~15) + 257 * 4


LARGEST_K = max(K for K in range(3000, 3500) if logspace_launch_bytes(K) + LDS_MARGIN <= LDS_BYTES)
assert LARGEST_K == 3325 and all(NATURAL[name][0] <= LARGEST_K for name in NATURAL)


@functools.lru_cache(maxsize=None)
def boundary_case(K):
    """A small corpus for K around the LDS limit: anchored documents (flagged in iteration 2), one-token and ordinary ones."""
    V = 300
    rng = np.random.default_rng(K)
    eta = anchored_model(rng, K, V)
    docs = [([j % ANCHORS, ANCHORS + j], [1, 1]) for j in range(4)] + [([20 + j], [1]) for j in range(3)]
    docs += documents_of_lengths(rng, V, (40, 120), first_word=ANCHORS)
    ptr, ids, cts = csr(docs)
    alpha = np.full(K, 1e-4)
    smallest, bad_at = predict_flagged(alpha, eta, ptr, ids, cts, 50, 1e-6, "max")
    assert margin_holds(smallest) and np.array_equal(np.nonzero(bad_at)[0], np.arange(4))
    return alpha, eta, ptr, ids, cts


# ---- the mpmath golden (tests/golden/make_logspace_mp.py) ----
MP_CASES = (                      # name, K, lengths, alpha (None: 0.1 + 0.05 (k mod 7)), V
    ("K65", 65, (1, 4, 5), None, 8),
    ("K257", 257, (1, 3), None, 8),
    ("K1024", 1024, (1, 1, 2), 1e-4, 8),
    ("K1", 1, (3,), None, 8),
)
MP_MAX_ITER = (50, 1)


def mp_inputs(name):
    """alpha, eta, ptr, ids, cts of a golden case, from closed formulas: the same doubles wherever they are evaluated."""
    _, K, lengths, a, V = next(c for c in MP_CASES if c[0] == name)
    k, w = np.arange(K)[:, None], np.arange(V)[None, :]
    eta = 0.5 + ((k * 7 + w * 13 + (k * w) % 5) % 29) / 8.0
    alpha = np.full(K, a) if a is not None else 0.1 + 0.05 * (np.arange(K) % 7)
    docs, at = [], 0
    for d, n in enumerate(lengths):
        i = [(at + 3 * j) % V for j in range(n)]
        at += 1
        c = [1 + (j + d) % 3 for j in range(n)]
        if d == len(lengths) - 1 and a is None:
            c[-1] = 10 ** 6                           # one heavy count per case (K = 1024 keeps its few-token documents)
        docs.append((i, c))
    return (alpha, eta) + csr(docs)

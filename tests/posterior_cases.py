"""States of the collapsed Gibbs engine at which its log posterior (pylda_gibbs_log_posterior, estep_gibbs.h) is compared
with mpmath, term by term, and the error bound of every term.  Deterministic builders, seeded, numpy only: the golden
maker (tests/golden/make_posterior_mp.py), tests/test_gibbs_posterior_host.py and tests/test_gpu_gibbs_posterior.py all
import this module, and tests/golden/posterior_mp.npz stores a hash of every case's inputs.

A case is (K, V, n_dk, n_kv, n_k, alpha, beta) plus a corpus and its tokens' topics that realise n_dk.  n_kv and n_k are
INJECTED through gibbs_set_state, which does not require the word-topic table to agree with the tokens: n_dk is recounted
from the topics, the table and n_k are taken as given.  That is what lets a cell hold 2^31 - 1 without two billion
tokens.  (Every case keeps n_k = the rows' sums of n_kv, so that gibbs_restatement.log_posterior, which derives n_k that
way, applies to all of them.)

The builders use no transcendental function - a "log-uniform" prior is a uniform mantissa in [1, 10) times an exact
power-of-ten literal - so the same numpy gives the same bits everywhere and the stored hashes hold.

What the grid covers:
  doc_K<K>_D<D>      the document kernel: one wavefront per document, k += 64, four documents per workgroup
  word_K<K>          the word kernel: one workgroup per word, k += 256, table stride ldk != K (255, 257, 700) and
                     ldk == K (256, 1024; host_plan.h table_stride_for)
  sum_D<D>_V<V>      the two sum kernels: one workgroup, strides of 256 over D, V and K = 300; D = 0 included
  prior_*_K<K>       alpha and beta at 1e-6, at 1e3 and spread over 1e-6 .. 1e3; sum alpha and sum beta just below and
                     just above 12 (lgamma_pos branches there) beside an empty document and topics with n_k = 0;
                     count + prior within 1e-9 of 12 from either side
  heavy_K<K>         a document of 10^6 tokens of one term in one topic; cells of 1, 2, 10^3, 10^6, 2^31 - 1; n_k up to
                     2^31 - 1
"""
import hashlib
import zlib

import numpy as np
import scipy.special

from special_bounds import LGAMMA_SCALED

U = 2.0 ** -53
INT32_MAX = 2 ** 31 - 1
DECADES = [1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e0, 1e1, 1e2]       # times a mantissa in [1, 10): 1e-6 .. 1e3

DOC_K = (1, 63, 64, 65, 127, 128, 129)
DOC_D = (1, 3, 4, 5, 9)
WORD_K = (255, 256, 257, 700, 1024)
SUM_D = (255, 256, 257)
SUM_V = (1, 255, 256, 257, 600)
PRIOR_K = (65, 257)
PRIOR_KINDS = ("tiny", "huge", "spread")
SLICE_CASES = ("doc_K65_D9", "sum_D257_V257")       # the states of the hyper-parameter step's test (K = 65, K = 300)
# numpy seeds (symmetric switches on / off) under which every accept decision of the step is far from its threshold
# (tests/test_gibbs_posterior_host.py vouches for them)
SLICE_SEEDS = {("doc_K65_D9", True): 2, ("doc_K65_D9", False): 3, ("sum_D257_V257", True): 6, ("sum_D257_V257", False): 0}


def corpus_of_counts(n_dk, n_kv):
    """A corpus and its tokens' topics whose counts are (n_dk, n_kv): per topic, the documents' slots paired with the
    terms' slots."""
    D, K = n_dk.shape
    V = n_kv.shape[1]
    docs, terms, topics = [], [], []
    for k in range(K):
        docs.append(np.repeat(np.arange(D), n_dk[:, k]))
        terms.append(np.repeat(np.arange(V), n_kv[k]))
        topics.append(np.full(int(n_kv[k].sum()), k))
    docs, terms, topics = np.concatenate(docs), np.concatenate(terms), np.concatenate(topics)
    order = np.lexsort((terms, docs))
    docs, terms, topics = docs[order], terms[order], topics[order]
    pair = docs * V + terms
    first = np.concatenate([[True], pair[1:] != pair[:-1]])
    ids = terms[first].astype(np.int32)
    cts = np.diff(np.concatenate([np.nonzero(first)[0], [len(pair)]])).astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(docs[first], minlength=D))]).astype(np.int64)
    return (ptr, ids, cts), topics.astype(np.int32)


class Case(object):
    def __init__(self, name, n_dk, n_kv, alpha, beta):
        self.name = name
        self.n_dk = np.ascontiguousarray(n_dk, dtype=np.int64)
        self.n_kv = np.ascontiguousarray(n_kv, dtype=np.int64)
        self.n_k = self.n_kv.sum(axis=1)
        self.alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        self.beta = np.ascontiguousarray(beta, dtype=np.float64)
        self.D, self.K = self.n_dk.shape
        self.V = self.n_kv.shape[1]
        assert self.n_kv.shape[0] == self.K and self.alpha.shape == (self.K,) and self.beta.shape == (self.V,)
        assert self.n_dk.min(initial=0) >= 0 and self.n_kv.min() >= 0 and self.n_k.max() <= INT32_MAX
        assert np.all(self.alpha > 0) and np.all(self.beta > 0)

    def corpus(self):
        """((doc_ptr, term_id, term_ct), topics): the tokens of topic k all carry the term k modulo V - the table that
        goes to the device is n_kv, not the tokens' own."""
        own = np.zeros((self.K, self.V), dtype=np.int64)
        own[np.arange(self.K), np.arange(self.K) % self.V] = self.n_dk.sum(axis=0)
        if self.D == 0:
            return (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)), np.zeros(0, np.int32)
        return corpus_of_counts(self.n_dk, own)

    def digest(self):
        h = hashlib.sha256()
        for a in (np.array([self.K, self.V, self.D], dtype=np.int64), self.n_dk, self.n_kv, self.n_k, self.alpha, self.beta):
            h.update(np.ascontiguousarray(a).tobytes())
        return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _usual_priors(rng, K, V):
    """vector alpha, vector beta, drawn as tests/test_gpu_gibbs.py draws them"""
    return rng.uniform(0.02, 0.5, K), rng.uniform(0.005, 0.2, V)


def _spread(rng, n):
    return rng.uniform(1.0, 10.0, n) * np.array(DECADES)[rng.integers(0, len(DECADES), n)]


def _sparse_rows(rng, rows, cols, nonzero, high):
    """(rows, cols) counts: `nonzero` cells of every row in 1 .. high, the others 0"""
    out = np.zeros((rows, cols), dtype=np.int64)
    for r in range(rows):
        at = rng.choice(cols, size=min(nonzero, cols), replace=False)
        out[r, at] = rng.integers(1, high + 1, at.size)
    return out


def _row_of_tokens(rng, K, tokens):
    """one document's counts: `tokens` tokens thrown at K topics"""
    return np.bincount(rng.integers(0, K, tokens), minlength=K)


def _document_case(K, D):
    name = "doc_K%d_D%d" % (K, D)
    rng = _rng(name)
    V = 40
    one = lambda k, n: np.bincount([k], weights=[n], minlength=K).astype(np.int64)
    special = [one(K - 1, 7),                                       # one non-zero topic, the last one
               np.zeros(K, dtype=np.int64),                          # an empty document
               one(64, 5) if K > 64 else one(K // 2, 5),             # only topic 64: the second trip's first lane
               _row_of_tokens(rng, K, 65), _row_of_tokens(rng, K, 63), _row_of_tokens(rng, K, 64),
               rng.integers(1, 30, K),                               # dense: no zero cell
               _row_of_tokens(rng, K, 200), _row_of_tokens(rng, K, 3)]
    start = 0 if D >= len(special) else (2 * D) % len(special)      # (the short corpora start at different rows)
    n_dk = np.array([special[(start + i) % len(special)] for i in range(D)])
    if n_dk.sum() == 0:
        n_dk[0] = special[3]
    n_kv = _sparse_rows(rng, K, V, 8, 50)
    alpha, beta = _usual_priors(rng, K, V)
    return Case(name, n_dk, n_kv, alpha, beta)


def _word_case(K):
    name = "word_K%d" % K
    rng = _rng(name)
    n_kv = np.zeros((K, 3), dtype=np.int64)                          # word 0: empty, lgamma(beta) on every cell
    n_kv[K - 1, 1] = 4                                               # word 1: the last topic, and the second trip's first
    if K > 256:
        n_kv[256, 1] = 9
    n_kv[:, 2] = rng.integers(1, 200, K)                             # word 2: dense
    n_dk = _sparse_rows(rng, 5, K, 12, 20)
    alpha, beta = _usual_priors(rng, K, 3)
    return Case(name, n_dk, n_kv, alpha, beta)


def _sum_case(D, V):
    name = "sum_D%d_V%d" % (D, V)
    rng = _rng(name)
    K = 300
    n_dk = _sparse_rows(rng, D, K, 3, 40)
    n_kv = _sparse_rows(rng, V, K, 2, 60).T
    alpha, beta = _usual_priors(rng, K, V)
    return Case(name, n_dk, n_kv, alpha, beta)


def _prior_of(kind, rng, n):
    return {"tiny": np.full(n, 1e-6), "huge": np.full(n, 1e3), "spread": _spread(rng, n)}[kind]


def _prior_state(rng, K, V=30, D=6):
    n_dk = _sparse_rows(rng, D, K, 6, 300)
    n_dk[1] = 0                                                       # an empty document: lgamma(sum alpha) itself
    n_kv = _sparse_rows(rng, V, K, 5, 400).T
    n_kv[3] = 0                                                       # topics with n_k = 0: lgamma(sum beta) itself
    n_kv[K - 1] = 0
    return n_dk, n_kv


def _prior_case(K, alpha_kind, beta_kind):
    name = "prior_a%s_b%s_K%d" % (alpha_kind, beta_kind, K)
    rng = _rng(name)
    n_dk, n_kv = _prior_state(rng, K)
    return Case(name, n_dk, n_kv, _prior_of(alpha_kind, rng, K), _prior_of(beta_kind, rng, n_kv.shape[1]))


def _scaled_to(values, target):
    """values times a factor that brings their sum to about `target`"""
    return values * (target / values.sum())


def _sum12_case(K, side):
    """sum alpha and sum beta at 12 (1 -/+ 1e-12): the exact sums and the sums in the host's order lie on that side
    (the tests assert it)"""
    name = "prior_sum12_%s_K%d" % (side, K)
    rng = _rng(name)
    n_dk, n_kv = _prior_state(rng, K)
    target = 12.0 * (1.0 - 1e-12) if side == "below" else 12.0 * (1.0 + 1e-12)
    alpha = _scaled_to(rng.uniform(0.02, 0.5, K), target)
    beta = _scaled_to(rng.uniform(0.005, 0.2, n_kv.shape[1]), target)
    return Case(name, n_dk, n_kv, alpha, beta)


def _near12_case(K):
    """count + prior within 1e-9 of 12, from below and from above, in the document and in the word kernel"""
    name = "prior_near12_K%d" % K
    rng = _rng(name)
    n_dk, n_kv = _prior_state(rng, K)
    alpha, beta = _usual_priors(rng, K, n_kv.shape[1])
    alpha[0], alpha[1], alpha[K - 1], alpha[K - 2] = 1.0 - 5e-10, 1.0 + 5e-10, 12.0 - 3e-10, 12.0 + 3e-10
    n_dk[0, 0] = n_dk[0, 1] = n_dk[2, 0] = n_dk[3, 1] = 11
    n_dk[:, K - 1] = n_dk[:, K - 2] = 0
    n_dk[4, K - 1] = 1                                               # (13 - 3e-10: the far side, for contrast)
    beta[0], beta[1], beta[2] = 2.0 - 7e-10, 2.0 + 7e-10, 12.0 + 1e-10
    n_kv[0, 0] = n_kv[1, 1] = n_kv[K - 2, 0] = n_kv[K - 2, 1] = 10
    n_kv[:, 2] = 0
    return Case(name, n_dk, n_kv, alpha, beta)


def _heavy_case(K):
    name = "heavy_K%d" % K
    rng = _rng(name)
    V = 12
    n_dk = _sparse_rows(rng, 4, K, 5, 50)
    n_dk[1] = 0
    n_dk[1, 64] = 10 ** 6                                            # 10^6 tokens of one term in one topic
    n_kv = _sparse_rows(rng, V, K, 3, 30).T
    n_kv[0] = 0
    n_kv[0, 5] = INT32_MAX                                           # a cell and an n_k of 2^31 - 1
    n_kv[K - 1] = 0
    n_kv[K - 1, V - 1] = INT32_MAX - 10 ** 6 - 10 ** 3 - 3           # n_k = 2^31 - 1 from four cells
    n_kv[K - 1, :4] = [1, 2, 10 ** 3, 10 ** 6]
    n_kv[62, 0] = 10 ** 6
    n_kv[63, 1] = 10 ** 3
    alpha, beta = _usual_priors(rng, K, V)
    return Case(name, n_dk, n_kv, alpha, beta)


def _builders():
    out = {}
    for K in DOC_K:
        for D in DOC_D:
            out["doc_K%d_D%d" % (K, D)] = (_document_case, (K, D))
    for K in WORD_K:
        out["word_K%d" % K] = (_word_case, (K,))
    for D in SUM_D:
        for V in SUM_V:
            out["sum_D%d_V%d" % (D, V)] = (_sum_case, (D, V))
    out["sum_D0_V257"] = (_sum_case, (0, 257))
    for K in PRIOR_K:
        for a in PRIOR_KINDS:
            for b in PRIOR_KINDS:
                out["prior_a%s_b%s_K%d" % (a, b, K)] = (_prior_case, (K, a, b))
        for side in ("below", "above"):
            out["prior_sum12_%s_K%d" % (side, K)] = (_sum12_case, (K, side))
        out["prior_near12_K%d" % K] = (_near12_case, (K,))
        out["heavy_K%d" % K] = (_heavy_case, (K,))
    return out


_BUILDERS = _builders()
NAMES = list(_BUILDERS)
_built = {}


def case(name):
    if name not in _built:
        fn, args = _BUILDERS[name]
        _built[name] = fn(*args)
        assert _built[name].name == name
    return _built[name]


# ---- the bound --------------------------------------------------------------------------------------------------------
def term_bound(values, psi=None, n_priors=0, prior_sum=0.0):
    """Bound of a device term that is a sum of the m values v_i = ln Gamma(x_i), each from lgamma_pos:
        sum_i LGAMMA_SCALED max(1, |v_i|)      the function's committed bound (special_bounds.py), per value
      + (m + 1) 2^-53 sum_i |v_i|              m - 1 additions in any order, with room for the last subtraction
      + sum_i |psi_i| n_priors 2^-53 prior_sum where x_i takes a sum of n_priors priors that the HOST added up in doubles
                                               (the reference takes the exact sum): that sum is off by at most
                                               (n_priors - 1) 2^-53 prior_sum, and d ln Gamma / dx = psi.
    psi: None, or psi(x_i) for the values that take such a sum and 0 for the others."""
    v = np.abs(np.asarray(values, dtype=np.float64)).ravel()
    bound = LGAMMA_SCALED * np.sum(np.maximum(1.0, v)) + (v.size + 1) * U * np.sum(v)
    if psi is not None:
        bound += np.sum(np.abs(psi)) * n_priors * U * prior_sum
    return float(bound)


def bound_ratio(error, bound):
    """|error| / bound, elementwise; a bound of 0 (a sum without terms) admits an error of exactly 0 only"""
    error, bound = np.abs(np.atleast_1d(np.asarray(error, dtype=np.float64))), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    out = np.where(error == 0.0, 0.0, np.inf)                    # (a NaN is not within any bound)
    np.divide(error, bound, out=out, where=bound > 0.0)
    return out


def sum_bound(term_bounds, terms):
    """A device sum of n terms: its terms' bounds plus n 2^-53 sum |terms| for its own additions."""
    terms = np.asarray(terms, dtype=np.float64).ravel()
    return float(np.sum(term_bounds) + terms.size * U * np.sum(np.abs(terms)))


class Evaluation(object):
    """Every term of the log posterior in doubles (scipy's gammaln, numpy's sums) and the bound of every device output."""

    def __init__(self, n_dk, n_kv, n_k, alpha, beta):
        gl, psi = scipy.special.gammaln, scipy.special.digamma
        n_dk, n_kv, n_k = (np.asarray(a, dtype=np.float64) for a in (n_dk, n_kv, n_k))
        D, K = n_dk.shape
        V = n_kv.shape[1]
        alpha_sum, beta_sum = float(np.sum(alpha)), float(np.sum(beta))
        doc_values = gl(n_dk + alpha[np.newaxis, :])                                 # (D, K)
        doc_norm_x = n_dk.sum(axis=1) + alpha_sum
        doc_norm = gl(doc_norm_x)                                                    # (D,)
        self.docs = doc_values.sum(axis=1) - doc_norm
        self.doc_bounds = np.array([term_bound(np.concatenate([doc_values[d], doc_norm[d:d + 1]]), psi(doc_norm_x[d]), K, alpha_sum)
                                    for d in range(D)])
        word_values = gl(n_kv + beta[np.newaxis, :])                                 # (K, V)
        self.words = word_values.sum(axis=0)
        self.word_bounds = np.array([term_bound(word_values[:, v]) for v in range(V)])
        topic_values = gl(n_k + beta_sum)                                            # (K,)
        topic_bound = term_bound(topic_values, psi(n_k + beta_sum), V, beta_sum)
        half_docs = float(np.sum(self.docs))
        half_words = float(np.sum(self.words) - np.sum(topic_values))
        self.sums = np.array([half_docs + half_words, half_docs, half_words])
        word_side = np.concatenate([self.words, topic_values])
        self.sum_bounds = np.array([
            sum_bound(np.concatenate([self.doc_bounds, self.word_bounds, [topic_bound]]), np.concatenate([self.docs, word_side])),
            sum_bound(self.doc_bounds, self.docs),
            sum_bound(np.concatenate([self.word_bounds, [topic_bound]]), word_side)])
        # the host's scalar terms (ln Gamma(sum alpha) - sum_k ln Gamma(alpha_k)) D and the same of beta times K
        prior_values = [np.concatenate([gl(alpha), [gl(alpha_sum)]]), np.concatenate([gl(beta), [gl(beta_sum)]])]
        scalar_alpha = (gl(alpha_sum) - np.sum(gl(alpha))) * D
        scalar_beta = (gl(beta_sum) - np.sum(gl(beta))) * K
        bound_alpha = term_bound(prior_values[0], psi(alpha_sum), K, alpha_sum) * D
        bound_beta = term_bound(prior_values[1], psi(beta_sum), V, beta_sum) * K
        self.scalars = np.array([scalar_alpha, scalar_beta])
        # [the whole, the documents' part, the words' part] as the two public entry points return them; 4 2^-53 of the
        # addends: the products by D and K and the additions
        self.totals = np.array([scalar_alpha + scalar_beta + self.sums[0], scalar_alpha + self.sums[1], scalar_beta + self.sums[2]])
        round_off = 4 * U * np.array([abs(scalar_alpha) + abs(scalar_beta) + abs(self.sums[0]), abs(scalar_alpha) + abs(self.sums[1]),
                                      abs(scalar_beta) + abs(self.sums[2])])
        self.total_bounds = np.array([bound_alpha + bound_beta, bound_alpha, bound_beta]) + self.sum_bounds + round_off


def evaluate(c, alpha=None, beta=None):
    return Evaluation(c.n_dk, c.n_kv, c.n_k, c.alpha if alpha is None else alpha, c.beta if beta is None else beta)


# ---- the hyper-parameter step, with its decisions' margins ---------------------------------------------------------------
def slice_sample_with_margins(log_posterior, alpha, beta, symmetric_alpha, symmetric_beta, samples=10, step=1.0, iterations=50):
    """pylda_amd.monte_carlo.slice_sample_hyperparameters restated with a record of every accept decision:
    returns (alpha, beta, [(proposal alpha, proposal beta, log posterior(proposal) - threshold), ...]).  The host test
    asserts that it ends where the package's routine ends from the same numpy state."""
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    point_alpha, point_beta = np.log(alpha), np.log(beta)
    jitter = lambda shape, symmetric: np.random.random() if symmetric else np.random.random(shape)
    decisions = []
    for _ in range(samples):
        threshold = np.log(np.random.random()) + log_posterior(alpha, beta)
        point_alpha -= jitter(point_alpha.shape, symmetric_alpha) * step
        upper_alpha = point_alpha + step
        point_beta -= jitter(point_beta.shape, symmetric_beta) * step
        upper_beta = point_beta + step
        for _ in range(iterations):
            point_alpha += jitter(point_alpha.shape, symmetric_alpha) * (upper_alpha - point_alpha)
            new_alpha = np.exp(point_alpha)
            point_beta += jitter(point_beta.shape, symmetric_beta) * (upper_beta - point_beta)
            new_beta = np.exp(point_beta)
            lp = log_posterior(new_alpha, new_beta)
            decisions.append((new_alpha, new_beta, lp - threshold))
            if lp > threshold:
                alpha, beta = new_alpha, new_beta
                break
            upper_alpha[:] = point_alpha
            upper_beta[:] = point_beta
    return alpha, beta, decisions

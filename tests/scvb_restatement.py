"""Stochastic collapsed variational Bayes (SCVB0: Foulds, Boyles, DuBois, Smyth & Welling 2013) in numpy: the specification
the HIP kernels (pylda_amd/csrc/scvb_kernels.h) are compared against.

No per-token state: T (word-major expected word-topic counts), n_k (its column sums) and N_dk.  Step t visits block
t mod B - the documents whose global index is that modulo B - in epoch e = t // B.  Every document of the block runs
burn_in + 1 passes over its slots against the T and n_k of the step's start: a slot's distribution is recomputed from the
counts, and N_dk moves towards C_j times it by the "clumped" step 1 - (1 - rho_theta) ** c of the slot's c copies; the last
pass also leaves c times the distribution as the slot's delta row.  The block's rows are summed per word in CVB0's segment
order, T = keep * T + gain * (the word's sum) over EVERY word, and n_k is recomputed from T in CVB0's chunks.  Same start,
slot order, lane layout and fp64 operation sequence as the kernels, so every number agrees bit for bit (an update is add,
multiply and divide; the power is adds and multiplies only); vectorised over the documents of a block, which do not see each other.

textbook_step() is the same step written straight from the formulas - sequential, `**`, plain sums, none of the orderings
- for the test that guards this file against being wrong the way the kernel is.  Pure host code."""
import numpy as np

from cvb0_restatement import Cvb0Chain, block_rounds, start_rows
from hybrid_restatement import WAVE, _lane_sums, _wave_scan
from pylda_amd.online_vb import step_size


def _split(a):
    """Veltkamp: a = hi + lo with 26 bits each, adds and one multiply"""
    t = 134217729.0 * a
    hi = t - (t - a)
    return hi, a - hi


def _dd_mul(ah, al, bh, bl):
    """(ah + al) * (bh + bl) as a double-double: Dekker's exact product of the high parts (no fused multiply-add), the
    cross terms, one renormalisation.  Every operation is a rounded add, subtract or multiply, in this order."""
    p = ah * bh
    a1, a2 = _split(ah)
    b1, b2 = _split(bh)
    e = (((a1 * b1 - p) + a1 * b2) + a2 * b1) + a2 * b2
    e = e + (ah * bl + al * bh)
    hi = p + e
    return hi, e - (hi - p)


def binary_power(x, c):
    """x ** c for a scalar x in [0, 1] and an integer array c >= 0 by binary exponentiation in double-double arithmetic -
    r = 1; while n: if n & 1: r = r * x; n >>= 1; if n: x = x * x, every product a _dd_mul - rounded to a double at the
    end (the high part).  Adds and multiplies only, the same sequence in numpy and on the device.  (The same loop in plain
    doubles is not accurate enough: a squaring doubles the relative error it inherits, and 0.874 ** 300 comes out 54 ulp
    off.)  c = 1 gives x itself: 1 * x is exact."""
    n = np.array(c, dtype=np.int64, ndmin=1)
    rh, rl = np.ones(len(n)), np.zeros(len(n))
    xh, xl = np.full(len(n), float(x)), np.zeros(len(n))
    while np.any(n):
        odd = (n & 1) == 1
        mh, ml = _dd_mul(rh, rl, xh, xl)
        rh, rl = np.where(odd, mh, rh), np.where(odd, ml, rl)
        n = n >> 1
        more = n > 0
        sh, sl = _dd_mul(xh, xl, xh, xl)
        xh, xl = np.where(more, sh, xh), np.where(more, sl, xl)
    return rh


def step_parameters(t, batches, burn_in, tau0, kappa, theta_tau0, theta_kappa, corpus_tokens, block_tokens):
    """(keep, gain, rho_theta (P + 1), one_minus (P + 1)) of step t, as the host hands them to pylda_scvb_step"""
    rho_phi = step_size(tau0, kappa, t)
    epoch = t // batches
    rho_theta = [step_size(theta_tau0, theta_kappa, epoch * (burn_in + 1) + p) for p in range(burn_in + 1)]
    return 1.0 - rho_phi, rho_phi * (float(corpus_tokens) / float(block_tokens)), rho_theta, [1.0 - r for r in rho_theta]


class _ZeroTable(object):
    """What Cvb0Chain._apply reads of a chain, with a table of zeros: ((0 + partial_0) + partial_1) + .. is a word's
    sequential sum from 0.0 of its segments' partial rows."""

    def __init__(self, chain):
        self.term_id, self.KP = chain.term_id, chain.KP
        if chain._zeros is None:
            chain._zeros = np.zeros((chain.V, chain.KP))
        self.T = chain._zeros

    def clear(self, words):
        self.T[words] = 0.0


class ScvbChain(Cvb0Chain):
    def __init__(self, doc_ptr, term_id, term_ct, K, V, first_document=0):
        Cvb0Chain.__init__(self, doc_ptr, term_id, term_ct, K, V, first_document)
        self.g = None                                  # (no per-slot state)
        self._zeros = None                             # a V x KP table of zeros, the blend's scratch
        tok_off = np.concatenate([[0], np.cumsum(self.term_ct)]).astype(np.int64)
        self.doc_tokens = tok_off[self.doc_ptr[1:]] - tok_off[self.doc_ptr[:-1]]
        self.tokens = int(np.sum(self.term_ct))
        self.t = 0

    # ---- state ----
    def init(self, seed):
        K = self.K
        m = start_rows(self.doc_ptr, self.term_ct, K, seed, 0, self.first_document)
        self.T[:] = 0.0
        self.n_dk[:] = 0.0
        np.add.at(self.T[:, :K], self.term_id, m)              # integers: exact in any order
        np.add.at(self.n_dk[:, :K], self.slot_doc, m)
        self.doc_change[:] = 0.0
        self.recompute_n_k()
        self.t = 0

    def state(self):
        """(n_kv (K, V), n_k, n_dk) as pylda_scvb_get_state returns them."""
        K = self.K
        return self.T[:, :K].T.copy(), self.n_k[:K].copy(), self.n_dk[:, :K].copy()

    def set_state(self, n_kv, n_k, n_dk, t=0):
        K = self.K
        self.T[:] = 0.0
        self.T[:, :K] = np.asarray(n_kv).T
        self.n_k = np.zeros(self.KP)
        self.n_k[:K] = n_k
        self.n_dk[:] = 0.0
        self.n_dk[:, :K] = n_dk
        self.doc_change[:] = 0.0
        self.t = int(t)

    # ---- a step ----
    def _update(self, docs, al, beta, beta_sum, one_minus, place, rows):
        """The block's documents against the frozen T and n_k; returns delta (`rows` rows: a slot's is place[slot])."""
        K, KP, S = self.K, self.KP, self.S
        n = len(docs)
        old = self.n_dk[docs]
        nd = old.copy()
        real = np.arange(KP) < K
        den = np.where(real, self.n_k + beta_sum, 1.0)
        Cj = self.doc_tokens[docs].astype(np.float64)[:, np.newaxis]
        delta = np.zeros((rows, KP))
        nterm, ptr = self.nterm[docs], self.doc_ptr[docs]
        last = len(one_minus) - 1
        slots = np.concatenate([np.arange(b, e) for b, e in zip(ptr, ptr + nterm)]) if n else np.zeros(0, dtype=np.int64)
        power = np.zeros(self.nnz)
        for p, om in enumerate(one_minus):
            power[slots] = binary_power(om, self.term_ct[slots])        # (1 - rho) ** c of every slot of the block, this pass
            for j in range(int(nterm.max()) if n else 0):
                a = np.nonzero(nterm > j)[0]
                q = ptr[a] + j
                term = self.term_id[q]
                c = self.term_ct[q]
                A = nd[a] + al
                B = self.T[term] + beta[term][:, np.newaxis]
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    w = np.where(real, A * B / den, 0.0)
                total = _wave_scan(_lane_sums(w.reshape(len(a), WAVE, S)))[:, WAVE - 1]
                moves = ((total > 0.0) & np.isfinite(total))[:, np.newaxis]
                with np.errstate(divide="ignore", invalid="ignore"):
                    gn = w / total[:, np.newaxis]
                qm = power[q][:, np.newaxis]
                with np.errstate(invalid="ignore", over="ignore"):
                    new = (qm * nd[a]) + (((1.0 - qm) * Cj[a]) * gn)
                    nd[a] = np.where(moves, new, nd[a])
                    if p == last:
                        delta[place[q]] = np.where(moves, c.astype(np.float64)[:, np.newaxis] * gn, 0.0)
        self.n_dk[docs] = nd
        chg = _lane_sums(np.abs(nd - old).reshape(n, WAVE, S))
        self.doc_change[docs] = _wave_scan(chg)[:, WAVE - 1] if n else 0.0
        return delta

    def _blend(self, postings, delta, keep, gain):
        """T[w] = (keep * T[w]) + (gain * s[w]) over every word, s[w] the sequential sum from 0.0 of the partial rows of the
        word's segments in this block (0.0 for a word without postings in it)."""
        sums = _ZeroTable(self)
        Cvb0Chain._apply(sums, postings, delta)
        np.multiply(self.T, keep, out=self.T)
        words = np.unique(self.term_id[postings])           # (elsewhere the sum is 0.0, and x + 0.0 is x: T is never negative)
        self.T[words] = self.T[words] + (gain * sums.T[words])
        sums.clear(words)

    def _block(self, batches, block):
        key = int(batches)
        if key not in self._rounds:
            rounds = block_rounds(self.doc_ptr, self.term_id, batches, self.first_document)
            place = np.zeros(self.nnz, dtype=np.int64)
            for _, _, postings in rounds:
                place[postings] = np.arange(len(postings))
            self._rounds = {key: ({b: (docs, postings) for b, docs, postings in rounds}, place)}
        by_block, place = self._rounds[key]
        docs, postings = by_block.get(block, (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)))
        return docs, postings, place

    def step(self, alpha, beta, batches, burn_in=1, tau0=10.0, kappa=0.9, theta_tau0=10.0, theta_kappa=0.9):
        """Step self.t on block self.t mod batches.  A block without tokens changes nothing; the counter still advances."""
        t = self.t
        self.t += 1
        docs, postings, place = self._block(batches, t % batches)
        if len(postings) == 0:
            return
        K = self.K
        al = np.zeros(self.KP)
        al[:K] = alpha
        beta = np.zeros(self.V) + beta
        beta_sum = float(np.sum(beta))
        block_tokens = int(np.sum(self.term_ct[postings]))
        keep, gain, _, one_minus = step_parameters(t, batches, burn_in, tau0, kappa, theta_tau0, theta_kappa, self.tokens, block_tokens)
        delta = self._update(docs, al, beta, beta_sum, one_minus, place, len(postings))
        self._blend(postings, delta, keep, gain)
        self.recompute_n_k()

    def epoch(self, alpha, beta, batches, **schedule):
        for _ in range(int(batches)):
            self.step(alpha, beta, batches, **schedule)


def textbook_step(doc_ptr, term_id, term_ct, n_kv, n_k, n_dk, alpha, beta, t, batches, burn_in, tau0, kappa, theta_tau0, theta_kappa,
                  first_document=0):
    """Step t of SCVB0 straight from the formulas, in place on lists: n_kv[k][w], n_k[k], n_dk[d][k].  gamma_k ~
    (N_dk + alpha_k) (N_kw + beta_w) / (N_k + beta_sum); N_d <- (1 - rho) ** c N_d + (1 - (1 - rho) ** c) C_j gamma for
    every pass; N_kw <- (1 - rho_phi) N_kw + rho_phi (C / C_M) sum over the block's slots of w of c gamma; N_k its sum."""
    K, V, D = len(n_k), len(beta), len(doc_ptr) - 1
    beta_sum = sum(beta)
    block, epoch = t % batches, t // batches
    docs = [d for d in range(D) if (first_document + d) % batches == block]
    C = float(sum(int(c) for c in term_ct))
    C_M = float(sum(int(term_ct[q]) for d in docs for q in range(int(doc_ptr[d]), int(doc_ptr[d + 1]))))
    if C_M == 0.0:
        return
    rho_phi = (tau0 + t) ** (-kappa)
    hat = [[0.0] * V for _ in range(K)]
    for d in docs:
        slots = range(int(doc_ptr[d]), int(doc_ptr[d + 1]))
        Cj = float(sum(int(term_ct[q]) for q in slots))
        for p in range(burn_in + 1):
            rho = (theta_tau0 + (epoch * (burn_in + 1) + p)) ** (-theta_kappa)
            for q in slots:
                w, c = int(term_id[q]), int(term_ct[q])
                weight = [(n_dk[d][k] + alpha[k]) * (n_kv[k][w] + beta[w]) / (n_k[k] + beta_sum) for k in range(K)]
                total = sum(weight)
                gamma = [x / total for x in weight]
                stay = (1.0 - rho) ** c
                for k in range(K):
                    n_dk[d][k] = stay * n_dk[d][k] + (1.0 - stay) * Cj * gamma[k]
                    if p == burn_in:
                        hat[k][w] += c * gamma[k]
    for k in range(K):
        for w in range(V):
            n_kv[k][w] = (1.0 - rho_phi) * n_kv[k][w] + rho_phi * (C / C_M) * hat[k][w]
        n_k[k] = sum(n_kv[k])

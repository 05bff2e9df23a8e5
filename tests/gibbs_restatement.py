"""The collapsed Gibbs engine in numpy: the specification the HIP sampler (pylda_amd/csrc/estep_gibbs.h) is compared against.

Document-parallel collapsed Gibbs with block-synchronous counts.  The documents whose global index
is g modulo `blocks` form block g; a sweep is `blocks` rounds.  In a round the word-topic table T and n_k stay at their
values of the round's start and every document of the block adds its own changes of the round on top: its n_dk is live,
n_k as it sees it is n_k + (n_dk - n_dk at the start of the round), and the row of the term it is on is T[w] + dw, dw the
moves of the copies of this term it has already visited (a term's copies are back to back).  After the round T and n_k are
brought up to date from the tokens that changed topic.  Same Philox stream, token order, lane layout and fp64 operation
sequence as the kernel, so every token's topic agrees; vectorised over the documents of a round, which do not see each
other by construction.

`replicas` > 1 runs that many independent chains of the same corpus side by side (replica r: seed + r, tables of its
own), for the tests that need the distribution of a chain rather than one path.  Pure host code."""
import numpy as np
import scipy.special

from hybrid_restatement import WAVE, _lane_sums, _wave_scan, hybrid_bits, hybrid_slots, philox4x32_10

PHASE_DRAW = 1 << 16


class GibbsChain(object):
    def __init__(self, doc_ptr, term_id, term_ct, K, V, seed, first_document=0, replicas=1, remove_own=True):
        doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
        term_id = np.asarray(term_id, dtype=np.int64)
        term_ct = np.asarray(term_ct, dtype=np.int64)
        self.K, self.V, self.R = int(K), int(V), int(replicas)
        self.S = hybrid_slots(self.K)
        self.KP = WAVE * self.S
        self.bits = hybrid_bits(self.K)
        self.remove_own = remove_own            # (False: a deliberately wrong chain, for the tests' own control)
        D1 = len(doc_ptr) - 1
        self.D1, self.D = D1, D1 * self.R
        tok_off = np.concatenate([[0], np.cumsum(term_ct)])
        term_doc = np.repeat(np.arange(D1), np.diff(doc_ptr))
        tok_term = np.repeat(term_id, term_ct)                       # grouped order: a term's copies back to back
        tok_first = np.zeros(len(tok_term), dtype=bool)
        tok_first[tok_off[:-1]] = True
        n1 = len(tok_term)
        self.N1 = n1
        self.tok_doc1 = np.repeat(term_doc, term_ct)
        rep = np.arange(self.R)
        # replicas one after the other; replica r's terms are r V + v (tables of its own)
        self.tok_term = (tok_term[np.newaxis, :] + rep[:, np.newaxis] * self.V).ravel()
        self.tok_first = np.tile(tok_first, self.R)
        doc_tok0 = tok_off[doc_ptr[:-1]]
        self.doc_tok0 = (doc_tok0[np.newaxis, :] + rep[:, np.newaxis] * n1).ravel()
        self.ntok = np.tile(tok_off[doc_ptr[1:]] - doc_tok0, self.R)
        self.gdoc = np.tile(first_document + np.arange(D1), self.R).astype(np.uint64)
        self.doc_rep = np.repeat(rep, D1)
        seed = int(seed)
        doc_seed = [(seed + int(r)) & (2 ** 64 - 1) for r in self.doc_rep]
        self.seed_lo = np.array([x & 0xFFFFFFFF for x in doc_seed], dtype=np.uint64)
        self.seed_hi = np.array([x >> 32 for x in doc_seed], dtype=np.uint64)
        self.z = np.zeros(n1 * self.R, dtype=np.int64)
        self.n_dk = np.zeros((self.D, self.K), dtype=np.int64)
        self.T = np.zeros((self.V * self.R, self.K), dtype=np.int64)        # word-major
        self.n_k = np.zeros((self.R, self.K), dtype=np.int64)

    def _uniform(self, pos, phase_index, docs, stream):
        """One [0, 1) double per document of `docs` (each replica under its own seed)."""
        x0, x1, _, _ = philox4x32_10(np.uint64(pos), np.uint64(phase_index), self.gdoc[docs], np.uint64(stream),
                                     self.seed_lo[docs], self.seed_hi[docs])
        return ((x0 | (x1 << np.uint64(32))) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53

    def init(self):
        """Every token's topic = floor(u K), u the block (position, phase 0 / index 0, global document, stream 0)."""
        self.z[:] = 0
        for pos in range(int(self.ntok.max()) if self.D else 0):
            docs = np.nonzero(self.ntok > pos)[0]
            u = self._uniform(pos, 0, docs, 0)
            self.z[self.doc_tok0[docs] + pos] = np.minimum((u * self.K).astype(np.int64), self.K - 1)
        self.recount()

    def recount(self):
        """The three count tables from the tokens' topics."""
        tok_doc = (self.tok_doc1[np.newaxis, :] + np.arange(self.R)[:, np.newaxis] * self.D1).ravel()
        self.n_dk[:] = 0
        self.T[:] = 0
        np.add.at(self.n_dk, (tok_doc, self.z), 1)
        np.add.at(self.T, (self.tok_term, self.z), 1)
        self.n_k = self.T.reshape(self.R, self.V, self.K).sum(axis=1)

    def round(self, alpha, beta, beta_sum, blocks, g, stream):
        docs = np.nonzero(self.gdoc % np.uint64(blocks) == np.uint64(g))[0]
        if len(docs) == 0:
            return
        K, KP, S = self.K, self.KP, self.S
        n = len(docs)
        rows = np.arange(n)
        al = np.asarray(alpha, dtype=np.float64)
        beta_tok = np.tile(np.asarray(beta, dtype=np.float64), self.R)
        nd = self.n_dk[docs].copy()
        nd0 = nd.copy()
        nk = self.n_k[self.doc_rep[docs]]
        dw = np.zeros((n, K), dtype=np.int64)
        ntok, tok0 = self.ntok[docs], self.doc_tok0[docs]
        moved_tok, moved_old, moved_new = [], [], []
        for pos in range(int(ntok.max())):
            a = np.nonzero(ntok > pos)[0]
            tok = tok0[a] + pos
            term = self.tok_term[tok]
            dw[a[self.tok_first[tok]]] = 0
            zo = self.z[tok]
            if self.remove_own:
                nd[a, zo] -= 1
                dw[a, zo] -= 1
            m = self.T[term] + dw[a]
            s = nk[a] + (nd[a] - nd0[a])
            w = np.zeros((len(a), KP))
            w[:, :K] = (nd[a] + al[np.newaxis, :]) * (m + beta_tok[term][:, np.newaxis]) / (s + beta_sum)
            w = w.reshape(len(a), WAVE, S)
            part = _lane_sums(w)
            incl = _wave_scan(part)
            total = incl[:, WAVE - 1]
            t = self._uniform(pos, PHASE_DRAW, docs[a], stream) * total
            over = (incl > t[:, np.newaxis]) & (part > 0.0)        # (a lane without weight never owns the draw)
            has = over.any(axis=1)
            lane = np.argmax(over, axis=1)
            ra = rows[:len(a)]
            excl = np.where(lane > 0, incl[ra, np.maximum(lane - 1, 0)], 0.0)
            wl = w[ra, lane]
            run = excl.copy()
            slot = np.full(len(a), -1)
            last = np.full(len(a), -1)
            for sl in range(S):
                run = run + wl[:, sl]
                slot = np.where((slot < 0) & (run > t), sl, slot)
                last = np.where(wl[:, sl] > 0.0, sl, last)
            slot = np.where(slot < 0, last, slot)
            if not has.all():                                      # no lane exceeds t: the last topic with weight
                positive = part > 0.0
                lane_nz = np.where(positive.any(axis=1), WAVE - 1 - np.argmax(positive[:, ::-1], axis=1), 0)
                wl2 = w[ra, lane_nz]
                last2 = np.zeros(len(a), dtype=np.int64)
                for sl in range(S):
                    last2 = np.where(wl2[:, sl] > 0.0, sl, last2)
                lane = np.where(has, lane, lane_nz)
                slot = np.where(has, slot, last2)
            zn = lane * S + slot
            nd[a, zn] += 1
            dw[a, zn] += 1
            self.z[tok] = zn
            ch = zn != zo
            moved_tok.append(term[ch])
            moved_old.append(zo[ch])
            moved_new.append(zn[ch])
            if not self.remove_own:
                # the control chain keeps its books consistent: the token does leave its old topic, after the draw
                nd[a, zo] -= 1
                dw[a, zo] -= 1
        # apply: T and n_k from the tokens that changed topic (integers: the order does not matter)
        term, zo, zn = np.concatenate(moved_tok), np.concatenate(moved_old), np.concatenate(moved_new)
        np.add.at(self.T, (term, zo), -1)
        np.add.at(self.T, (term, zn), 1)
        rep = term // self.V
        np.add.at(self.n_k, (rep, zo), -1)
        np.add.at(self.n_k, (rep, zn), 1)
        self.n_dk[docs] = nd

    def sweep(self, alpha, beta, blocks, stream):
        alpha = np.zeros(self.K) + alpha
        beta = np.zeros(self.V) + beta
        beta_sum = float(np.sum(beta))
        for g in range(blocks):
            self.round(alpha, beta, beta_sum, blocks, g, stream)

    # ---- views of one replica ----
    def n_kv(self, r=0):
        return self.T[r * self.V:(r + 1) * self.V].T.copy()

    def n_dk_of(self, r=0):
        return self.n_dk[r * self.D1:(r + 1) * self.D1]

    def topics(self, r=0):
        return self.z[r * self.N1:(r + 1) * self.N1]

    def log_posterior(self, alpha, beta, r=0):
        return log_posterior(self.n_dk_of(r), self.n_kv(r), np.zeros(self.K) + alpha, np.zeros(self.V) + beta)


def log_posterior(n_dk, n_kv, alpha, beta):
    """monte_carlo.py:217-256 of the reference on count tables (n_k = the rows' sums of n_kv)."""
    gl = scipy.special.gammaln
    D, K = n_dk.shape
    alpha_sum, beta_sum = np.sum(alpha), np.sum(beta)
    ll = 0.0
    ll += gl(np.sum(alpha)) * D
    ll -= np.sum(gl(alpha)) * D
    for d in range(D):
        ll += np.sum(gl(n_dk[d, :] + alpha))
        ll -= gl(np.sum(n_dk[d, :]) + alpha_sum)
    ll += gl(np.sum(beta)) * K
    ll -= np.sum(gl(beta)) * K
    n_k = n_kv.sum(axis=1)
    for k in range(K):
        ll += np.sum(gl(n_kv[k, :] + beta))
        ll -= gl(n_k[k] + beta_sum)
    return ll

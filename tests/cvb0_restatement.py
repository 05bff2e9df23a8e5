"""The collapsed variational Bayes engine (CVB0) in numpy: the specification the HIP kernels (pylda_amd/csrc/estep_cvb0.h)
are compared against.

A distinct (document, term) slot q of the CSR carries a row g[q] over the topics, shared by the c_q copies of the term; T
(word-major), n_k and N_dk are expected counts.  The documents whose global index is b modulo `blocks` form block b; a sweep
is a round per block: every document of the block is updated against the T and n_k of the round's start plus its own
changes, then the block's changes go into T through per-word segment sums in a fixed order, and n_k is recomputed from T in
chunks of 1024 words.  Same Philox start, slot order, lane layout and fp64 operation sequence as the kernels, so every
number agrees bit for bit (an update is add, multiply and divide); vectorised over the documents of a round, which do not
see each other by construction.

textbook_sweep() is the same chain written straight from the formula - sequential over the documents, plain sums, none of
the orderings - for the test that guards this file against being wrong the way the kernel is.  Pure host code."""
import numpy as np

from foldin_restatement import fixed_order_total
from hybrid_restatement import WAVE, _lane_sums, _wave_scan, _wave_sum, hybrid_slots, uniform

SEGMENT = 256       # postings of a word in a block per partial sum
CHUNK = 1024        # words per chunk of the n_k sums


def start_rows(doc_ptr, term_ct, K, seed, stream, first_document=0):
    """m (nnz, K) float64: per slot the copies that drew each topic - topic = min(K - 1, (int)(uniform(token position,
    phase 0, global document, stream) * K)), the collapsed Gibbs engine's start."""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    term_ct = np.asarray(term_ct, dtype=np.int64)
    D, nnz = len(doc_ptr) - 1, len(term_ct)
    tok_off = np.concatenate([[0], np.cumsum(term_ct)])
    slot_doc = np.repeat(np.arange(D), np.diff(doc_ptr))
    tok_slot = np.repeat(np.arange(nnz), term_ct)
    tok_doc = slot_doc[tok_slot]
    pos = np.arange(int(tok_off[-1])) - tok_off[doc_ptr[:-1]][tok_doc]
    m = np.zeros((nnz, K))
    if len(pos):
        u = uniform(pos.astype(np.uint64), np.uint64(0), (first_document + tok_doc).astype(np.uint64), stream, seed)
        z = np.minimum((u * K).astype(np.int64), K - 1)
        np.add.at(m, (tok_slot, z), 1.0)
    return m


def block_rounds(doc_ptr, term_id, blocks, first_document=0):
    """The rounds of a sweep, in ascending block: (block, documents, postings) - the block's documents in index order and
    its slots sorted by (word, document)."""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    term_id = np.asarray(term_id, dtype=np.int64)
    D = len(doc_ptr) - 1
    block = (first_document + np.arange(D)) % blocks
    slot_doc = np.repeat(np.arange(D), np.diff(doc_ptr))
    rounds = []
    for b in np.unique(block):
        docs = np.nonzero(block == b)[0]
        slots = np.nonzero(block[slot_doc] == b)[0]
        order = np.lexsort((slot_doc[slots], term_id[slots]))
        rounds.append((int(b), docs, slots[order]))
    return rounds


def _normalise(w, go, S):
    """(moves (n,), gn, df): total = lane 63 of the Hillis-Steele scan of the lanes' sequential slot sums."""
    n = len(w)
    total = _wave_scan(_lane_sums(w.reshape(n, WAVE, S)))[:, WAVE - 1]
    moves = (total > 0.0) & np.isfinite(total)
    with np.errstate(divide="ignore", invalid="ignore"):
        gn = np.where(moves[:, np.newaxis], w / total[:, np.newaxis], go)
    df = np.where(moves[:, np.newaxis], gn - go, 0.0)
    return moves, gn, df


class Cvb0Chain(object):
    def __init__(self, doc_ptr, term_id, term_ct, K, V, first_document=0, remove_own=True):
        self.doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
        self.term_id = np.asarray(term_id, dtype=np.int64)
        self.term_ct = np.asarray(term_ct, dtype=np.int64)
        self.K, self.V, self.first_document = int(K), int(V), int(first_document)
        self.S = hybrid_slots(self.K)
        self.KP = WAVE * self.S
        self.D, self.nnz = len(self.doc_ptr) - 1, len(self.term_id)
        self.remove_own = remove_own            # (False: the own token stays in the counts - a deliberately wrong chain)
        self.nterm = np.diff(self.doc_ptr)
        self.slot_doc = np.repeat(np.arange(self.D), self.nterm)
        self.g = np.zeros((self.nnz, self.KP))
        chunks = (self.V + CHUNK - 1) // CHUNK
        self._chunked = np.zeros((chunks, CHUNK, self.KP))      # T, padded with zero rows up to whole chunks
        self.T = self._chunked.reshape(chunks * CHUNK, self.KP)[:self.V]
        self.n_k = np.zeros(self.KP)
        self.n_dk = np.zeros((self.D, self.KP))
        self.doc_change = np.zeros(self.D)
        self._rounds = {}

    # ---- state ----
    def init(self, seed):
        K = self.K
        m = start_rows(self.doc_ptr, self.term_ct, K, seed, 0, self.first_document)
        self.g[:] = 0.0
        self.g[:, :K] = m / self.term_ct[:, np.newaxis].astype(np.float64)
        self.T[:] = 0.0
        self.n_dk[:] = 0.0
        np.add.at(self.T[:, :K], self.term_id, m)              # integers: exact in any order
        np.add.at(self.n_dk[:, :K], self.slot_doc, m)
        self.doc_change[:] = 0.0
        self.recompute_n_k()

    def recompute_n_k(self):
        """Chunks of 1024 words summed sequentially from 0.0 in word order (cumsum is sequential; 0.0 + x = x), then the
        chunk sums summed sequentially from 0.0."""
        sums = np.cumsum(self._chunked, axis=1)[:, -1, :]           # (x + 0.0 = x: the zero rows change nothing)
        self.n_k = np.cumsum(sums, axis=0)[-1]

    def state(self):
        """(n_kv (K, V), n_k, n_dk, g) as pylda_cvb0_get_state returns them."""
        K = self.K
        return self.T[:, :K].T.copy(), self.n_k[:K].copy(), self.n_dk[:, :K].copy(), self.g[:, :K].copy()

    # ---- a sweep ----
    def _update(self, docs, al, beta, beta_sum, place, rows):
        """The block's documents against the frozen T and n_k; returns delta (`rows` rows: a slot's is place[slot])."""
        K, KP, S = self.K, self.KP, self.S
        n = len(docs)
        nd = self.n_dk[docs].copy()
        nks = np.tile(self.n_k, (n, 1))
        chg = np.zeros((n, WAVE))
        delta = np.zeros((rows, KP))
        nterm, ptr = self.nterm[docs], self.doc_ptr[docs]
        real = np.arange(KP) < K
        own = 1.0 if self.remove_own else 0.0
        for j in range(int(nterm.max()) if n else 0):
            a = np.nonzero(nterm > j)[0]
            q = ptr[a] + j
            go = self.g[q]
            gx = go * own
            term = self.term_id[q]
            c = self.term_ct[q].astype(np.float64)[:, np.newaxis]
            A = (nd[a] - gx) + al
            B = (self.T[term] - gx) + beta[term][:, np.newaxis]
            N = (nks[a] - gx) + beta_sum
            with np.errstate(divide="ignore", invalid="ignore"):
                w = np.where(real, A * B / N, 0.0)
            _, gn, df = _normalise(w, go, S)
            dl = c * df
            nd[a] = nd[a] + dl
            nks[a] = nks[a] + dl
            self.g[q] = gn
            delta[place[q]] = dl
            inc = (c * np.abs(df)).reshape(len(a), WAVE, S)
            acc = chg[a]
            for s in range(S):
                acc = acc + inc[:, :, s]
            chg[a] = acc
        self.n_dk[docs] = nd
        self.doc_change[docs] = _wave_scan(chg)[:, WAVE - 1] if n else 0.0
        return delta

    def _apply(self, postings, delta):
        """T[w] = ((T[w] + partial_0) + partial_1) + .., partial_i the sequential sum from 0.0 of the deltas of the word's
        i-th segment of 256 postings (document order).  delta: a row per posting, in posting order."""
        if len(postings) == 0:
            return
        term = self.term_id[postings]
        first = np.concatenate([[True], term[1:] != term[:-1]])
        run_start = np.nonzero(first)[0]
        run_of = np.cumsum(first) - 1
        rank = np.arange(len(postings)) - run_start[run_of]          # position within the word's run
        seg_in_run, rank_in_seg = rank // SEGMENT, rank % SEGMENT
        seg_first = rank_in_seg == 0
        seg_of = np.cumsum(seg_first) - 1
        nseg = int(seg_of[-1]) + 1
        partial = np.zeros((nseg, self.KP))
        for r in range(int(rank_in_seg.max()) + 1):
            at = np.nonzero(rank_in_seg == r)[0]
            partial[seg_of[at]] = partial[seg_of[at]] + delta[at]
        seg_word, seg_ord = term[seg_first], seg_in_run[seg_first]
        for i in range(int(seg_ord.max()) + 1):
            at = np.nonzero(seg_ord == i)[0]
            self.T[seg_word[at]] = self.T[seg_word[at]] + partial[at]

    def sweep(self, alpha, beta, blocks):
        K = self.K
        al = np.zeros(self.KP)
        al[:K] = alpha
        beta = np.zeros(self.V) + beta
        beta_sum = float(np.sum(beta))
        key = int(blocks)
        if key not in self._rounds:
            rounds = block_rounds(self.doc_ptr, self.term_id, blocks, self.first_document)
            place = np.zeros(self.nnz, dtype=np.int64)          # a slot's place among its round's postings
            for _, _, postings in rounds:
                place[postings] = np.arange(len(postings))
            self._rounds = {key: (rounds, place)}
        rounds, place = self._rounds[key]
        for _, docs, postings in rounds:
            delta = self._update(docs, al, beta, beta_sum, place, len(postings))
            if len(postings):
                self._apply(postings, delta)
                self.recompute_n_k()

    # ---- the training plug-in likelihood ----
    def log_likelihood(self, alpha, beta):
        """(total, per document, the last sweep's total change) - the scoring form of the fold-in."""
        K, KP, S, D = self.K, self.KP, self.S, self.D
        al = np.zeros(KP)
        al[:K] = alpha
        beta = np.zeros(self.V) + beta
        beta_sum = float(np.sum(beta))
        real = np.arange(KP) < K
        th = np.where(real, self.n_dk + al, 0.0)
        gsum = _wave_sum(_lane_sums(th.reshape(D, WAVE, S))) if D else np.zeros(0)
        theta = th / gsum[:, np.newaxis]
        den = np.where(real, self.n_k + beta_sum, 1.0)
        doc_ll = np.zeros(D)
        for j in range(int(self.nterm.max()) if D else 0):
            a = np.nonzero(self.nterm > j)[0]
            q = self.doc_ptr[a] + j
            term = self.term_id[q]
            row = np.where(real, (self.T[term] + beta[term][:, np.newaxis]) / den, 0.0)
            x = _wave_sum(_lane_sums((theta[a] * row).reshape(len(a), WAVE, S)))
            doc_ll[a] = doc_ll[a] + self.term_ct[q].astype(np.float64) * np.log(x)
        return fixed_order_total(doc_ll), doc_ll, fixed_order_total(self.doc_change)


def textbook_sweep(doc_ptr, term_id, term_ct, n_kv, n_k, n_dk, g, alpha, beta):
    """One sweep of sequential CVB0 straight from the formula, in place: for every document and every slot of it,
    gamma_k ~ (N_dk - g + alpha_k) (N_kw - g + beta_w) / (N_k - g + beta_sum), the c copies of the slot moved together."""
    K = len(n_k)
    beta_sum = sum(beta)
    for d in range(len(doc_ptr) - 1):
        for q in range(int(doc_ptr[d]), int(doc_ptr[d + 1])):
            w, c = int(term_id[q]), float(term_ct[q])
            weight = [(n_dk[d][k] - g[q][k] + alpha[k]) * (n_kv[k][w] - g[q][k] + beta[w]) / (n_k[k] - g[q][k] + beta_sum)
                      for k in range(K)]
            total = sum(weight)
            for k in range(K):
                new = weight[k] / total
                change = c * (new - g[q][k])
                n_dk[d][k] += change
                n_kv[k][w] += change
                n_k[k] += change
                g[q][k] = new


def predictive_table(n_kv, beta):
    """P (V, K) as pylda_set_eta(n_kv + beta) and pylda_completion_set_model build it: eta[k][w] / sum_v eta[k][v], the row
    sum in the device's fixed order (thread t of 256 takes v = t, t + 256, .., then the wavefronts' sums)."""
    eta = np.asarray(n_kv, dtype=np.float64) + (np.zeros(np.shape(n_kv)[1]) + beta)[np.newaxis, :]
    return (eta / np.array([fixed_order_total(row) for row in eta])[:, np.newaxis]).T.copy()


def fold_in(doc_ptr, term_id, term_ct, P, alpha, seed, stream, sweeps, first_document=0):
    """Held-out fold-in against the frozen predictive table P (V, K).  Returns a dict: gamma (D, K), doc_words_ll (D,),
    words_log_likelihood."""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    term_id = np.asarray(term_id, dtype=np.int64)
    term_ct = np.asarray(term_ct, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    V, K = P.shape
    D = len(doc_ptr) - 1
    S = hybrid_slots(K)
    KP = WAVE * S
    al = np.zeros(KP)
    al[:K] = alpha
    Pp = np.zeros((V, KP))
    Pp[:, :K] = P
    real = np.arange(KP) < K
    nterm = np.diff(doc_ptr)
    slot_doc = np.repeat(np.arange(D), nterm)
    m = start_rows(doc_ptr, term_ct, K, seed, stream, first_document)
    g = np.zeros((len(term_id), KP))
    g[:, :K] = m / term_ct[:, np.newaxis].astype(np.float64)
    nd = np.zeros((D, KP))
    # (the kernel adds a document's slots one after the other; the sums are of small integers, exact in any order)
    np.add.at(nd[:, :K], slot_doc, m)
    maxn = int(nterm.max()) if D else 0
    for _ in range(sweeps):
        for j in range(maxn):
            a = np.nonzero(nterm > j)[0]
            q = doc_ptr[a] + j
            go = g[q]
            c = term_ct[q].astype(np.float64)[:, np.newaxis]
            w = np.where(real, ((nd[a] - go) + al) * Pp[term_id[q]], 0.0)
            _, gn, df = _normalise(w, go, S)
            nd[a] = nd[a] + c * df
            g[q] = gn
    gam = np.where(real, al + nd, 0.0)
    gsum = _wave_sum(_lane_sums(gam.reshape(D, WAVE, S))) if D else np.zeros(0)
    theta = gam / gsum[:, np.newaxis]
    doc_ll = np.zeros(D)
    for j in range(maxn):
        a = np.nonzero(nterm > j)[0]
        q = doc_ptr[a] + j
        x = _wave_sum(_lane_sums((theta[a] * Pp[term_id[q]]).reshape(len(a), WAVE, S)))
        doc_ll[a] = doc_ll[a] + term_ct[q].astype(np.float64) * np.log(x)
    return {"gamma": gam[:, :K], "doc_words_ll": doc_ll, "words_log_likelihood": fixed_order_total(doc_ll)}

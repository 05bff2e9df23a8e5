"""The hybrid E-step in numpy: the specification the HIP sampler (pylda_amd/csrc/estep_hybrid.h) is compared against.

Same Philox4x32-10 stream, token order, sampling rule and fp64 operation sequence as the kernel ("Hybrid
E-step"), vectorised over documents (all documents step through their token positions together).  Topic k lives in
lane k // S, slot k % S of a 64-lane wavefront, S = hybrid_slots(K); the lane sums, the wavefront sum and the lane scan
are written out in the order the kernel computes them.  Pure host code: it runs without a GPU."""
import numpy as np
import scipy.special

MASK32 = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
WAVE = 64


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (broadcast) of 32-bit words; returns the four output words as uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK32 for x in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    for r in range(10):
        if r:
            k0 = (k0 + _W0) & MASK32
            k1 = (k1 + _W1) & MASK32
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
    return c0, c1, c2, c3


def uniform(pos, phase_index, doc, stream, seed):
    """[0, 1) double of the block named by (token position, phase << 16 | index, global document, stream; seed)."""
    seed = int(seed) & (2 ** 64 - 1)
    x0, x1, _, _ = philox4x32_10(pos, phase_index, doc, stream, seed & 0xFFFFFFFF, seed >> 32)
    u = x0 | (x1 << np.uint64(32))
    return (u >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def hybrid_slots(K):
    return 1 if K <= 64 else 2 if K <= 128 else 4 if K <= 256 else 8 if K <= 512 else 16


def hybrid_bits(K):
    b = 1
    while (1 << b) < K:
        b += 1
    return b


def shifted_table(eta):
    """B[w][k] = exp(E_log_eta[k][w] - max_k E_log_eta[k][w]) and the unnormalised E_log_eta (K, V)."""
    elog = scipy.special.psi(eta) - scipy.special.psi(np.sum(eta, axis=1))[:, np.newaxis]
    return np.exp(elog - elog.max(axis=0)[np.newaxis, :]).T, elog


def _lane_sums(x):
    """(n, 64, S) -> (n, 64): each lane's slots summed in slot order."""
    acc = x[:, :, 0].copy()
    for s in range(1, x.shape[2]):
        acc = acc + x[:, :, s]
    return acc


def _wave_sum(part):
    """(n, 64) -> (n,): pairwise by lane index (xor 1, 2, 4, .., 32), the order of the kernel's wave_sum."""
    while part.shape[1] > 1:
        part = part[:, 0::2] + part[:, 1::2]
    return part[:, 0]


def _wave_scan(part):
    """(n, 64) -> (n, 64): inclusive Hillis-Steele scan, distances 1, 2, .., 32."""
    x = part.copy()
    d = 1
    while d < WAVE:
        x[:, d:] = x[:, d:] + x[:, :-d]
        d *= 2
    return x


def hybrid_estep(doc_ptr, term_id, term_ct, alpha, eta, seed, stream=0, first_document=0, number_of_samples=10,
                 burn_in_samples=5, heldout=False):
    """One hybrid E-step over a CSR corpus.  Returns a dict: gamma (D, K), doc_ll (D,), doc_words_ll (D,),
    document_log_likelihood, words_log_likelihood, counts (K, V) raw post-burn-in counts, sstats = counts / m,
    history (tokens, m) post-burn-in topics per token (grouped order), min_gap (D,) the smallest distance of a draw's
    t to a cumulative weight, relative to the draw's total (where a rounding difference could move a draw)."""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    term_id = np.asarray(term_id, dtype=np.int64)
    term_ct = np.asarray(term_ct, dtype=np.int64)
    alpha = np.asarray(alpha, dtype=np.float64)
    eta = np.asarray(eta, dtype=np.float64)
    K, V = eta.shape
    D = len(doc_ptr) - 1
    S = hybrid_slots(K)
    KP = WAVE * S
    m = number_of_samples - burn_in_samples
    B, elog = shifted_table(eta)
    Bp = np.zeros((V, KP))
    Bp[:, :K] = B
    al = np.zeros(KP)
    al[:K] = alpha

    # tokens in grouped order: the c_n copies of a term back to back, terms in CSR order
    tok_term = np.repeat(term_id, term_ct)
    tok_doc = np.repeat(np.repeat(np.arange(D), np.diff(doc_ptr)), term_ct)
    tok_off = np.concatenate([[0], np.cumsum(term_ct)])
    doc_tok0 = tok_off[doc_ptr[:-1]]
    ntok = tok_off[doc_ptr[1:]] - doc_tok0
    maxn = int(ntok.max()) if D else 0
    gdoc = (first_document + np.arange(D)).astype(np.uint64)
    kk = np.arange(KP, dtype=np.uint64)
    real = (np.arange(KP) < K)

    def start_column(idx, pos):
        r = uniform(np.uint64(pos), kk[np.newaxis, :], gdoc[idx][:, np.newaxis], stream, seed)
        r = np.where(real[np.newaxis, :], r, 0.0).reshape(len(idx), WAVE, S)
        colsum = _wave_sum(_lane_sums(r))
        return (r / colsum[:, np.newaxis, np.newaxis]).reshape(len(idx), KP)

    ps = np.zeros((D, KP))
    for pos in range(maxn):
        idx = np.nonzero(ntok > pos)[0]
        ps[idx] = ps[idx] + start_column(idx, pos)

    z_cur = np.zeros(int(tok_off[-1]), dtype=np.int64)
    history = np.zeros((int(tok_off[-1]), m), dtype=np.int64)
    min_gap = np.full(D, np.inf)
    for it in range(number_of_samples):
        for pos in range(maxn):
            idx = np.nonzero(ntok > pos)[0]
            tok = doc_tok0[idx] + pos
            if it == 0:
                v = ps[idx] - start_column(idx, pos)
                ps[idx] = np.where(v > 0.0, v, 0.0)
            else:
                zo = z_cur[tok]
                v = ps[idx, zo] - 1.0
                ps[idx, zo] = np.where(v > 0.0, v, 0.0)
            w = ((ps[idx] + al[np.newaxis, :]) * Bp[tok_term[tok]]).reshape(len(idx), WAVE, S)
            part = _lane_sums(w)
            incl = _wave_scan(part)
            total = incl[:, WAVE - 1]
            t = uniform(np.uint64(pos), np.uint64((1 + it) << 16), gdoc[idx], stream, seed) * total
            over = (incl > t[:, np.newaxis]) & (part > 0.0)      # (a lane without weight never owns the draw)
            has = over.any(axis=1)
            lane = np.argmax(over, axis=1)
            excl = np.where(lane > 0, incl[np.arange(len(idx)), np.maximum(lane - 1, 0)], 0.0)
            wl = w[np.arange(len(idx)), lane]                       # (n, S) the owner lane's weights
            run = excl.copy()
            slot = np.full(len(idx), -1)
            last = np.full(len(idx), -1)
            for s in range(S):
                run = run + wl[:, s]
                slot = np.where((slot < 0) & (run > t), s, slot)
                last = np.where(wl[:, s] > 0.0, s, last)
            slot = np.where(slot < 0, last, slot)
            if not has.all():                                      # no lane exceeds t: the last non-zero topic
                positive = part > 0.0
                lane_nz = np.where(positive.any(axis=1), WAVE - 1 - np.argmax(positive[:, ::-1], axis=1), 0)
                wl2 = w[np.arange(len(idx)), lane_nz]
                last2 = np.zeros(len(idx), dtype=np.int64)          # (no weight at all: topic 0)
                for s in range(S):
                    last2 = np.where(wl2[:, s] > 0.0, s, last2)
                lane = np.where(has, lane, lane_nz)
                slot = np.where(has, slot, last2)
            znew = lane * S + slot
            ps[idx, znew] = ps[idx, znew] + 1.0
            z_cur[tok] = znew
            if it >= burn_in_samples:
                history[tok, it - burn_in_samples] = znew
            cum = np.cumsum(w.reshape(len(idx), KP), axis=1)
            gap = np.min(np.abs(cum - t[:, np.newaxis]), axis=1) / total
            min_gap[idx] = np.minimum(min_gap[idx], gap)

    gamma = al[np.newaxis, :K] + ps[:, :K]
    alpha_term = scipy.special.gammaln(np.sum(alpha)) - np.sum(scipy.special.gammaln(alpha))
    same = history[:, :, np.newaxis] == history[:, np.newaxis, :]
    cnt = same.sum(axis=2)                                          # (tokens, m): count of each sample's topic
    f = cnt / float(m)
    ent_tok = np.sum(f * np.log(f) / cnt, axis=1) + (K - np.sum(1.0 / cnt, axis=1)) * (1e-100 * np.log(1e-100))
    ent = np.bincount(tok_doc, weights=ent_tok, minlength=D)
    doc_ll = alpha_term + np.sum(scipy.special.gammaln(gamma), axis=1) - scipy.special.gammaln(np.sum(gamma, axis=1)) - ent
    if heldout:
        wtok = np.sum(f * elog[history, tok_term[:, np.newaxis]] / cnt, axis=1)
        doc_wll = np.bincount(tok_doc, weights=wtok, minlength=D)
    else:
        doc_wll = np.zeros(D)
    counts = np.zeros((K, V))
    np.add.at(counts, (history.ravel(), np.repeat(tok_term, m)), 1.0)
    return {"gamma": gamma, "doc_ll": doc_ll, "doc_words_ll": doc_wll, "document_log_likelihood": float(np.sum(doc_ll)),
            "words_log_likelihood": float(np.sum(doc_wll)), "counts": counts, "sstats": counts / float(m),
            "history": history, "min_gap": min_gap, "token_doc": tok_doc, "token_term": tok_term}

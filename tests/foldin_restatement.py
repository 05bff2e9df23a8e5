"""Held-out fold-in for the collapsed Gibbs engine in numpy: the specification the HIP kernels (pylda_amd/csrc/estep_foldin.h)
are compared against.

With the word-topic counts frozen the held-out documents are independent chains.  Per document: a uniformly random topic
per token, `number_of_samples` sweeps with weight ((double)n_dk + alpha_k) * P[w][k], the document's topic counts summed
after every sweep from `burn_in_samples` on, gamma = alpha + the mean kept count, and the plug-in likelihood
sum_n c_n log(sum_k theta_k P[w_n][k]) with theta = gamma / sum(gamma).  Same Philox stream, token order, lane layout and fp64
operation sequence as the kernel, so gamma agrees bit for bit (there is no transcendental in the chain); vectorised over the
documents, which step through their token positions together.  Pure host code."""
import numpy as np

from gibbs_restatement import WAVE, _lane_sums, _wave_scan, hybrid_slots
from hybrid_restatement import _wave_sum, uniform


def predictive_table(n_kv, n_k, beta, beta_sum):
    """P (V, K): ((double)n_kv[k][w] + beta_w) / ((double)n_k[k] + beta_sum) - add, add, divide."""
    n_kv = np.asarray(n_kv, dtype=np.int64)
    K, V = n_kv.shape
    beta = np.zeros(V) + beta
    return (n_kv.T.astype(np.float64) + beta[:, np.newaxis]) / (np.asarray(n_k, dtype=np.int64).astype(np.float64) + beta_sum)[np.newaxis, :]


def fixed_order_total(values):
    """The corpus total as the device sums it: thread t of 256 takes documents t, t + 256, .. in order, then the
    wavefronts' sums (pairwise by lane), then the four wavefronts in order."""
    part = np.zeros(256)
    for at in range(0, len(values), 256):
        chunk = values[at:at + 256]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    total = 0.0
    for wave in _wave_sum(part.reshape(4, WAVE)):
        total = total + wave
    return float(total)


def fold_in(doc_ptr, term_id, term_ct, P, alpha, seed, stream, number_of_samples, burn_in_samples, first_document=0,
            remove_own=True):
    """Returns a dict: gamma (D, K), doc_words_ll (D,), words_log_likelihood, topics (the tokens' last topics, grouped order).
    remove_own=False is a deliberately wrong chain (the token stays in its document's counts while it is drawn), for the
    tests' own control."""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    term_id = np.asarray(term_id, dtype=np.int64)
    term_ct = np.asarray(term_ct, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    V, K = P.shape
    D = len(doc_ptr) - 1
    S = hybrid_slots(K)
    KP = WAVE * S
    kept = number_of_samples - burn_in_samples
    al = np.zeros(KP)
    al[:K] = alpha
    Pp = np.zeros((V, KP))
    Pp[:, :K] = P

    tok_term = np.repeat(term_id, term_ct)                       # grouped order: a term's copies back to back
    tok_off = np.concatenate([[0], np.cumsum(term_ct)])
    doc_tok0 = tok_off[doc_ptr[:-1]]
    ntok = tok_off[doc_ptr[1:]] - doc_tok0
    maxn = int(ntok.max()) if D else 0
    gdoc = (first_document + np.arange(D)).astype(np.uint64)
    rows = np.arange(D)

    z = np.zeros(int(tok_off[-1]), dtype=np.int64)
    nd = np.zeros((D, KP), dtype=np.int64)
    for pos in range(maxn):
        a = np.nonzero(ntok > pos)[0]
        u = uniform(np.uint64(pos), np.uint64(0), gdoc[a], stream, seed)
        start = np.minimum((u * K).astype(np.int64), K - 1)
        z[doc_tok0[a] + pos] = start
        nd[a, start] += 1

    acc = np.zeros((D, KP), dtype=np.int64)
    for it in range(number_of_samples):
        for pos in range(maxn):
            a = np.nonzero(ntok > pos)[0]
            tok = doc_tok0[a] + pos
            zo = z[tok]
            if remove_own:
                nd[a, zo] -= 1
            w = ((nd[a] + al[np.newaxis, :]) * Pp[tok_term[tok]]).reshape(len(a), WAVE, S)
            part = _lane_sums(w)
            incl = _wave_scan(part)
            total = incl[:, WAVE - 1]
            t = uniform(np.uint64(pos), np.uint64((1 + it) << 16), gdoc[a], stream, seed) * total
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
            z[tok] = zn
            if not remove_own:
                nd[a, zo] -= 1          # (the control keeps its books: the token does leave its old topic, after the draw)
        if it >= burn_in_samples:
            acc += nd

    gam = np.zeros((D, KP))
    gam[:, :K] = al[np.newaxis, :K] + acc[:, :K].astype(np.float64) / float(kept)
    gsum = _wave_sum(_lane_sums(gam.reshape(D, WAVE, S))) if D else np.zeros(0)
    theta = gam / gsum[:, np.newaxis]
    doc_ll = np.zeros(D)
    nterm = np.diff(doc_ptr)
    for j in range(int(nterm.max()) if D else 0):
        a = np.nonzero(nterm > j)[0]
        q = doc_ptr[a] + j
        x = _wave_sum(_lane_sums((theta[a] * Pp[term_id[q]]).reshape(len(a), WAVE, S)))
        doc_ll[a] = doc_ll[a] + term_ct[q].astype(np.float64) * np.log(x)
    return {"gamma": gam[:, :K], "doc_words_ll": doc_ll, "words_log_likelihood": fixed_order_total(doc_ll), "topics": z}

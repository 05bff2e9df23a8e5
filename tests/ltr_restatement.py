"""The left-to-right held-out likelihood in numpy: the specification the HIP kernels (pylda_amd/csrc/left_to_right.h) are
compared against (Wallach, Murray, Salakhutdinov & Mimno 2009, Algorithm 3).

Per (document, particle) a chain over the document's tokens - its CSR terms in order, a term's copies back to back.  For
position n in order: if `resample`, the topics of positions 0 .. n - 1 are drawn again one after the other from
((double)nd[k] + alpha[k]) * P[w][k] with the token itself left out; p[n][r] = sum_k of those weights for w_n over
((double)n + alpha_sum); the topic of token n is drawn from the same weights.  The document's estimate is
sum_n log((p[n][0] + .. + p[n][R - 1]) / R).  Same Philox stream - counter [inner position, n, global document, stream + r],
key the seed -, lane layout, slot sums, lane scan, owner rule and fp64 operation sequence as the kernel, so the topics and
the predictive probabilities agree bit for bit (there is no transcendental in the chain); the reduction takes one log per
token.  Vectorised over the chains, which step through their positions together.  Pure host code."""
import numpy as np

from gibbs_restatement import WAVE, _lane_sums, _wave_scan, hybrid_slots
from hybrid_restatement import _wave_sum, uniform


def _draw(w, u):
    """One topic per chain from the weights w (A, 64, S) and the uniforms u (A,): slot sums in slot order, the Hillis-Steele
    lane scan, t = u * total, the first lane with weight whose inclusive sum exceeds t and inside it the first slot whose
    running sum does - the last topic with weight where rounding lets none exceed it (estep_foldin.h)."""
    A, _, S = w.shape
    rows = np.arange(A)
    part = _lane_sums(w)
    incl = _wave_scan(part)
    t = u * incl[:, WAVE - 1]
    over = (incl > t[:, np.newaxis]) & (part > 0.0)
    has = over.any(axis=1)
    positive = part > 0.0
    lane_nz = np.where(positive.any(axis=1), WAVE - 1 - np.argmax(positive[:, ::-1], axis=1), 0)
    lane = np.where(has, np.argmax(over, axis=1), lane_nz)
    excl = np.where(lane > 0, incl[rows, np.maximum(lane - 1, 0)], 0.0)
    wl = w[rows, lane]                                               # (A, S)
    run = np.cumsum(np.concatenate([excl[:, np.newaxis], wl], axis=1), axis=1)[:, 1:]     # ((excl + w_0) + w_1) + ..
    beyond = run > t[:, np.newaxis]
    weighted = wl > 0.0
    last = np.where(weighted.any(axis=1), S - 1 - np.argmax(weighted[:, ::-1], axis=1), 0)
    slot = np.where(has & beyond.any(axis=1), np.argmax(beyond, axis=1), last)
    return lane * S + slot, part


def reduce_documents(p, doc_tok, particles):
    """doc_ll (D,): per document and token m = (p[n][0] + .. + p[n][R - 1]) / R in r order, log m, the wavefront's sum per
    batch of 64 tokens, the batches in order.  Also returns sum_n |log m_n| per document (the tests' bar)."""
    R = int(particles)
    p = np.asarray(p, dtype=np.float64).reshape(-1, R)
    m = p[:, 0].copy()
    for r in range(1, R):
        m = m + p[:, r]
    logs = np.log(m / float(R))
    D = len(doc_tok) - 1
    doc_ll, abs_logs = np.zeros(D), np.zeros(D)
    for d in range(D):
        v = logs[doc_tok[d]:doc_tok[d + 1]]
        abs_logs[d] = np.sum(np.abs(v))
        for at in range(0, len(v), WAVE):
            batch = np.zeros((1, WAVE))
            batch[0, :len(v[at:at + WAVE])] = v[at:at + WAVE]
            doc_ll[d] = doc_ll[d] + _wave_sum(batch)[0]
    return doc_ll, abs_logs


def fixed_order_total(values):
    """The corpus total as the device sums it: thread t of 1024 takes documents t, t + 1024, .. in order, then the
    wavefronts' sums (pairwise by lane), then the sixteen wavefronts in order."""
    part = np.zeros(1024)
    for at in range(0, len(values), 1024):
        chunk = np.asarray(values[at:at + 1024], dtype=np.float64)
        part[:len(chunk)] = part[:len(chunk)] + chunk
    total = 0.0
    for wave in _wave_sum(part.reshape(16, WAVE)):
        total = total + wave
    return float(total)


def left_to_right(doc_ptr, term_id, term_ct, P, alpha, particles, resample, seed, stream, first_document=0, remove_own=True):
    """Returns a dict: z (tokens * R,) the topics in the device's layout (document d's block at its first token * R, as
    (R, N_d)), p (tokens * R,) as (tokens, R), doc_ll (D,), abs_logs (D,), log_likelihood, tokens, doc_tok (D + 1,).
    remove_own=False is a deliberately wrong chain (a token stays in the counts while it is drawn again), for the tests' own
    control."""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    term_id = np.asarray(term_id, dtype=np.int64)
    term_ct = np.asarray(term_ct, dtype=np.int64)
    P = np.asarray(P, dtype=np.float64)
    V, K = P.shape
    D, R = len(doc_ptr) - 1, int(particles)
    S = hybrid_slots(K)
    KP = WAVE * S
    al = np.zeros(KP)
    al[:K] = alpha
    Pp = np.zeros((V, KP))
    Pp[:, :K] = P
    asum = float(_wave_sum(_lane_sums(al.reshape(1, WAVE, S)))[0])

    tok_term = np.repeat(term_id, term_ct)
    tok_off = np.concatenate([[0], np.cumsum(term_ct)]).astype(np.int64)
    doc_tok = tok_off[doc_ptr]
    ntok_d = np.diff(doc_tok)
    maxn = int(ntok_d.max()) if D else 0
    # chain c = d * R + r
    chain_doc = np.repeat(np.arange(D), R)
    chain_r = np.tile(np.arange(R), D)
    gdoc = (first_document + chain_doc).astype(np.uint64)
    strm = (int(stream) + chain_r).astype(np.uint64)
    ntok = ntok_d[chain_doc]
    tok0 = doc_tok[chain_doc]
    C = D * R
    z = np.zeros((C, max(maxn, 1)), dtype=np.int64)
    pred = np.zeros((C, max(maxn, 1)))
    nd = np.zeros((C, KP), dtype=np.int64)

    for n in range(maxn):
        a = np.nonzero(ntok > n)[0]
        A = len(a)
        rows = np.arange(A)
        if resample and n > 0:
            U = uniform(np.arange(n, dtype=np.uint64)[np.newaxis, :], np.uint64(n), gdoc[a][:, np.newaxis], strm[a][:, np.newaxis], seed)
            nda = nd[a]
            for pos in range(n):
                zo = z[a, pos]
                if remove_own:
                    nda[rows, zo] -= 1
                w = ((nda + al[np.newaxis, :]) * Pp[tok_term[tok0[a] + pos]]).reshape(A, WAVE, S)
                zn, _ = _draw(w, U[:, pos])
                nda[rows, zn] += 1
                if not remove_own:
                    nda[rows, zo] -= 1      # (the control keeps its books: the token does leave its old topic, after the draw)
                z[a, pos] = zn
            nd[a] = nda
        w = ((nd[a] + al[np.newaxis, :]) * Pp[tok_term[tok0[a] + n]]).reshape(A, WAVE, S)
        u = uniform(np.uint64(n), np.uint64(n), gdoc[a], strm[a], seed)
        zn, part = _draw(w, u)
        pred[a, n] = _wave_sum(part) / (float(n) + asum)
        nd[a, zn] += 1
        z[a, n] = zn

    tokens = int(doc_tok[-1])
    z_flat = np.zeros(tokens * R, dtype=np.uint16)
    p_flat = np.zeros(tokens * R)
    for d in range(D):
        N = int(ntok_d[d])
        z_flat[doc_tok[d] * R:(doc_tok[d] + N) * R] = z[d * R:(d + 1) * R, :N].reshape(-1)
        p_flat[doc_tok[d] * R:(doc_tok[d] + N) * R] = pred[d * R:(d + 1) * R, :N].T.reshape(-1)
    doc_ll, abs_logs = reduce_documents(p_flat, doc_tok, R)
    return {"z": z_flat, "p": p_flat, "doc_ll": doc_ll, "abs_logs": abs_logs, "log_likelihood": fixed_order_total(doc_ll),
            "tokens": tokens, "doc_tok": doc_tok}


def bar(K, particles, doc_tok, doc_ll, abs_logs):
    """The kernels' distance from left_to_right() per document, the chains being equal draw for draw:
    N_d (K + R + 16) 2^-53 - a positive K-term sum, the R-term mean and a few ulps of divide and log, all relative errors of
    m_n and so absolute errors of log m_n - plus 4 * 2^-53 * sum_n |log m_n| for the two logs' own rounding, plus the
    document's sum of N_d terms, N_d 2^-53 |ll_d|."""
    u = 2.0 ** -53
    n = np.diff(np.asarray(doc_tok)).astype(np.float64)
    return n * (K + particles + 16) * u + 4 * u * np.asarray(abs_logs) + n * u * np.abs(doc_ll)

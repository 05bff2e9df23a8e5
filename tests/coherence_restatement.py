"""Topic coherence restated in numpy, and once more by brute force.

Definitions (the kernels of pylda_amd/csrc/coherence_kernels.h and pylda_amd/coherence.py follow the same):

  top words of topic k   the first M entries of row k of a (K, V) table under "larger value first, among equal values the
                         smaller word id first"
  D, D(v), D(v, v')      documents of the reference corpus (CSR; term counts ignored, empty documents counted), those that
                         contain word v, those that contain both
  UMass of topic k       sum over m = 2..M, l = 1..m-1 of log((D(v_m, v_l) + 1) / D(v_l)), the top words in rank order; a pair
                         whose D(v_l) is 0 contributes 0 and is counted as undefined
  NPMI of topic k        the mean over the same pairs of log(p_ml / (p_m p_l)) / (-log p_ml), p = count / D; -1 where
                         D(v_m, v_l) = 0, 0 where it is D
  M = 1                  0 for both

The numpy form: lexsort for the top words, a boolean presence matrix documents x distinct top words and its product with
itself for the counts, math.fsum for the scores.  The brute-force form: sorted() with a key, Python sets of documents
per word.  Both are exact in everything but the logarithm."""
import math

import numpy as np
import scipy.sparse


def top_words(table, M):
    """(top_ids (K, M) int32, top_values (K, M)): numpy.lexsort((ids, -values)), its first M."""
    table = np.asarray(table, dtype=np.float64)
    K, V = table.shape
    ids = np.empty((K, M), dtype=np.int32)
    for k in range(K):
        ids[k] = np.lexsort((np.arange(V), -table[k]))[:M]
    return ids, np.take_along_axis(table, ids.astype(np.int64), axis=1)


def counts(doc_ptr, term_id, top_ids):
    """(doc_freq (K, M) int64, co_doc_freq (K, M, M) int64) over the corpus' documents."""
    doc_ptr, term_id = np.asarray(doc_ptr, dtype=np.int64), np.asarray(term_id, dtype=np.int64)
    top_ids = np.asarray(top_ids, dtype=np.int64)
    D = len(doc_ptr) - 1
    words, slot = np.unique(top_ids, return_inverse=True)           # the distinct top words and every top word's slot
    slot = slot.reshape(top_ids.shape)
    doc_of = np.repeat(np.arange(D), np.diff(doc_ptr))
    at = np.searchsorted(words, term_id)
    hit = (at < len(words)) & (words[np.minimum(at, len(words) - 1)] == term_id)
    present = np.zeros((D, len(words)), dtype=bool)
    present[doc_of[hit], at[hit]] = True
    X = scipy.sparse.csr_matrix(present, dtype=np.int64)            # (the product of the zeros is skipped, nothing else)
    co = np.asarray((X.T @ X).todense(), dtype=np.int64)            # (U, U): documents that hold both
    co_doc_freq = co[slot[:, :, None], slot[:, None, :]]
    return np.diagonal(co)[slot].copy(), co_doc_freq


def scores(doc_freq, co_doc_freq, documents):
    """(umass (K,), npmi (K,), undefined_pairs (K,) int64) with exact sums."""
    K, M = doc_freq.shape
    umass, npmi, undefined = np.zeros(K), np.zeros(K), np.zeros(K, dtype=np.int64)
    for k in range(K):
        u_terms, n_terms = [], []
        for m in range(1, M):
            for l in range(m):
                both, of_m, of_l = int(co_doc_freq[k, m, l]), int(doc_freq[k, m]), int(doc_freq[k, l])
                if of_l == 0:
                    undefined[k] += 1
                else:
                    u_terms.append(math.log((both + 1.0) / of_l))
                if both == 0:
                    n_terms.append(-1.0)
                elif both == documents:
                    n_terms.append(0.0)
                else:
                    p_ml, p_m, p_l = both / documents, of_m / documents, of_l / documents
                    n_terms.append(math.log(p_ml / (p_m * p_l)) / (-math.log(p_ml)))
        umass[k] = math.fsum(u_terms)
        npmi[k] = math.fsum(n_terms) / len(n_terms) if n_terms else 0.0
    return umass, npmi, undefined


def coherence(table, M, doc_ptr, term_id):
    """Everything topic_coherence() returns, as a dict."""
    ids, values = top_words(table, M)
    doc_freq, co_doc_freq = counts(doc_ptr, term_id, ids)
    documents = len(doc_ptr) - 1
    umass, npmi, undefined = scores(doc_freq, co_doc_freq, documents)
    return {"top_ids": ids, "top_values": values, "doc_freq": doc_freq, "co_doc_freq": co_doc_freq, "umass": umass, "npmi": npmi,
            "undefined_pairs": undefined, "documents": documents, "top_words_count": M,
            "umass_mean": float(np.mean(umass)), "npmi_mean": float(np.mean(npmi))}


# ---- the same by brute force ----
def brute_top_words(table, M):
    return [sorted(range(len(row)), key=lambda v: (-row[v], v))[:M] for row in np.asarray(table, dtype=np.float64).tolist()]


def brute_counts(doc_ptr, term_id, top_ids):
    holders = {}
    for d in range(len(doc_ptr) - 1):
        for w in term_id[doc_ptr[d]:doc_ptr[d + 1]]:
            holders.setdefault(int(w), set()).add(d)
    empty = set()
    doc_freq = [[len(holders.get(int(v), empty)) for v in row] for row in top_ids]
    co = [[[len(holders.get(int(a), empty) & holders.get(int(b), empty)) for b in row] for a in row] for row in top_ids]
    return doc_freq, co


def brute_scores(doc_freq, co, documents):
    out = []
    for df, c in zip(doc_freq, co):
        umass, npmi, pairs, undefined = 0.0, 0.0, 0, 0
        for m in range(1, len(df)):
            for l in range(m):
                pairs += 1
                if df[l] == 0:
                    undefined += 1
                else:
                    umass += math.log((c[m][l] + 1) / df[l])
                if c[m][l] == 0:
                    npmi += -1.0
                elif c[m][l] != documents:
                    npmi += (math.log(c[m][l] * documents / (df[m] * df[l]))) / (-math.log(c[m][l] / documents))
        out.append((umass, npmi / pairs if pairs else 0.0, undefined))
    return out


def random_case(rng, K, V, M, D, max_terms=12, levels=None):
    """A table (continuous, or integer-valued in `levels` plus a constant: ties) and a corpus with empty documents."""
    table = rng.random((K, V)) if levels is None else rng.integers(0, levels, size=(K, V)).astype(np.float64) + 0.5
    lengths = rng.integers(0, min(V, max_terms) + 1, size=D)
    ids = [rng.choice(V, size=n, replace=False) for n in lengths]
    doc_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    term_id = (np.concatenate(ids) if D else np.zeros(0)).astype(np.int32)
    term_ct = rng.integers(1, 5, size=len(term_id)).astype(np.int32)
    return table, doc_ptr, term_id, term_ct

"""The document-completion held-out likelihood in numpy: the specification the HIP kernels (pylda_amd/csrc/completion_score.h)
and pylda_amd.corpus.split_for_completion are compared against.

The split walks every document token by token; the table and the score take every sum with math.fsum, so what they return
is the correctly rounded value of the sums the kernels take in their own fixed orders - the tests' bar is the kernels'
distance from that.  Pure host code."""
import math

import numpy as np


def split(doc_ptr, term_id, term_ct):
    """(observed_csr, held_csr): token position p of a document - its CSR terms in order, a term's copies back to back - is
    observed when p is even, held when p is odd; a term with no copy in a half is left out of it."""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    halves = ([0], [], []), ([0], [], [])
    for d in range(len(doc_ptr) - 1):
        position = 0
        for q in range(int(doc_ptr[d]), int(doc_ptr[d + 1])):
            share = [0, 0]
            for _ in range(int(term_ct[q])):
                share[position & 1] += 1
                position += 1
            for (ptr, ids, cts), copies in zip(halves, share):
                if copies:
                    ids.append(int(term_id[q]))
                    cts.append(copies)
        for ptr, ids, cts in halves:
            ptr.append(len(ids))
    return tuple((np.array(ptr, np.int64), np.array(ids, np.int32), np.array(cts, np.int32)) for ptr, ids, cts in halves)


def predictive_table(eta):
    """P (V, K): eta[k][w] / sum_v eta[k][v], the row sum exact, the division rounded once."""
    eta = np.asarray(eta, dtype=np.float64)
    return (eta / np.array([math.fsum(row.tolist()) for row in eta])[:, np.newaxis]).T.copy()


def score(doc_ptr, term_id, term_ct, P, gamma):
    """Per held document sum_n c_n log(sum_k theta_k P[w_n][k]), theta = gamma / sum(gamma); returns (doc_ll (D,), the
    documents' held tokens (D,), their distinct held terms (D,))."""
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    P, gamma = np.asarray(P, dtype=np.float64), np.asarray(gamma, dtype=np.float64)
    D = len(doc_ptr) - 1
    doc_ll, tokens = np.zeros(D), np.zeros(D, dtype=np.int64)
    for d in range(D):
        theta = gamma[d] / math.fsum(gamma[d].tolist())
        terms = []
        for q in range(int(doc_ptr[d]), int(doc_ptr[d + 1])):
            p = math.fsum((theta * P[int(term_id[q])]).tolist())
            terms.append(float(term_ct[q]) * math.log(p))
            tokens[d] += int(term_ct[q])
        doc_ll[d] = math.fsum(terms)
    return doc_ll, tokens, np.diff(doc_ptr)


def bar(V, K, tokens, terms, doc_ll):
    """The kernels' distance from score(), per document: a positive sum of V terms in any order (the table's row sums,
    V 2^-53 relative in p), the theta sum and the K-term dot (2 K 2^-53), a few ulps of divide and log and the wavefront's
    sum of the batch (64 2^-53) - all relative errors of p, so absolute errors of log p, once per held token - and the
    document's own sum of n terms (n 2^-53 relative to |ll|)."""
    u = 2.0 ** -53
    return (V + 2 * K + 64) * u * np.asarray(tokens, dtype=np.float64) + np.asarray(terms, dtype=np.float64) * u * np.abs(doc_ll)

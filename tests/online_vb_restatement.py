"""Online variational Bayes (pylda_amd/online_vb.py) restated in numpy on top of the project's
oracles - oracle.c_oracle.e_step for the E-step, oracle.vb_numpy.m_step for the topic term - operation for operation.
TEST INFRASTRUCTURE ONLY.

Step t = 0, 1, 2, ...:
    minibatch   b = t mod B, the documents whose index is b modulo B; scale = D / |S_b| (doubles)
    step size   rho = (tau0 + t) ** (-kappa)
    E-step      the training-mode E-step (50 inner iterations, 1e-6) on the minibatch, current eta and alpha
    blend       omr = 1.0 - rho;  m = scale * s;  a = m + beta;  b = rho * a;  c = omr * eta;  eta = c + b
                (every array operation of numpy rounds each element once: the five roundings of the device kernel)
    objective   scale * document_log_likelihood(minibatch) + topic_log_likelihood(eta before the blend)
alpha is fixed."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import csr_slice
from oracle import c_oracle, vb_numpy


def step_size(tau0, kappa, t):
    return (float(tau0) + t) ** (-float(kappa))


def batch_documents(D, B, b):
    return list(range(b, D, B))


def blend(eta, sstats, beta, rho, scale):
    """The blended eta; sstats is (K, V) like eta, beta is (V,)."""
    omr = 1.0 - rho
    m = scale * sstats
    a = m + beta
    b = rho * a
    c = omr * eta
    return c + b


class OnlineRun(object):
    def __init__(self, doc_ptr, term_id, term_ct, alpha, beta, eta, batches, tau0=1.0, kappa=0.7, e_step=c_oracle.e_step):
        self.csr = (np.asarray(doc_ptr), np.asarray(term_id), np.asarray(term_ct))
        self.D = len(doc_ptr) - 1
        self.alpha = np.array(alpha, dtype=np.float64)
        self.beta = np.array(beta, dtype=np.float64)
        self.eta = np.array(eta, dtype=np.float64)
        self.B, self.tau0, self.kappa = int(batches), float(tau0), float(kappa)
        self.t = 0
        self.e_step = e_step
        K, V = self.eta.shape
        self.gamma = np.zeros((self.D, K)) + self.alpha[np.newaxis, :] + 1.0 * V / K     # variational_bayes.py:92
        self.batch_csr = {}
        self.last = None

    def batch(self, b):
        if b not in self.batch_csr:
            self.batch_csr[b] = csr_slice(*self.csr, batch_documents(self.D, self.B, b))
        return self.batch_csr[b]

    def step(self):
        b = self.t % self.B
        docs = batch_documents(self.D, self.B, b)
        rho = step_size(self.tau0, self.kappa, self.t)
        scale = float(self.D) / float(len(docs))
        e = self.e_step(self.alpha, self.eta, *self.batch(b))
        topic_ll, _, _ = vb_numpy.m_step(self.eta, self.beta, e["sstats"], e["gamma"])
        self.eta = blend(self.eta, e["sstats"], self.beta, rho, scale)
        self.gamma[docs] = e["gamma"]
        self.t += 1
        self.last = {"batch": b, "rho": rho, "scale": scale, "sstats": e["sstats"], "gamma": e["gamma"],
                     "document_log_likelihood": e["document_log_likelihood"], "topic_log_likelihood": topic_ll}
        return scale * e["document_log_likelihood"] + topic_ll


def threaded_e_step(alpha, eta, doc_ptr, term_id, term_ct, threads=8):
    """c_oracle.e_step with the documents dealt to `threads` calls that run side by side (the C oracle holds no state and
    ctypes releases the interpreter lock): every per-document value is the one call's, the statistics are the calls'
    statistics added in the order of the deal.  For the references of large K, where one call takes tens of seconds."""
    D = len(doc_ptr) - 1
    deals = [list(range(i, D, threads)) for i in range(threads) if i < D]
    with ThreadPoolExecutor(len(deals)) as pool:
        parts = list(pool.map(lambda docs: c_oracle.e_step(alpha, eta, *csr_slice(doc_ptr, term_id, term_ct, docs)), deals))
    gamma = np.zeros((D, np.shape(eta)[0]))
    sstats = np.zeros(np.shape(eta))
    for docs, part in zip(deals, parts):
        gamma[docs] = part["gamma"]
        sstats += part["sstats"]
    return {"document_log_likelihood": float(sum(part["document_log_likelihood"] for part in parts)), "sstats": sstats,
            "gamma": gamma}


def heldout_words_log_likelihood(alpha, eta, doc_ptr, term_id, term_ct):
    return c_oracle.e_step(alpha, eta, doc_ptr, term_id, term_ct, heldout=True)["words_log_likelihood"]

"""StochasticCollapsedVariationalBayes: stochastic collapsed variational Bayes (SCVB0: Foulds, Boyles, DuBois, Smyth &
Welling 2013) on an MI355X - the minibatch form of CollapsedVariationalBayes.  The reference has no such engine.

No token carries a state: the engine keeps the expected word-topic counts, their column sums and the documents' expected
topic counts, which is what lets it hold a corpus whose CVB0 rows do not fit one GPU.  The documents are dealt into
`batches` minibatches by their index modulo `batches` (CVB0's blocks, online VB's minibatches).  Step t = 0, 1, 2, ...
visits minibatch t mod B in epoch e = t // B:

    documents    every document of the minibatch runs burn_in + 1 passes over its slots against the counts of the step's
                 start; pass p has the step size rho_theta = (theta_tau0 + e (burn_in + 1) + p) ** (-theta_kappa); a slot
                 of c copies recomputes its distribution gamma from the counts and moves the document's counts by
                 N_d <- (1 - rho_theta) ** c N_d + (1 - (1 - rho_theta) ** c) C_d gamma
    blend        rho_phi = (tau0 + t) ** (-kappa); N_kw <- (1 - rho_phi) N_kw + rho_phi (C / C_M) (the minibatch's sum of
                 c gamma of the last pass) over every word, in a fixed order of summation; N_k is the column sum

(C the corpus' tokens, C_M the minibatch's, C_d the document's).  The engine is HIP kernels
(pylda_amd/csrc/scvb_kernels.h) reached through the C ABI; there is no CPU implementation of it in this package.  alpha
and beta stay fixed.  Everything that reads the trained counts - inference(), document_completion(), left_to_right(),
top_words(), topic_coherence(), similar_documents(), top_documents(), topic_distances(), the exports - is the parent's.
"""
import time

import numpy

from pylda_amd.corpus import grouped_csr
from pylda_amd.cvb0 import CollapsedVariationalBayes
from pylda_amd.online_vb import check_schedule, step_size

MAX_BURN_IN = 15


def check_burn_in(burn_in):
    """ValueError unless burn_in is an integer in [0, 15]"""
    if int(burn_in) != burn_in or not 0 <= burn_in <= MAX_BURN_IN:
        raise ValueError("burn_in=%r: the burn-in passes over a document must be an integer in [0, %d]" % (burn_in, MAX_BURN_IN))


class StochasticCollapsedVariationalBayes(CollapsedVariationalBayes):
    """step() is one minibatch, learning() one epoch (`batches` steps); everything else is CollapsedVariationalBayes'."""

    def __init__(self, batches, burn_in=1, tau0=10.0, kappa=0.9, theta_tau0=10.0, theta_kappa=0.9, device=0, seed=None):
        check_schedule(batches, tau0, kappa)
        check_schedule(batches, theta_tau0, theta_kappa)
        check_burn_in(burn_in)
        CollapsedVariationalBayes.__init__(self, device=device, seed=seed, blocks=int(batches))
        self._batches = int(batches)
        self._burn_in = int(burn_in)
        self._tau0, self._kappa = float(tau0), float(kappa)
        self._theta_tau0, self._theta_kappa = float(theta_tau0), float(theta_kappa)
        self._step = 0                                    # minibatch steps taken
        self._batch_tokens = None

    # ------------------------------------------------------------ initialise
    def _initialize_parsed(self):
        self._number_of_documents = len(self._parsed_corpus)
        if self._batches > self._number_of_documents:
            raise ValueError("batches=%d exceeds the corpus' %d documents: a minibatch would be empty"
                             % (self._batches, self._number_of_documents))
        self._train_csr = grouped_csr(self._parsed_corpus)
        self._number_of_tokens = int(self._train_csr[2].sum())
        self._ctx = self._train_corpus = self._host_state = None
        self._step = 0
        self._batch_tokens = None
        self._context().scvb_init(self._training_corpus(), self._sampler_seed, self._first_document)

    # ------------------------------------------------------------------ state
    def _get_device_state(self, corpus, want_n_kv, want_rows):
        """(n_kv, n_k, n_dk): the engine keeps no per-slot rows"""
        return self._context().scvb_get_state(corpus, want_n_kv)[:3]

    def _set_device_state(self, corpus, state):
        self._context().scvb_set_state(corpus, *state[:3])

    # --------------------------------------------------------------- learning
    def _tokens_of_batch(self, batch):
        """The tokens of every minibatch (of the global index modulo `batches`), counted once."""
        if self._batch_tokens is None:
            doc_ptr, _, term_ct = self._train_csr
            offsets = numpy.concatenate([[0], numpy.cumsum(term_ct, dtype=numpy.int64)])
            doc_tokens = offsets[doc_ptr[1:]] - offsets[doc_ptr[:-1]]
            which = (self._first_document + numpy.arange(len(doc_tokens), dtype=numpy.int64)) % self._batches
            self._batch_tokens = numpy.bincount(which, weights=doc_tokens, minlength=self._batches).astype(numpy.int64)
        return int(self._batch_tokens[batch])

    def step_parameters(self, step):
        """(minibatch, keep, gain, rho_theta) of step `step`: keep = 1 - rho_phi, gain = rho_phi * (C / C_M), rho_theta the
        step sizes of the burn_in + 1 passes; (minibatch, None, None, None) for a minibatch without tokens."""
        batch, epoch = step % self._batches, step // self._batches
        block_tokens = self._tokens_of_batch(batch)
        if block_tokens == 0:
            return batch, None, None, None
        rho_phi = step_size(self._tau0, self._kappa, step)
        passes = self._burn_in + 1
        rho_theta = [step_size(self._theta_tau0, self._theta_kappa, epoch * passes + p) for p in range(passes)]
        return batch, 1.0 - rho_phi, rho_phi * (float(self._number_of_tokens) / float(block_tokens)), rho_theta

    def step(self):
        """One minibatch step, enqueued (no host wait).  A minibatch without tokens changes nothing; the counter advances."""
        step = self._step
        self._step += 1
        batch, keep, gain, rho_theta = self.step_parameters(step)
        if keep is not None:
            self._context().scvb_step(self._training_corpus(), batch, self._batches, self._alpha_alpha, self._alpha_beta, keep, gain,
                                      rho_theta, self._first_document)

    def learning(self):
        """One epoch - `batches` steps enqueued back to back, then one likelihood call; returns the training plug-in
        log-likelihood it prints.  last_change: the documents' sum_k |N_dk after - before| of their last visit, per token."""
        self._counter += 1
        processing_time = time.time()
        for _ in range(self._batches):
            self.step()
        log_likelihood, change = self.log_likelihood()
        self.last_change = change / self._number_of_tokens if self._number_of_tokens else 0.0
        processing_time = time.time() - processing_time
        if self._verbose:
            print("iteration %i finished in %d seconds with log-likelihood %g" % (self._counter, processing_time, log_likelihood))
        return log_likelihood


if __name__ == "__main__":
    print("not implemented")

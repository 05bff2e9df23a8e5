"""CollapsedVariationalBayes: collapsed variational Bayes in its zero-order form (CVB0: Teh, Newman & Welling 2006;
Asuncion, Welling, Smyth & Teh 2009) on an MI355X.  The reference has no such engine.

A token carries a distribution over the topics in place of one sampled topic: the counts are expected counts and an update
is add, multiply and divide, deterministic after the start (the collapsed Gibbs engine's uniformly random topic per token).
The copies of a term in a document share one distribution - exact CVB0 with a term's copies updated together.  The
documents are dealt into `blocks` blocks by their index modulo `blocks`, a sweep is `blocks` rounds, and in a round every
document of the block is updated at once - one wavefront each - against the expected word-topic counts of the round's start
plus its own changes; the block's changes then go into the counts in a fixed order of summation.
blocks >= the number of documents is sequential CVB0.  The engine is HIP kernels (pylda_amd/csrc/estep_cvb0.h) reached
through the C ABI; there is no CPU implementation of it in this package.  alpha and beta stay fixed.

Held-out documents are scored by inference(): with the counts frozen they are independent and folded in exactly.
"""
import time

import numpy

from pylda_amd.corpus import grouped_csr
from pylda_amd.count_engine import HELD_OUT_STREAM_BASE, CountEngine


INFERENCE_STREAM_BASE = HELD_OUT_STREAM_BASE       # inference()'s streams: the n-th held-out call starts from stream 2^31 + n


class CollapsedVariationalBayes(CountEngine):
    """The state tuple is (n_kv, n_k, n_dk, g: the slots' rows), float64."""
    _calls_attribute, _fold_in_entry = "_inference_calls", "inference"

    def __init__(self, device=0, seed=None, blocks=16, process_group=None):
        if process_group is not None:
            raise NotImplementedError("CollapsedVariationalBayes runs on one GPU: sharding it over several is not built")
        CountEngine.__init__(self, 1, device, seed, blocks)
        self.last_change = None                           # the last sweep's mean change per token

    # ------------------------------------------------------------ initialise
    def _initialize(self, corpus, vocab, number_of_topics, alpha_alpha, alpha_beta):
        """Parse, then the collapsed Gibbs engine's start: a uniformly random topic for every token, a slot's distribution
        the histogram of its copies.  alpha_alpha and alpha_beta: scalars, or vectors over the topics / the word types."""
        CountEngine._initialize(self, vocab, number_of_topics, 1.0, 1.0)
        self._alpha_alpha = numpy.zeros(number_of_topics) + numpy.asarray(alpha_alpha, dtype=numpy.float64)
        self._alpha_beta = numpy.zeros(self._number_of_types) + numpy.asarray(alpha_beta, dtype=numpy.float64)
        self._parsed_corpus = self.parse_data(corpus)
        self._initialize_parsed()

    def _initialize_parsed(self):
        self._number_of_documents = len(self._parsed_corpus)
        self._train_csr = grouped_csr(self._parsed_corpus)
        self._number_of_tokens = int(numpy.sum(self._train_csr[2]))
        self._ctx = self._train_corpus = self._host_state = None
        self._context().cvb0_init(self._training_corpus(), self._sampler_seed, self._first_document)

    # ------------------------------------------------------------------ state
    def _get_device_state(self, corpus, want_n_kv, want_rows):
        return self._context().cvb0_get_state(corpus, want_n_kv, want_rows)

    def _set_device_state(self, corpus, state):
        self._context().cvb0_set_state(corpus, *state)

    @property
    def _n_kv(self):
        return self._state()[0]

    @property
    def _n_k(self):
        return self._state(want_n_kv=False)[1]

    @property
    def _n_dk(self):
        return self._state(want_n_kv=False)[2]

    # --------------------------------------------------------------- learning
    def log_likelihood(self):
        """(the training plug-in log-likelihood sum_d sum_n c_n log(sum_k theta_dk p(w_n | k)), the last sweep's sum of
        c |change of a slot's distribution|): fixed-order sums on the device, the same state gives the same bits."""
        return self._context().cvb0_log_likelihood(self._training_corpus(), self._alpha_alpha, self._alpha_beta)

    def learning(self):
        """One sweep over the corpus (`blocks` rounds); returns the training plug-in log-likelihood it prints."""
        self._counter += 1
        processing_time = time.time()
        self._context().cvb0_sweep(self._training_corpus(), self._alpha_alpha, self._alpha_beta, self._blocks, self._first_document)
        log_likelihood, change = self.log_likelihood()
        self.last_change = change / self._number_of_tokens if self._number_of_tokens else 0.0
        processing_time = time.time() - processing_time
        if self._verbose:
            print("iteration %i finished in %d seconds with log-likelihood %g" % (self._counter, processing_time, log_likelihood))
        return log_likelihood

    # ---------------------------------------------------------------- held-out
    def _install_predictive_table(self, ctx, what):
        """p(w | k) = (n_kv + beta) / its row sum into the context's predictive table, the frozen model of every held-out call"""
        ctx.set_eta(self._topic_table())
        ctx.completion_set_model()

    def _fold_in_device(self, ctx, corpus, stream, sweeps):
        return ctx.cvb0_foldin(corpus, self._alpha_alpha, sweeps, self._sampler_seed, stream)

    def inference(self, corpus, sweeps=50):
        """Topic proportions and the likelihood of held-out documents under the frozen expected counts: per document the
        start of training (under a stream of this call's own) and `sweeps` CVB0 sweeps over its slots.  Returns
        (words_log_likelihood, gamma_values (D, K)) with gamma = alpha + the document's expected topic counts and
        words_log_likelihood = sum_d sum_n c_n log(sum_k theta_dk p(w_n | k)), theta_d = gamma_d / sum(gamma_d): the plug-in
        estimate, theta from the same tokens.  Documents left empty by the vocabulary are dropped, as in training.  The
        training state is read, never written; a restored snapshot is evaluated from its host state."""
        return self._fold_in(corpus, sweeps=sweeps)

    def document_completion(self, corpus, sweeps=50):
        """CountEngine._document_completion, the observed halves folded in as inference() folds documents in."""
        return self._document_completion(corpus, sweeps=sweeps)

    def similar_documents(self, queries=None, top=10, metric="hellinger", sweeps=50):
        """ModelQueries.similar_documents, a training document's row being n_dk + alpha; a list of documents is folded in as
        inference(documents, sweeps) does."""
        return self._similar_documents(queries, top, metric, sweeps=sweeps)


if __name__ == "__main__":
    print("not implemented")

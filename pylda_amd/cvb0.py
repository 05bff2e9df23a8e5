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
import os
import sys
import time

import numpy

from pylda_amd import _capi, coherence, similarity, topics
from pylda_amd.inferencer import Inferencer


INFERENCE_STREAM_BASE = 1 << 31       # inference()'s streams: the n-th held-out call starts from stream 2^31 + n


class CollapsedVariationalBayes(Inferencer):
    def __init__(self, device=0, seed=None, blocks=16, process_group=None):
        Inferencer.__init__(self, 1)
        if process_group is not None:
            raise NotImplementedError("CollapsedVariationalBayes runs on one GPU: sharding it over several is not built")
        if int(blocks) < 1:
            raise ValueError("blocks must be at least 1")
        self._blocks = int(blocks)
        if seed is None:
            seed = os.environ.get("PYLDA_SEED")
        if seed is None:
            seed = numpy.random.randint(0, 2 ** 62)      # (a numpy-seeded driver stays reproducible)
        self._sampler_seed = int(seed) & (2 ** 64 - 1)
        self._device = device
        self._first_document = 0
        self._ctx = None
        self._train_corpus = None
        self._host_state = None                           # (n_kv, n_k, n_dk, g) while no device copy exists
        self._inference_calls = 0
        self.last_change = None                           # the last sweep's mean change per token
        self._verbose = True

    # ------------------------------------------------------------ initialise
    def _initialize(self, corpus, vocab, number_of_topics, alpha_alpha, alpha_beta):
        """Parse, then the collapsed Gibbs engine's start: a uniformly random topic for every token, a slot's distribution
        the histogram of its copies.  alpha_alpha and alpha_beta: scalars, or vectors over the topics / the word types."""
        Inferencer._initialize(self, vocab, number_of_topics, 1.0, 1.0)
        self._alpha_alpha = numpy.zeros(number_of_topics) + numpy.asarray(alpha_alpha, dtype=numpy.float64)
        self._alpha_beta = numpy.zeros(self._number_of_types) + numpy.asarray(alpha_beta, dtype=numpy.float64)
        self._parsed_corpus = self.parse_data(corpus)
        self._initialize_parsed()

    def _initialize_parsed(self):
        from pylda_amd.hybrid import _grouped_csr
        self._number_of_documents = len(self._parsed_corpus)
        self._train_csr = _grouped_csr(self._parsed_corpus)
        self._number_of_tokens = int(numpy.sum(self._train_csr[2]))
        self._ctx = self._train_corpus = self._host_state = None
        self._context().cvb0_init(self._training_corpus(), self._sampler_seed, self._first_document)

    def parse_data(self, corpus):
        """Per document the list of its in-vocabulary token ids, in text order (as MonteCarlo.parse_data)."""
        word_idss = []
        for document_line in corpus:
            word_ids = [self._type_to_index[token] for token in document_line.split() if token in self._type_to_index]
            if len(word_ids) == 0:
                sys.stderr.write("warning: document collapsed during parsing")
                continue
            word_idss.append(word_ids)
            if len(word_idss) % 10000 == 0 and self._verbose:
                print("successfully parse %d documents..." % len(word_idss))
        if self._verbose:
            print("successfully parse %d documents..." % len(word_idss))
        return word_idss

    # ------------------------------------------------------------------ state
    def _context(self):
        if self._ctx is None:
            self._ctx = _capi.Context(self._number_of_topics, self._number_of_types, self._device)
        return self._ctx

    def _training_corpus(self):
        """The device corpus; a restored snapshot's state goes back to the device here, as it was."""
        if self._train_corpus is None:
            self._train_corpus = self._context().corpus(*self._train_csr)
            if self._host_state is not None:
                self._context().cvb0_set_state(self._train_corpus, *self._host_state)
                self._host_state = None
        return self._train_corpus

    def _state(self, want_n_kv=True, want_g=False):
        """(n_kv, n_k, n_dk, g): from the device, or a restored snapshot's host copy (nothing is uploaded for it)"""
        if self._train_corpus is None and self._host_state is not None:
            return self._host_state
        return self._context().cvb0_get_state(self._training_corpus(), want_n_kv, want_g)

    @property
    def _n_kv(self):
        return self._state()[0]

    @property
    def _n_k(self):
        return self._state(want_n_kv=False)[1]

    @property
    def _n_dk(self):
        return self._state(want_n_kv=False)[2]

    def __getstate__(self):
        """Snapshots are pickles of the whole object: n_kv, n_k, n_dk, g, priors, seed and counter, no device handle."""
        state = dict(self.__dict__)
        if self._train_corpus is not None:
            state["_host_state"] = self._context().cvb0_get_state(self._train_corpus, True, True)
        state["_ctx"] = state["_train_corpus"] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

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
    def _topic_table(self):
        """The (K, V) table of the topics: n_kv + beta - what top_words() ranks and the held-out entries normalise."""
        return self._n_kv + self._alpha_beta[numpy.newaxis, :]

    def _predictive_table(self, ctx):
        """p(w | k) = (n_kv + beta) / its row sum into the context's predictive table, the frozen model of every held-out call"""
        ctx.set_eta(self._topic_table())
        ctx.completion_set_model()

    def _next_stream(self):
        calls = self.__dict__.get("_inference_calls", 0)
        self._inference_calls = calls + 1
        return INFERENCE_STREAM_BASE + calls

    def inference(self, corpus, sweeps=50):
        """Topic proportions and the likelihood of held-out documents under the frozen expected counts: per document the
        start of training (under a stream of this call's own) and `sweeps` CVB0 sweeps over its slots.  Returns
        (words_log_likelihood, gamma_values (D, K)) with gamma = alpha + the document's expected topic counts and
        words_log_likelihood = sum_d sum_n c_n log(sum_k theta_dk p(w_n | k)), theta_d = gamma_d / sum(gamma_d): the plug-in
        estimate, theta from the same tokens.  Documents left empty by the vocabulary are dropped, as in training.  The
        training state is read, never written; a restored snapshot is evaluated from its host state."""
        from pylda_amd.hybrid import _grouped_csr
        parsed = self.parse_data(corpus)
        if len(parsed) == 0:
            return 0.0, numpy.zeros((0, self._number_of_topics))
        ctx = self._context()
        self._predictive_table(ctx)
        heldout = ctx.corpus(*_grouped_csr(parsed))
        try:
            words_log_likelihood = ctx.cvb0_foldin(heldout, self._alpha_alpha, sweeps, self._sampler_seed, self._next_stream())
            gamma_values = numpy.array(ctx.get_gamma(heldout))
        finally:
            heldout.close()
        return words_log_likelihood, gamma_values

    def document_completion(self, corpus, sweeps=50):
        """The document-completion held-out likelihood: every test document is split into two halves
        (pylda_amd.corpus.split_for_completion), the observed half is folded in exactly as inference() does - it consumes
        one stream number - and the OTHER half is scored under theta = gamma / sum(gamma) and the same predictive table.
        Returns (held_log_likelihood, held_tokens, gamma_values (D, K)); per-word perplexity is
        exp(-held_log_likelihood / held_tokens).  The training state is read, never written."""
        from pylda_amd.corpus import split_for_completion
        from pylda_amd.hybrid import _grouped_csr
        parsed = self.parse_data(corpus)
        if len(parsed) == 0:
            return 0.0, 0, numpy.zeros((0, self._number_of_topics))
        observed_csr, held_csr = split_for_completion(*_grouped_csr(parsed))
        ctx = self._context()
        self._predictive_table(ctx)
        observed = held = None
        try:
            observed = ctx.corpus(*observed_csr)
            held = ctx.corpus(*held_csr)
            ctx.cvb0_foldin(observed, self._alpha_alpha, sweeps, self._sampler_seed, self._next_stream())
            gamma_values = numpy.array(ctx.get_gamma(observed))
            held_log_likelihood, held_tokens = ctx.completion_score(held, observed=observed)
        finally:
            for device_corpus in (observed, held):
                if device_corpus is not None:
                    device_corpus.close()
        return held_log_likelihood, held_tokens, gamma_values

    def left_to_right(self, corpus, particles=20, resample=True):
        """The left-to-right held-out likelihood (Wallach et al. 2009, Algorithm 3): an estimate of
        log p(w | Phi, alpha) of every test document with theta integrated out, Phi the predictive table of the frozen
        expected counts - the quantity the other engines' left_to_right() reports.  Returns (log_likelihood, tokens,
        per_document_log_likelihood (D,)).  It takes streams of its own; the training state is read, never written."""
        from pylda_amd.hybrid import _grouped_csr
        from pylda_amd.variational_bayes import check_left_to_right, run_left_to_right
        check_left_to_right(self, particles)
        parsed = self.parse_data(corpus)
        ctx = self._context()
        self._predictive_table(ctx)
        return run_left_to_right(self, ctx, _grouped_csr(parsed), particles, resample)

    # ------------------------------------------------------ topic coherence
    def _ranked_on_device(self, top_words, what):
        """(context, top_ids, top_values): the top words of every topic of the host table n_kv + beta"""
        coherence.refuse_process_group(self, what)
        ctx = self._context()
        return (ctx,) + ctx.top_words(top_words, table=self._topic_table())

    def topic_coherence(self, corpus=None, top_words=10):
        """UMass and NPMI coherence of the topics' top words against a reference corpus: None - the
        engine's own training documents - or a list of documents, parsed as inference() parses them.  Returns a
        pylda_amd.coherence.TopicCoherence."""
        from pylda_amd.hybrid import _grouped_csr
        ctx, top_ids, top_values = self._ranked_on_device(top_words, "topic_coherence()")
        opened = None
        try:
            if corpus is not None:
                reference = opened = ctx.corpus(*_grouped_csr(self.parse_data(corpus)))
            elif self._train_corpus is not None:
                reference = self._train_corpus
            else:               # (a restored snapshot: only the CSR is read, its state stays on the host)
                reference = opened = ctx.corpus(*self._train_csr)
            return coherence.score_topics(ctx, top_ids, top_values, reference)
        finally:
            if opened is not None:
                opened.close()

    def top_words(self, top_words=10):
        """K lists of (word, value): the top words of every topic, most probable first, with their n_kv + beta."""
        _, top_ids, top_values = self._ranked_on_device(top_words, "top_words()")
        return coherence.words_of(self, top_ids, top_values)

    # ------------------------------------------------------ nearest documents
    def similar_documents(self, queries=None, top=10, metric="hellinger", sweeps=50):
        """The `top` nearest training documents of every query by topic mixture, a training
        document's row being n_dk + alpha.  queries: None - every training document against the others -, a list of
        documents, folded in as inference(documents, sweeps) does, or a (Q, K) array of gamma rows.  Returns a
        pylda_amd.similarity.SimilarDocuments."""
        return similarity.similar_documents(self, self._n_dk + self._alpha_alpha[numpy.newaxis, :], queries, top, metric,
                                            lambda documents: self.inference(documents, sweeps)[1])

    def top_documents(self, top=10):
        """K lists of (document index, theta_dk), theta from n_dk + alpha: the training documents that show every topic
        best, best first."""
        return similarity.top_documents(self, self._n_dk + self._alpha_alpha[numpy.newaxis, :], top)

    # ------------------------------------------------------- topic distances
    def topic_distances(self, other=None, metric="jensen_shannon"):
        """The topics of this model against those of `other` as distributions over the words; this
        model's table is n_kv + beta.  Returns a pylda_amd.topics.TopicDistances (nearest(), matching())."""
        coherence.refuse_process_group(self, "topic_distances()")
        return topics.topic_distances(self, self._topic_table(), other, metric)

    # -------------------------------------------------------------- exports
    def export_beta(self, exp_beta_path, top_display=-1):
        """Per-topic word distribution from the expected counts, most probable first."""
        n_kv = self._n_kv
        with open(exp_beta_path, 'w') as output:
            for topic_index in range(self._number_of_topics):
                output.write("==========\t%d\t==========\n" % (topic_index))
                beta_probability = n_kv[topic_index, :] + self._alpha_beta
                beta_probability /= numpy.sum(beta_probability)
                ranked = numpy.argsort(beta_probability)[::-1]
                if top_display > 0:
                    ranked = ranked[:top_display]
                for type_index in ranked:
                    output.write("%s\t%g\n" % (self._index_to_type[type_index], beta_probability[type_index]))

    def export_gamma(self, exp_gamma_path, top_display=-1):
        """Per-document topic proportions from the expected counts, largest first."""
        n_dk = self._n_dk
        gamma_probability = 1.0 * n_dk / numpy.sum(n_dk, axis=1)[:, numpy.newaxis]
        with open(exp_gamma_path, 'w') as output:
            for document_index in range(self._number_of_documents):
                ranked = numpy.argsort(gamma_probability[document_index, :])[::-1]
                if top_display > 0:
                    ranked = ranked[:top_display]
                output.write("%s\n" % "\t".join("%d:%g" % (topic_index, gamma_probability[document_index, topic_index])
                                                for topic_index in ranked))


if __name__ == "__main__":
    print("not implemented")

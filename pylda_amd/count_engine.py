"""CountEngine: what the engines that keep word-topic COUNTS share - collapsed Gibbs (pylda_amd/monte_carlo.py), CVB0
(pylda_amd/cvb0.py) and, through it, SCVB0 (pylda_amd/scvb0.py).  Their training state lives in the device corpus, their
topics' table is n_kv + beta, a training document's row is n_dk + alpha, and a held-out call installs the frozen
counts' predictive table in the context and folds the documents in under a stream of its own: the n-th such call of an
engine draws from stream 2^31 + n.

Beside the training step itself an engine fills these hooks:

  _calls_attribute, _fold_in_entry             the name of its held-out call counter in __dict__ (snapshots keep it), and of
                                               its public fold-in method ("fold_in" / "inference")
  _get_device_state(corpus, want_n_kv, want_rows)   the state tuple (n_kv or None, n_k, ...) from the device; want_rows: with
                                               the per-token / per-slot part, which only a snapshot needs
  _set_device_state(corpus, state)             a snapshot's tuple back into a fresh device corpus
  _n_kv, _n_dk                                 (K, V) and (D, K) float64 counts
  _install_predictive_table(ctx, what)         the frozen model into the context, before any held-out corpus is opened
  _fold_in_device(ctx, corpus, stream, **options)   the fold-in call; returns words_log_likelihood
  _bind_context(ctx)                           (optional) what a fresh context needs beyond its creation
"""
import os
import sys

import numpy

from pylda_amd import _capi
from pylda_amd.analysis import ModelQueries
from pylda_amd.corpus import grouped_csr
from pylda_amd.inferencer import Inferencer
from pylda_amd.variational_bayes import check_left_to_right, run_left_to_right

HELD_OUT_STREAM_BASE = 1 << 31       # the held-out calls' streams: a range of their own, beside the iteration counter's


class CountEngine(ModelQueries, Inferencer):
    _device_handles = ("_ctx", "_train_corpus")         # what a snapshot leaves behind

    def __init__(self, hyper_parameter_optimize_interval, device, seed, blocks):
        Inferencer.__init__(self, hyper_parameter_optimize_interval)
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
        self._host_state = None                           # the state tuple while no device copy exists
        setattr(self, self._calls_attribute, 0)
        self._verbose = True

    def parse_data(self, corpus):
        """monte_carlo.py:76-102 of the reference: per document the list of its in-vocabulary token ids, in text order."""
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
            self._bind_context(self._ctx)
        return self._ctx

    def _bind_context(self, ctx):
        pass

    def _training_corpus(self):
        """The device corpus; a restored snapshot's state goes back to the device here, as it was."""
        if self._train_corpus is None:
            self._train_corpus = self._context().corpus(*self._train_csr)
            if self._host_state is not None:
                self._set_device_state(self._train_corpus, self._host_state)
                self._host_state = None
        return self._train_corpus

    def _state(self, want_n_kv=True, want_rows=False):
        """The state tuple: from the device, or a restored snapshot's host copy (nothing is uploaded for it)"""
        if self._train_corpus is None and self._host_state is not None:
            return self._host_state
        return self._get_device_state(self._training_corpus(), want_n_kv, want_rows)

    def __getstate__(self):
        """Snapshots are pickles of the whole object: the state tuple, priors, seed and counters, no device handle."""
        state = dict(self.__dict__)
        if self._train_corpus is not None:
            state["_host_state"] = self._get_device_state(self._train_corpus, True, True)
        for key in self._device_handles:
            state[key] = None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    # ---------------------------------------------------------------- held-out
    def _next_stream(self):
        calls = self.__dict__.get(self._calls_attribute, 0)       # (snapshots from before the counter existed have none)
        setattr(self, self._calls_attribute, calls + 1)
        return HELD_OUT_STREAM_BASE + calls

    def _fold_in(self, corpus, **options):
        """(words_log_likelihood, gamma_values (D, K)) of held-out documents under the frozen counts; consumes one stream
        number.  Documents left empty by the vocabulary are dropped, as in training."""
        parsed = self.parse_data(corpus)
        if len(parsed) == 0:
            return 0.0, numpy.zeros((0, self._number_of_topics))
        ctx = self._context()
        self._install_predictive_table(ctx, self._fold_in_entry)
        stream = self._next_stream()
        heldout = ctx.corpus(*grouped_csr(parsed))
        try:
            words_log_likelihood = self._fold_in_device(ctx, heldout, stream, **options)
            gamma_values = numpy.array(ctx.get_gamma(heldout))
        finally:
            heldout.close()
        return words_log_likelihood, gamma_values

    def _fit_queries(self, documents, **options):
        return getattr(self, self._fold_in_entry)(documents, **options)[1]

    def _document_completion(self, corpus, **options):
        """The document-completion held-out likelihood: every test document is split into two halves
        (pylda_amd.corpus.split_for_completion), the observed half is folded in exactly as the engine's fold-in does - it
        consumes one stream number - and the OTHER half is scored under theta = gamma / sum(gamma) and the same predictive
        table.  Returns (held_log_likelihood, held_tokens, gamma_values (D, K)); per-word perplexity is
        exp(-held_log_likelihood / held_tokens).  The training state is read, never written."""
        parsed = self.parse_data(corpus)
        if len(parsed) == 0:
            return 0.0, 0, numpy.zeros((0, self._number_of_topics))
        ctx = self._context()
        self._install_predictive_table(ctx, "document_completion")
        stream = self._next_stream()

        def fit(ctx, observed):
            self._fold_in_device(ctx, observed, stream, **options)
            return numpy.array(ctx.get_gamma(observed))
        return self._completion_score(ctx, grouped_csr(parsed), fit)

    def left_to_right(self, corpus, particles=20, resample=True):
        """The left-to-right held-out likelihood (Wallach et al. 2009, Algorithm 3): an estimate of
        log p(w | Phi, alpha) of every test document with theta integrated out, Phi the predictive table of the frozen
        counts - the quantity VariationalBayes.left_to_right() reports, so the engines compare.  Returns
        (log_likelihood, tokens, per_document_log_likelihood (D,)).  It takes streams of its own ((3 << 30) + 256 n for the
        n-th call): the fold-in and document_completion() keep theirs.  The training state is read, never written; a
        restored snapshot is evaluated from its host state."""
        check_left_to_right(self, particles)
        parsed = self.parse_data(corpus)
        ctx = self._context()
        self._install_predictive_table(ctx, "left_to_right")
        return run_left_to_right(self, ctx, grouped_csr(parsed), particles, resample)

    # ------------------------------------------- the hooks of ModelQueries
    def _topic_table(self):
        """The (K, V) table of the topics: n_kv + beta - what top_words() ranks and the held-out entries normalise."""
        return self._n_kv + self._alpha_beta[numpy.newaxis, :]

    def _device_topic_table(self):
        return self._topic_table()

    def _document_rows(self):
        return self._n_dk + self._alpha_alpha[numpy.newaxis, :]

    def _heldout_csr(self, corpus):
        return grouped_csr(self.parse_data(corpus))

    def _reference_csr(self):            # (a restored snapshot: only the CSR is read, its state stays on the host)
        return self._train_csr

    # -------------------------------------------------------------- exports
    def export_beta(self, exp_beta_path, top_display=-1):
        """Per-topic word distribution from the counts, most probable first (monte_carlo.py:322-337)."""
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
        """Per-document topic proportions from the counts, largest first (monte_carlo.py:339-352)."""
        n_dk = self._n_dk
        gamma_probability = 1.0 * n_dk / numpy.sum(n_dk, axis=1)[:, numpy.newaxis]
        with open(exp_gamma_path, 'w') as output:
            for document_index in range(self._number_of_documents):
                ranked = numpy.argsort(gamma_probability[document_index, :])[::-1]
                if top_display > 0:
                    ranked = ranked[:top_display]
                output.write("%s\n" % "\t".join("%d:%g" % (topic_index, gamma_probability[document_index, topic_index])
                                                for topic_index in ranked))

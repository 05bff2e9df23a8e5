"""ModelQueries: what one can ask of a trained model without changing it, written once for every engine - the topics' top
words and their coherence, the nearest documents and the documents that show a topic best
(section 18), the distances between the topics of two models (section 20), and the two-corpora skeleton of the
document-completion likelihood (section 15).  The device work is in pylda_amd.coherence, .similarity and .topics; this
class only says which table and which rows an engine puts under them.

An engine mixes the class in and fills these hooks:

  _context()                         the engine's pylda_amd._capi.Context, opened on first use
  _train_corpus                      its training documents' device corpus, or None while they are not resident
  _device_topic_table()              the `table` of Context.top_words / topic_distances: a (K, V) host array, or None once
                                     the engine's eta is on the device
  _topic_table()                     the same table as a (K, V) host array, for another engine to compare with
  _document_rows()                   (D, K) rows of the training documents, whose normalised form is theta
  _heldout_csr(documents)            CSR of a list of document strings, parsed as the engine parses held-out text
  _reference_csr()                   CSR of the training documents while they are not resident
  _fit_queries(documents, **options) (Q, K) gamma rows of held-out documents, fitted as the engine's inference fits them
"""
from pylda_amd import coherence, similarity, topics
from pylda_amd.corpus import split_for_completion


class ModelQueries(object):
    # ------------------------------------------------------ topic coherence
    def _ranked_on_device(self, top_words, what):
        """(context, top_ids, top_values): the top words of every topic of the engine's table; equal entries tie, and the
        smaller word id goes first"""
        coherence.refuse_process_group(self, what)
        ctx = self._context()
        return (ctx,) + ctx.top_words(top_words, table=self._device_topic_table())

    def topic_coherence(self, corpus=None, top_words=10):
        """UMass and NPMI coherence of the topics' top words against a reference corpus: None - the
        engine's own training documents - or a list of documents, parsed as the engine parses held-out documents.  The top
        words are picked and their co-document counts taken on the device; the training state is read, never written.
        Returns a pylda_amd.coherence.TopicCoherence."""
        ctx, top_ids, top_values = self._ranked_on_device(top_words, "topic_coherence()")
        opened = None
        try:
            if corpus is not None:
                reference = opened = ctx.corpus(*self._heldout_csr(corpus))
            elif self._train_corpus is not None:
                reference = self._train_corpus
            else:               # (a restored snapshot, an online engine: the training documents are not resident)
                reference = opened = ctx.corpus(*self._reference_csr())
            return coherence.score_topics(ctx, top_ids, top_values, reference)
        finally:
            if opened is not None:
                opened.close()

    def top_words(self, top_words=10):
        """K lists of (word, value): the top words of every topic, most probable first, with their entries of the engine's
        table (eta, or n_kv + beta)."""
        _, top_ids, top_values = self._ranked_on_device(top_words, "top_words()")
        return coherence.words_of(self, top_ids, top_values)

    # ------------------------------------------------------ nearest documents
    def similar_documents(self, queries=None, top=10, metric="hellinger"):
        """The `top` nearest training documents of every query by topic mixture.  queries: None -
        every training document against the others, itself left out -, a list of documents, fitted as the engine's
        inference fits them, or a (Q, K) array of gamma rows.  metric "hellinger" (the Bhattacharyya coefficient of the two
        thetas, and the distance from it) or "dot".  Scored and selected on the device; the training state is read, never
        written.  Returns a pylda_amd.similarity.SimilarDocuments.  (An engine whose fit takes options overrides this
        signature with them and passes them on to _similar_documents.)"""
        return self._similar_documents(queries, top, metric)

    def _similar_documents(self, queries, top, metric, **fit_options):
        return similarity.similar_documents(self, self._document_rows(), queries, top, metric,
                                            lambda documents: self._fit_queries(documents, **fit_options))

    def top_documents(self, top=10):
        """K lists of (document index, theta_dk): the training documents that show every topic best, best first."""
        return similarity.top_documents(self, self._document_rows(), top)

    # ------------------------------------------------------- topic distances
    def topic_distances(self, other=None, metric="jensen_shannon"):
        """The topics of this model against those of `other` as distributions over the words:
        None - this model against itself -, another engine of any kind over the same vocabulary, or a (K', V) array.
        metric "jensen_shannon" (the divergence in nats, and its square root as the distance) or "hellinger" (the
        Bhattacharyya coefficient, and the distance from it).  This model's table is what top_words() ranks.  Computed on
        the device; the training state is read, never written.  Returns a pylda_amd.topics.TopicDistances (nearest(),
        matching())."""
        coherence.refuse_process_group(self, "topic_distances()")
        return topics.topic_distances(self, self._device_topic_table(), other, metric)

    # --------------------------------------------------- document completion
    def _completion_score(self, ctx, csr, fit):
        """The document-completion likelihood of the documents of `csr`: their two halves
        (pylda_amd.corpus.split_for_completion) as device corpora, fit(ctx, observed corpus) -> gamma rows - the engine's
        whole step up to the score, which leaves gamma in the observed corpus and the predictive table in the context -,
        then the held halves' score.  Returns (held_log_likelihood, held_tokens, gamma_values (D, K))."""
        observed_csr, held_csr = split_for_completion(*csr)
        observed = held = None
        try:
            observed = ctx.corpus(*observed_csr)
            held = ctx.corpus(*held_csr)
            gamma_values = fit(ctx, observed)
            held_log_likelihood, held_tokens = ctx.completion_score(held, observed=observed)
        finally:
            for device_corpus in (observed, held):
                if device_corpus is not None:
                    device_corpus.close()
        return held_log_likelihood, held_tokens, gamma_values

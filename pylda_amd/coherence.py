"""Topic coherence from the device's counts.

The device answers two exact counting questions - the top words of every topic, and for every pair of a topic's top
words the documents of a reference corpus that contain both (pylda_top_words, pylda_codocument_counts) - and this
module turns the K x M x M integers into the two figures the field reports next to perplexity:

  UMass (Mimno et al. 2011)   sum over m = 2..M, l = 1..m-1 of log((D(v_m, v_l) + 1) / D(v_l)), the top words v_1 .. v_M in
                              rank order; a pair whose D(v_l) is 0 contributes 0 and is counted as undefined
  NPMI (document level)       the mean over the same M (M - 1) / 2 pairs of log(p_ml / (p_m p_l)) / (-log p_ml), p = count / D;
                              a pair that never co-occurs scores -1, one that every document holds scores 0

M = 1 gives 0 for both.  The model's figure is the plain mean over the topics.  tests/coherence_restatement.py restates
the counting and the scores with exact sums.
"""
import numpy


def scores_from_counts(doc_freq, co_doc_freq, documents):
    """(umass (K,), npmi (K,), undefined_pairs (K,)) from doc_freq (K, M), co_doc_freq (K, M, M) and the number of
    documents of the reference corpus."""
    doc_freq = numpy.asarray(doc_freq, dtype=numpy.int64)
    co_doc_freq = numpy.asarray(co_doc_freq, dtype=numpy.int64)
    K, M = doc_freq.shape
    if co_doc_freq.shape != (K, M, M):
        raise ValueError("co_doc_freq has shape %s, expected %s" % (co_doc_freq.shape, (K, M, M)))
    documents = int(documents)
    if documents < 1:
        raise ValueError("the reference corpus has no documents")
    m, l = numpy.tril_indices(M, -1)                                  # the pairs: l < m, both in rank order
    if len(m) == 0:
        return numpy.zeros(K), numpy.zeros(K), numpy.zeros(K, dtype=numpy.int64)
    both = co_doc_freq[:, m, l].astype(numpy.float64)                 # (K, pairs)
    of_m, of_l = doc_freq[:, m].astype(numpy.float64), doc_freq[:, l].astype(numpy.float64)
    defined = of_l > 0
    with numpy.errstate(divide="ignore", invalid="ignore"):
        umass_terms = numpy.where(defined, numpy.log((both + 1.0) / numpy.where(defined, of_l, 1.0)), 0.0)
        p_ml, p_m, p_l = both / documents, of_m / documents, of_l / documents
        npmi_terms = numpy.log(p_ml / (p_m * p_l)) / (-numpy.log(p_ml))
    npmi_terms = numpy.where(both == 0, -1.0, numpy.where(both == documents, 0.0, npmi_terms))
    return umass_terms.sum(axis=1), npmi_terms.sum(axis=1) / len(m), (~defined).sum(axis=1).astype(numpy.int64)


class TopicCoherence(object):
    """What topic_coherence() returns: the device's integers and table entries, and the scores from them.

      top_ids (K, M) int32, top_values (K, M) float64     the top words of every topic in rank order, with their entries
      doc_freq (K, M) int64, co_doc_freq (K, M, M) int64  documents of the reference corpus that hold a word / both words
      umass (K,), npmi (K,), undefined_pairs (K,)         per topic; umass_mean, npmi_mean: the plain means over the topics
      documents, top_words_count                          D of the reference corpus, M
    """

    def __init__(self, top_ids, top_values, doc_freq, co_doc_freq, documents):
        self.top_ids, self.top_values = top_ids, top_values
        self.doc_freq, self.co_doc_freq = doc_freq, co_doc_freq
        self.documents = int(documents)
        self.top_words_count = int(top_ids.shape[1])
        self.umass, self.npmi, self.undefined_pairs = scores_from_counts(doc_freq, co_doc_freq, documents)
        self.umass_mean = float(numpy.mean(self.umass))
        self.npmi_mean = float(numpy.mean(self.npmi))

    def as_dict(self):
        return dict(self.__dict__)


def score_topics(ctx, top_ids, top_values, reference):
    """The counts of the top words over the device corpus `reference`, and the scores."""
    doc_freq, co_doc_freq = ctx.codocument_counts(reference, top_ids)
    return TopicCoherence(top_ids, top_values, doc_freq, co_doc_freq, reference.D)


def refuse_process_group(engine, what):
    """A sharded engine holds a shard of the documents: the counts of one rank are not the corpus'."""
    group = engine.__dict__.get("_process_group")
    if group is not None:
        from pylda_amd import distributed
        if distributed.world_of(group) > 1:
            raise NotImplementedError("%s on an engine with a process group of %d ranks: every rank holds a shard of the "
                                      "documents, and a count summed over the shards is not built.  Score a snapshot "
                                      "in one process." % (what, distributed.world_of(group)))


def words_of(engine, top_ids, top_values):
    """K lists of (word, value) through the engine's vocabulary (the word id itself where the engine has none)."""
    names = engine._index_to_type
    return [[(names.get(int(v), int(v)), float(x)) for v, x in zip(ids, values)] for ids, values in zip(top_ids, top_values)]

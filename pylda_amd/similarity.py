"""Nearest documents by topic mixture.

The device answers one question - for every query row the first N rows of a base by the score sum_k a_k b_k, larger first,
equal scores by the smaller index (pylda_similarity_set_base, pylda_similar_documents) - and this module turns it into
what a user asks of a trained model:

  similar_documents   "which documents are like this one?"  Both sides as sqrt(theta), theta = gamma / sum(gamma): the score
                      is the Bhattacharyya coefficient BC, and the Hellinger distance sqrt(max(0, 1 - BC)) is taken here, on
                      the host.  metric "dot" scores theta . theta instead.
  top_documents       "which documents best show topic k?"  The base as theta and one-hot queries as given: the products
                      with 0 are exact zeros, so the score is theta_dk itself.

tests/similarity_restatement.py restates the arithmetic in numpy; the device's results equal it bit for bit.
"""
import numpy

from pylda_amd import coherence

METRICS = {"hellinger": 2, "dot": 1}       # metric -> the transform of both sides
MAX_TOP = 64


def hellinger_distance(affinity, ids):
    """sqrt(max(0, 1 - BC)) of the Bhattacharyya coefficients `affinity`; inf where the id is -1 (no document)."""
    affinity = numpy.asarray(affinity, dtype=numpy.float64)
    with numpy.errstate(invalid="ignore"):
        distance = numpy.sqrt(numpy.maximum(0.0, 1.0 - affinity))
    return numpy.where(numpy.asarray(ids) < 0, numpy.inf, distance)


class SimilarDocuments(object):
    """What similar_documents() returns.

      ids (Q, top) int32         the nearest documents of every query, nearest first; -1 where the base has no more
      affinity (Q, top) float64  their scores (hellinger: the Bhattacharyya coefficient; dot: theta . theta); -inf at id -1
      distance (Q, top)          hellinger only (None otherwise): sqrt(max(0, 1 - affinity)), inf at id -1
      metric, documents          the metric's name, D of the base
      query_rows (Q, K)          the gamma rows the queries were scored as
    """

    def __init__(self, ids, affinity, metric, documents, query_rows=None):
        self.ids, self.affinity = ids, affinity
        self.metric = metric
        self.documents = int(documents)
        self.distance = hellinger_distance(affinity, ids) if metric == "hellinger" else None
        self.query_rows = query_rows

    def as_dict(self):
        return dict(self.__dict__)


def _base_rows(rows, what):
    if rows is None or len(rows) == 0:
        raise RuntimeError("%s: the engine holds no rows of its training documents" % what)
    return numpy.ascontiguousarray(rows, dtype=numpy.float64)


def similar_documents(engine, base_rows, queries, top, metric, fit):
    """base_rows (D, K): the training documents' gamma rows.  queries: None - every training document against the
    others, itself left out -, a list of document strings - fitted by fit(documents) -> gamma rows -, or a (Q, K) array of
    gamma rows."""
    what = "similar_documents()"
    coherence.refuse_process_group(engine, what)
    if metric not in METRICS:
        raise ValueError("metric %r: one of %s" % (metric, ", ".join(sorted(METRICS))))
    top = int(top)
    if top < 1 or top > MAX_TOP:
        raise ValueError("top=%d (1 .. %d)" % (top, MAX_TOP))
    base_rows = _base_rows(base_rows, what)
    self_ids = None
    if queries is None:
        query_rows, self_ids = base_rows, numpy.arange(len(base_rows), dtype=numpy.int32)
    elif isinstance(queries, numpy.ndarray):
        query_rows = numpy.ascontiguousarray(queries, dtype=numpy.float64)
        if query_rows.ndim != 2 or query_rows.shape[1] != base_rows.shape[1]:
            raise ValueError("queries has shape %s, expected (Q, %d)" % (query_rows.shape, base_rows.shape[1]))
    else:
        query_rows = numpy.ascontiguousarray(fit(list(queries)), dtype=numpy.float64)
    if len(query_rows) == 0:
        empty = numpy.zeros((0, top))
        return SimilarDocuments(empty.astype(numpy.int32), empty, metric, len(base_rows), query_rows)
    ctx = engine._context()
    ctx.similarity_set_base(base_rows, METRICS[metric])
    ids, affinity = ctx.similar_documents(query_rows, top, METRICS[metric], self_ids)
    return SimilarDocuments(ids, affinity, metric, len(base_rows), query_rows)


def top_documents(engine, base_rows, top):
    """K lists of (document index, theta_dk), best first, equal values by the smaller index; at most `top` each."""
    what = "top_documents()"
    coherence.refuse_process_group(engine, what)
    top = int(top)
    if top < 1 or top > MAX_TOP:
        raise ValueError("top=%d (1 .. %d)" % (top, MAX_TOP))
    base_rows = _base_rows(base_rows, what)
    ctx = engine._context()
    ctx.similarity_set_base(base_rows, 1)
    ids, values = ctx.similar_documents(numpy.eye(base_rows.shape[1]), top, 0)
    return [[(int(d), float(x)) for d, x in zip(row_ids, row_values) if d >= 0] for row_ids, row_values in zip(ids, values)]

"""Topic distances and topic matching between two models.

The device answers one question - for every pair of rows of two (K', V) tables, as distributions over the words, their
Bhattacharyya coefficient or their Jensen-Shannon divergence in nats (pylda_topic_distances) - and this module turns the
matrix into what a user asks of two trained models: which topic of the other model is this one (nearest), and which
one-to-one assignment of the topics is the cheapest (matching).

An engine's table is what its top_words() ranks: the device eta for the variational family, n_kv + beta for the
collapsed Gibbs engine.  tests/topic_distance_restatement.py restates the arithmetic in numpy.
"""
import numpy

from pylda_amd import coherence

METRICS = {"hellinger": 0, "jensen_shannon": 1}
MAX_TOPICS = 1 << 15


def distance_from_values(values, metric):
    """hellinger: sqrt(max(0, 1 - BC)); jensen_shannon: sqrt(max(0, JS)), the Jensen-Shannon distance."""
    values = numpy.asarray(values, dtype=numpy.float64)
    return numpy.sqrt(numpy.maximum(0.0, 1.0 - values if metric == "hellinger" else values))


class TopicDistances(object):
    """What topic_distances() returns.

      values (Ka, Kb) float64   the device's numbers: the Bhattacharyya coefficient (hellinger) or the Jensen-Shannon
                                divergence in nats (jensen_shannon)
      distance (Ka, Kb)         the Hellinger distance sqrt(max(0, 1 - BC)), or sqrt(max(0, JS)); for a model against
                                itself the diagonal is exactly 0
      metric, against_itself    the metric's name; whether b is a
    """

    def __init__(self, values, metric, against_itself=False):
        if metric not in METRICS:
            raise ValueError("metric %r: one of %s" % (metric, ", ".join(sorted(METRICS))))
        self.values = numpy.asarray(values, dtype=numpy.float64)
        self.metric = metric
        self.against_itself = bool(against_itself)
        self.distance = distance_from_values(self.values, metric)
        if self.against_itself:
            numpy.fill_diagonal(self.distance, 0.0)

    def nearest(self, top=1):
        """(ids (Ka, n) int64, distances (Ka, n)): for every topic of a the n = min(top, candidates) nearest topics of b,
        smaller distance first, among equal distances the smaller index first.  Against itself the topic is left out."""
        top = int(top)
        if top < 1:
            raise ValueError("top=%d (at least 1)" % top)
        Ka, Kb = self.distance.shape
        keyed = self.distance.copy()
        if self.against_itself:
            numpy.fill_diagonal(keyed, numpy.inf)       # (every distance is finite: the topic itself goes last)
        order = numpy.argsort(keyed, axis=1, kind="stable")
        if self.against_itself:
            order = order[:, :Kb - 1]
        ids = order[:, :top].astype(numpy.int64)
        return ids, numpy.take_along_axis(self.distance, ids, axis=1)

    def matching(self):
        """(pairs (min(Ka, Kb), 2) int64, distances): the one-to-one assignment of a's topics to b's with the smallest
        total distance (scipy.optimize.linear_sum_assignment), sorted by a's index."""
        from scipy.optimize import linear_sum_assignment
        rows, cols = linear_sum_assignment(self.distance)
        order = numpy.argsort(rows, kind="stable")
        pairs = numpy.stack([rows[order], cols[order]], axis=1).astype(numpy.int64)
        return pairs, self.distance[pairs[:, 0], pairs[:, 1]]

    def as_dict(self):
        return dict(self.__dict__)


def first_differing_word(mine, theirs):
    """None where two word -> index maps are equal; else a sentence that names the first word (by index) that differs."""
    if mine == theirs:
        return None
    mine_by_index = sorted((index, word) for word, index in mine.items())
    theirs_by_index = sorted((index, word) for word, index in theirs.items())
    for (i, word), (j, other) in zip(mine_by_index, theirs_by_index):
        if (i, word) != (j, other):
            return "word %d is %r here and %r there" % (i, word, other)
    longer, which = (mine_by_index, "here") if len(mine_by_index) > len(theirs_by_index) else (theirs_by_index, "there")
    index, word = longer[min(len(mine_by_index), len(theirs_by_index))]
    return "word %d, %r, exists only %s (%d and %d words)" % (index, word, which, len(mine_by_index), len(theirs_by_index))


def table_of(engine):
    """The host table an engine's top_words() ranks, (K, V)."""
    return numpy.ascontiguousarray(engine._topic_table(), dtype=numpy.float64)


def topic_distances(engine, own_table, other, metric):
    """own_table: the engine's (K, V) host table, or None - its device eta, pushed by the caller.  other: None, an engine
    or a (K', V) array."""
    what = "topic_distances()"
    coherence.refuse_process_group(engine, what)
    if metric not in METRICS:
        raise ValueError("metric %r: one of %s" % (metric, ", ".join(sorted(METRICS))))
    V = engine._number_of_types
    if other is None:
        other_table = None
    elif isinstance(other, numpy.ndarray) or isinstance(other, (list, tuple)):
        other_table = numpy.ascontiguousarray(other, dtype=numpy.float64)
        if other_table.ndim != 2 or other_table.shape[1] != V:
            raise ValueError("other has shape %s, expected (K', %d)" % (other_table.shape, V))
    else:
        if not hasattr(other, "_topic_table"):
            raise TypeError("topic_distances(): %r is neither an engine nor an array" % type(other).__name__)
        coherence.refuse_process_group(other, what)
        differs = first_differing_word(engine._type_to_index, other._type_to_index)
        if differs:
            raise ValueError("topic_distances(): the two engines have different vocabularies: %s" % differs)
        other_table = table_of(other)
    for table in (own_table, other_table):
        if table is not None and not 1 <= table.shape[0] <= MAX_TOPICS:
            raise ValueError("a table of %d topics (1 .. %d)" % (table.shape[0], MAX_TOPICS))
    values = engine._context().topic_distances(own_table, other_table, METRICS[metric])
    return TopicDistances(values, metric, against_itself=other is None)

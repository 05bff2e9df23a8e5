"""The collapsed Gibbs engine sharded over several ranks, in numpy: the specification
pylda_gibbs_round_sample / pylda_gibbs_round_apply (pylda_amd/csrc/gibbs_exchange.h) are compared against.

Every shard is a gibbs_restatement.GibbsChain over a contiguous range of the documents, given its offset
(first_document) and a replica of the WHOLE corpus' word-topic table and n_k.  In a round every shard samples its
documents of the block against its own replica and packs one move record per token of the block; the records of all
shards, each segment padded with zeros to the longest, are then applied to every replica.  Pure host code."""
import numpy as np

from gibbs_restatement import GibbsChain


def pack_records(term, z_old, z_new):
    """uint64 per token: word << 32 | topic before the draw << 16 | topic after it."""
    term, z_old, z_new = (np.asarray(a).astype(np.uint64) for a in (term, z_old, z_new))
    return (term << np.uint64(32)) | (z_old << np.uint64(16)) | z_new


def apply_records(T, n_k, records):
    """T (V, K) and n_k (K,) in place: a record whose two topics differ moves one count; the others (tokens that stayed,
    zero padding) change nothing."""
    records = np.asarray(records, dtype=np.uint64)
    term = (records >> np.uint64(32)).astype(np.int64)
    z_old = ((records >> np.uint64(16)) & np.uint64(0xffff)).astype(np.int64)
    z_new = (records & np.uint64(0xffff)).astype(np.int64)
    moved = z_old != z_new
    np.add.at(T, (term[moved], z_old[moved]), -1)
    np.add.at(T, (term[moved], z_new[moved]), 1)
    np.add.at(n_k, z_old[moved], -1)
    np.add.at(n_k, z_new[moved], 1)


def shard_csr(doc_ptr, term_id, term_ct, lo, hi):
    doc_ptr = np.asarray(doc_ptr, dtype=np.int64)
    a, b = int(doc_ptr[lo]), int(doc_ptr[hi])
    return doc_ptr[lo:hi + 1] - a, np.asarray(term_id)[a:b], np.asarray(term_ct)[a:b]


class ShardedChain(object):
    def __init__(self, doc_ptr, term_id, term_ct, K, V, seed, cuts):
        """cuts: the shards' document boundaries, [0, .., D] (equal neighbours: a shard without documents)."""
        self.K, self.V, self.cuts = int(K), int(V), [int(c) for c in cuts]
        self.D = self.cuts[-1]
        self.shards = [GibbsChain(*shard_csr(doc_ptr, term_id, term_ct, lo, hi), K, V, seed=seed, first_document=lo)
                       for lo, hi in zip(self.cuts[:-1], self.cuts[1:])]

    def init(self):
        """Every shard draws its own tokens' topics; the sum of the shards' tables is every replica's start."""
        for s in self.shards:
            s.init()
        T, n_k = sum(s.T for s in self.shards), sum(s.n_k for s in self.shards)
        for s in self.shards:
            s.T, s.n_k = T.copy(), n_k.copy()

    def rounds(self, blocks):
        """blocks >= the corpus' documents: every document a round of its own, numbered by its global index."""
        return max(1, min(int(blocks), self.D))

    def block_tokens(self, shard, rounds, g):
        """Token indices of the shard's segment in round g: the block's documents in local order, their tokens in order."""
        docs = np.nonzero(shard.gdoc % np.uint64(rounds) == np.uint64(g))[0]
        if len(docs) == 0:
            return np.zeros(0, dtype=np.int64)
        return np.concatenate([shard.doc_tok0[d] + np.arange(shard.ntok[d]) for d in docs]).astype(np.int64)

    def round_records(self, shard, alpha, beta, beta_sum, rounds, g, stream):
        """The shard samples its block against its replica, which stays as it was: its changes travel as records."""
        tok = self.block_tokens(shard, rounds, g)
        z_before = shard.z[tok].copy()
        T, n_k = shard.T.copy(), shard.n_k.copy()
        shard.round(alpha, beta, beta_sum, rounds, g, stream)
        shard.T, shard.n_k = T, n_k
        return pack_records(shard.tok_term[tok], z_before, shard.z[tok])

    def round(self, alpha, beta, beta_sum, rounds, g, stream):
        """Returns what every rank receives: the shards' segments, each padded with zeros to the round's capacity."""
        segments = [self.round_records(s, alpha, beta, beta_sum, rounds, g, stream) for s in self.shards]
        capacity = max(len(r) for r in segments)
        gathered = np.zeros(capacity * len(segments), dtype=np.uint64)
        for i, r in enumerate(segments):
            gathered[i * capacity:i * capacity + len(r)] = r
        for s in self.shards:
            apply_records(s.T, s.n_k[0], gathered)
        return gathered

    def sweep(self, alpha, beta, blocks, stream):
        alpha, beta = np.zeros(self.K) + alpha, np.zeros(self.V) + beta
        rounds = self.rounds(blocks)
        for g in range(rounds):
            self.round(alpha, beta, float(np.sum(beta)), rounds, g, stream)

    def topics(self):
        return np.concatenate([s.z for s in self.shards])

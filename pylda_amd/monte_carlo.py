"""MonteCarlo: PyLDA's collapsed Gibbs engine (reference monte_carlo.py; Griffiths & Steyvers 2004) on an MI355X.

The reference resamples one token at a time against counts that are always current.  This class runs a document-parallel
approximation of that chain: the documents are dealt into `blocks` blocks by their index modulo `blocks`, a sweep is
`blocks` rounds, and in a round every document of the block is sampled at once - one wavefront each - against the
word-topic counts of the round's start plus its own changes.  blocks >= the number of documents is
the reference's sequential sampler; the fewer the blocks, the staler the counts a document sees and the slower the chain
mixes.  The sampler is a HIP kernel (pylda_amd/csrc/estep_gibbs.h) reached through the C ABI; there is no CPU
implementation of it in this package.

Held-out documents are scored by fold_in(): with the word-topic counts frozen they are independent chains, which the
document-parallel sampler runs exactly.  inference() stays NotImplementedError, as in the reference.

With a torch.distributed process group the chain is sharded over the ranks: every rank holds a
contiguous range of the documents and a full replica of the word-topic counts, and a round is sample -> all-gather of the
block's move records -> apply.  The counts are integers and a draw is named by the GLOBAL document index, so an N-rank
run assigns every token the topic the one-GPU run assigns it.

Random numbers of the sampler are counter-based (Philox4x32-10): a draw is a function of (seed, iteration, document index,
token position).  The hyper-parameter step (optimize_hyperparameters) runs on the host and draws from numpy's global
stream in the reference's order; its log posterior is evaluated on the device.
"""
import time

import numpy

from pylda_amd.corpus import grouped_csr
from pylda_amd.count_engine import HELD_OUT_STREAM_BASE, CountEngine


FOLD_IN_STREAM_BASE = HELD_OUT_STREAM_BASE      # fold_in's streams: a range of their own, beside the iteration counter's


def slice_sample_hyperparameters(log_posterior, alpha, beta, symmetric_alpha=True, symmetric_beta=True,
                                 hyper_parameter_samples=10, hyper_parameter_step=1.0, hyper_parameter_iteration=50):
    """monte_carlo.py:106-212 of the reference: slice sampling of (log alpha, log beta) against log_posterior(alpha, beta).
    Returns the (alpha, beta) it ends on.

    Kept quirk: the reference binds its interval ends and its proposal to ONE numpy array per prior (`l = old`, `l -= ..`,
    `new = l`, `new += ..`), so the lower end, the proposal and the current point move together; after a rejected
    proposal the upper end is set to that same point and every later proposal of the sample repeats it.  The arithmetic
    below is the reference's, in place on one array, with its draws from numpy's global stream in its order."""
    alpha, beta = numpy.asarray(alpha, dtype=numpy.float64), numpy.asarray(beta, dtype=numpy.float64)
    point_alpha, point_beta = numpy.log(alpha), numpy.log(beta)      # lower end = proposal = current point (one array)

    def jitter(shape, symmetric):
        return numpy.random.random() if symmetric else numpy.random.random(shape)

    for _ in range(hyper_parameter_samples):
        threshold = numpy.log(numpy.random.random()) + log_posterior(alpha, beta)
        point_alpha -= jitter(point_alpha.shape, symmetric_alpha) * hyper_parameter_step
        upper_alpha = point_alpha + hyper_parameter_step
        point_beta -= jitter(point_beta.shape, symmetric_beta) * hyper_parameter_step
        upper_beta = point_beta + hyper_parameter_step
        for _ in range(hyper_parameter_iteration):
            point_alpha += jitter(point_alpha.shape, symmetric_alpha) * (upper_alpha - point_alpha)
            new_alpha = numpy.exp(point_alpha)
            point_beta += jitter(point_beta.shape, symmetric_beta) * (upper_beta - point_beta)
            new_beta = numpy.exp(point_beta)
            if log_posterior(new_alpha, new_beta) > threshold:
                alpha, beta = new_alpha, new_beta
                break
            # (the proposal is never below the current point - they are one array - so only the upper end moves)
            upper_alpha[:] = point_alpha
            upper_beta[:] = point_beta
    return alpha, beta


class MonteCarlo(CountEngine):
    """The state tuple is (n_kv, n_k, the tokens' topics), int32."""
    _calls_attribute, _fold_in_entry = "_fold_in_calls", "fold_in"
    _device_handles = CountEngine._device_handles + ("_process_group", "_exchange")

    def __init__(self, hyper_parameter_optimize_interval=10, symmetric_alpha_alpha=True, symmetric_alpha_beta=True, device=0,
                 seed=None, blocks=16, process_group=None):
        CountEngine.__init__(self, hyper_parameter_optimize_interval, device, seed, blocks)
        self._process_group = process_group             # torch.distributed group: the documents are sharded over its ranks
        self._symmetric_alpha_alpha = symmetric_alpha_alpha
        self._symmetric_alpha_beta = symmetric_alpha_beta
        if process_group is not None:
            # one chain: rank 0's seed, wherever it came from (an argument or an environment that differs between the
            # ranks would run them as different chains and let the replicas drift apart in silence)
            from pylda_amd import distributed
            carried = numpy.array([self._sampler_seed], dtype=numpy.uint64).view(numpy.int64)     # (all 64 bits)
            self._sampler_seed = int(distributed.broadcast_int64(carried, process_group, device)[0]) & (2 ** 64 - 1)
        self._exchange = None                             # sharded: (corpus, rounds, capacity, send, recv) of the record exchange

    # ------------------------------------------------------------ initialise
    def _initialize(self, corpus, vocab, number_of_topics, alpha_alpha, alpha_beta):
        """monte_carlo.py:45-74: parse, then a uniformly random topic for every token."""
        CountEngine._initialize(self, vocab, number_of_topics, alpha_alpha, alpha_beta)
        self._parsed_corpus = self.parse_data(corpus)
        self._initialize_parsed()

    def _initialize_parsed(self):
        self._number_of_documents = len(self._parsed_corpus)
        self._train_csr = grouped_csr(self._parsed_corpus)
        self._ctx = self._train_corpus = self._host_state = self._exchange = None
        group = self.__dict__.get("_process_group")
        if group is not None:
            # the shards are contiguous: the documents on the ranks before this one name this rank's streams and blocks
            from pylda_amd import distributed
            sizes = distributed.allgather_int64(self._number_of_documents, group, self._device)
            self._first_document = int(sum(sizes[:distributed.rank_of(group)]))
            self._global_documents = int(sum(sizes))
        self._context().gibbs_init(self._training_corpus(), self._sampler_seed, self._first_document)
        if group is not None:
            # every rank counted its own documents: the replicas hold the corpus' counts from here on.  One stream of
            # host draws for the hyper-parameter step: rank 0's (a rank that proposed differently would take another
            # number of steps, and a collective would wait for ever)
            distributed.allreduce_gibbs_table(self._ctx, self._train_corpus, group)
            distributed.broadcast_numpy_random_state(group, self._device)

    # ------------------------------------------------------------------ state
    def _bind_context(self, ctx):
        if self.__dict__.get("_process_group") is not None:
            # on a stream torch knows: the collectives issued through torch.distributed are ordered with the kernels
            from pylda_amd import distributed
            distributed.bind_to_torch_stream(ctx)

    def _get_device_state(self, corpus, want_n_kv, want_rows):
        return self._context().gibbs_get_counts(corpus, want_n_kv, want_rows)

    def _set_device_state(self, corpus, state):
        self._context().gibbs_set_state(corpus, *state)

    def _counts(self, want_n_kv=True, want_topics=False):
        return self._state(want_n_kv, want_topics)

    @property
    def _n_dk(self):
        if self._train_corpus is None and self._host_state is not None:
            # a restored snapshot, or the ranks' shards gathered for an export: counted on the host, nothing uploaded
            doc_ptr, _, term_ct = self._train_csr
            documents = len(doc_ptr) - 1
            token_end = numpy.concatenate([[0], numpy.cumsum(term_ct, dtype=numpy.int64)])[numpy.asarray(doc_ptr, dtype=numpy.int64)]
            doc_tokens = numpy.diff(token_end)
            token_doc = numpy.repeat(numpy.arange(documents), doc_tokens)
            flat = numpy.bincount(token_doc * self._number_of_topics + numpy.asarray(self._host_state[2], dtype=numpy.int64),
                                  minlength=documents * self._number_of_topics)
            return flat.reshape(documents, self._number_of_topics).astype(numpy.float64)
        return numpy.array(self._context().get_gamma(self._training_corpus()))

    @property
    def _n_kv(self):
        return self._counts()[0].astype(numpy.float64)

    @property
    def _n_k(self):
        return self._counts(want_n_kv=False)[1].astype(numpy.float64)

    @property
    def _k_dn(self):
        """document -> its tokens' topics, in the order the sampler visits them (a term's copies back to back, the terms in
        first-occurrence order; the reference keeps text order, which LDA's exchangeability makes equivalent)."""
        topics = self._counts(want_n_kv=False, want_topics=True)[2]
        doc_ptr, _, term_ct = self._train_csr
        ends = numpy.concatenate([[0], numpy.cumsum(term_ct)])[numpy.asarray(doc_ptr)]
        return {d: numpy.array(topics[ends[d]:ends[d + 1]], dtype=numpy.int64) for d in range(len(doc_ptr) - 1)}

    # --------------------------------------------------------------- learning
    def log_posterior(self, alpha, beta):
        """monte_carlo.py:217-256 on the device (fixed-order sums: the same state gives the same bits)."""
        group = self.__dict__.get("_process_group")
        if group is None:
            return self._context().gibbs_log_posterior(self._training_corpus(), alpha, beta)
        # the documents' part summed over the ranks, the replica's part once; rank 0's total on every rank, so that the
        # slice sampler's accept decisions - and with them the number of collectives - are the same everywhere
        from pylda_amd import distributed
        documents, words = self._context().gibbs_log_posterior_parts(self._training_corpus(), alpha, beta)
        return distributed.sum_then_rank0_total(documents, words, group, self._device)

    def optimize_hyperparameters(self, hyper_parameter_samples=10, hyper_parameter_step=1.0, hyper_parameter_iteration=50):
        self._alpha_alpha, self._alpha_beta = slice_sample_hyperparameters(
            self.log_posterior, self._alpha_alpha, self._alpha_beta, self._symmetric_alpha_alpha, self._symmetric_alpha_beta,
            hyper_parameter_samples, hyper_parameter_step, hyper_parameter_iteration)

    def learning(self):
        """monte_carlo.py:302-320: one sweep over the corpus (`blocks` rounds), the hyper-parameter step every
        hyper_parameter_optimize_interval iterations; returns the log posterior it prints."""
        self._counter += 1
        processing_time = time.time()
        if self.__dict__.get("_process_group") is None:
            self._context().gibbs_sweep(self._training_corpus(), self._alpha_alpha, self._alpha_beta, self._blocks,
                                        self._sampler_seed, self._counter, self._first_document)
        else:
            self._sharded_sweep()
        if self._counter % self._hyper_parameter_optimize_interval == 0:
            self.optimize_hyperparameters()
        log_posterior = self.log_posterior(self._alpha_alpha, self._alpha_beta)
        processing_time = time.time() - processing_time
        if self._verbose:
            print("iteration %i finished in %d seconds with log-likelihood %g" % (self._counter, processing_time, log_posterior))
        return log_posterior

    def _exchange_plan(self):
        """(rounds, capacity, send, recv): the rounds of a sweep, the records every rank sends in each (the largest
        block of the round over the ranks: one all-reduce, once) and the device addresses of the record buffers."""
        from pylda_amd import distributed
        ctx, corpus, group = self._context(), self._training_corpus(), self._process_group
        if self._exchange is None or self._exchange[0] is not corpus:
            # blocks >= the corpus' documents: every document a round of its own, numbered by its global index
            rounds = max(1, min(self._blocks, self._global_documents))
            mine = ctx.gibbs_round_tokens(corpus, rounds, self._first_document)
            capacity = distributed.allreduce_max_int64(mine, group, self._device)
            send, recv = ctx.gibbs_exchange_prepare(corpus, rounds, self._first_document, distributed.world_of(group),
                                                    distributed.rank_of(group), capacity)
            self._exchange = (corpus, rounds, capacity, send, recv)
        return self._exchange[1:]

    def _sharded_sweep(self):
        """One sweep over the ranks' shards: per round the sampler on this rank's documents of the block, the all-gather
        of every rank's move records, and all of them applied to this rank's replica - all on the context's stream."""
        from pylda_amd import distributed
        ctx, corpus, group = self._context(), self._training_corpus(), self._process_group
        rounds, capacity, send, recv = self._exchange_plan()
        for g in range(rounds):
            if capacity[g] == 0:                          # no rank has a token in this block
                continue
            ctx.gibbs_round_sample(corpus, self._alpha_alpha, self._alpha_beta, rounds, g, self._sampler_seed, self._counter,
                                   self._first_document)
            distributed.allgather_gibbs_records(ctx, send, recv, capacity[g], group)
            ctx.gibbs_round_apply(corpus, g)

    # ---------------------------------------------------------------- held-out
    def fold_in(self, corpus, number_of_samples=50, burn_in_samples=25):
        """Topic proportions and the likelihood of held-out documents under the frozen counts: per document a Gibbs chain
        over its tokens, number_of_samples sweeps, the topic counts of the sweeps from burn_in_samples on averaged.  Returns
        (words_log_likelihood, gamma_values (D, K)) - the tuple inference() returns in the other engines - with
        gamma = alpha + the mean count and words_log_likelihood = sum_d sum_n c_n log(sum_k theta_dk p(w_n | k)),
        theta_d = gamma_d / sum(gamma_d): the plug-in estimate, theta from the same tokens.  Documents left empty by the
        vocabulary are dropped, as in training.  The training state is read, never written; a restored snapshot is
        evaluated from its host counts, without uploading its training corpus.  The n-th held-out call draws from stream
        2^31 + n."""
        return self._fold_in(corpus, number_of_samples=number_of_samples, burn_in_samples=burn_in_samples)

    def _fold_in_device(self, ctx, corpus, stream, number_of_samples, burn_in_samples):
        return ctx.foldin(corpus, self._alpha_alpha, number_of_samples, burn_in_samples, self._sampler_seed, stream)

    def _install_predictive_table(self, ctx, what):
        """The frozen counts' predictive table into the context: from the device corpus, or from a restored snapshot's
        host counts"""
        if self._train_corpus is not None:
            ctx.foldin_set_model(self._alpha_beta, trained=self._train_corpus)
        elif self._host_state is not None:
            ctx.foldin_set_model(self._alpha_beta, n_kv=self._host_state[0], n_k=self._host_state[1])
        else:
            raise RuntimeError("%s: no trained state (call _initialize first)" % what)

    def document_completion(self, corpus, number_of_samples=50, burn_in_samples=25):
        """CountEngine._document_completion, the observed halves folded in as fold_in() folds documents in."""
        return self._document_completion(corpus, number_of_samples=number_of_samples, burn_in_samples=burn_in_samples)

    def similar_documents(self, queries=None, top=10, metric="hellinger", number_of_samples=50, burn_in_samples=25):
        """ModelQueries.similar_documents, a training document's row being n_dk + alpha; a list of documents is folded in as
        fold_in(documents, number_of_samples, burn_in_samples) does (it consumes one fold-in stream number)."""
        return self._similar_documents(queries, top, metric, number_of_samples=number_of_samples, burn_in_samples=burn_in_samples)


if __name__ == "__main__":
    print("not implemented")

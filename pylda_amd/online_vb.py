"""OnlineVariationalBayes: online (minibatch) variational Bayes for LDA (Hoffman, Blei & Bach 2010) on the engine of
VariationalBayes.  The reference has no such class; DESIGN.md section 14 has the update, the dealing and the numbers.

Step t = 0, 1, 2, ... (t is _counter before learning() increments it):

    minibatch    b = t mod B: the documents whose index is b modulo B (the dealing of the Gibbs blocks: no RNG, and a
                 corpus sorted by date or source still gives mixed batches); scale = D / |S_b|
    step size    rho_t = (tau0 + t) ** (-kappa)
    E-step       the training-mode E-step of VariationalBayes (50 inner iterations, 1e-6) on the minibatch with the
                 current eta and alpha: gamma is initialised per document, nothing is carried over from earlier visits
    blend        eta <- (1 - rho_t) eta + rho_t (scale * sstats + beta), on the device (mstep_online_eta_kernel)
    returns      scale * document_log_likelihood(minibatch) + topic_log_likelihood(eta before the blend)

alpha is fixed: the class takes no hyper_parameter_optimize_interval and never runs the Newton update (stepping alpha
online is not built).  The minibatches are not sharded over several GPUs either: a process_group is refused.
"""
import time

import numpy

from pylda_amd.variational_bayes import VariationalBayes


def step_size(tau0, kappa, t):
    """rho_t = (tau0 + t) ** (-kappa), in double."""
    return (float(tau0) + t) ** (-float(kappa))


def check_schedule(batches, tau0, kappa):
    """ValueError unless batches >= 1, tau0 >= 1 (so that rho <= 1) and 0.5 < kappa <= 1 (Robbins-Monro)."""
    if int(batches) != batches or batches < 1:
        raise ValueError("batches=%r: the number of minibatches must be an integer >= 1" % (batches,))
    if not tau0 >= 1.0 or tau0 == float("inf"):
        raise ValueError("tau0=%r: needs a finite tau0 >= 1, so that the step size (tau0 + t) ** (-kappa) is at most 1" % (tau0,))
    if not 0.5 < kappa <= 1.0:
        raise ValueError("kappa=%r: needs 0.5 < kappa <= 1 for the step sizes to converge" % (kappa,))


def batch_documents(number_of_documents, batches, batch):
    """Indices of the documents of one minibatch: batch, batch + B, batch + 2 B, ..."""
    return numpy.arange(batch, number_of_documents, batches, dtype=numpy.int64)


def batch_csr(doc_ptr, term_id, term_ct, batches, batch):
    """CSR of one minibatch, its documents in corpus order."""
    doc_ptr = numpy.asarray(doc_ptr, dtype=numpy.int64)
    docs = batch_documents(len(doc_ptr) - 1, batches, batch)
    lengths = doc_ptr[docs + 1] - doc_ptr[docs]
    ptr = numpy.concatenate([numpy.zeros(1, numpy.int64), numpy.cumsum(lengths)])
    take = numpy.repeat(doc_ptr[docs] - ptr[:-1], lengths) + numpy.arange(ptr[-1], dtype=numpy.int64)
    return ptr, numpy.asarray(term_id)[take], numpy.asarray(term_ct)[take]


class OnlineVariationalBayes(VariationalBayes):
    """learning() is one online step on one minibatch; everything else - initialisation, exports, inference(),
    snapshots - is VariationalBayes'.

    learning() always takes the device path (E-step, blend, pack, ONE host wait): a subclass or an instance that
    replaces e_step or m_step is not honoured here, unlike in VariationalBayes.learning().  The public e_step() and
    m_step() keep their whole-corpus meaning.

    _gamma is a (D, K) array in document order: a document's row is the gamma of its last visit, rows of minibatches
    not visited yet hold VariationalBayes' initial value.  The minibatches' device corpora are created on their first
    visit and stay resident (plan, postings and hand-over buffers are per corpus)."""

    def __init__(self, batches, tau0=1.0, kappa=0.7, device=0, process_group=None):
        check_schedule(batches, tau0, kappa)
        if process_group is not None:
            raise NotImplementedError("OnlineVariationalBayes runs on one GPU: sharding the minibatches over a process "
                                      "group is not built.")
        # (a positive interval for the base class; the update it would schedule never runs here)
        VariationalBayes.__init__(self, 1, device, None)
        self._batches = int(batches)
        self._tau0 = float(tau0)
        self._kappa = float(kappa)
        self._batch_corpora = {}             # batch -> device corpus, created on the first visit
        self._batch_gamma_newer = set()      # batches whose device gamma is ahead of their rows of the host copy

    # ------------------------------------------------------------------ state
    def _get_gamma(self):
        gamma = VariationalBayes._gamma.fget(self)
        if self._batch_gamma_newer:
            for batch in sorted(self._batch_gamma_newer):
                gamma[batch::self._batches] = self._ctx.get_gamma(self._batch_corpora[batch])
            self._batch_gamma_newer.clear()
        return gamma

    def _set_gamma(self, value):
        VariationalBayes._gamma.fset(self, value)
        self._batch_gamma_newer.clear()

    _gamma = property(_get_gamma, _set_gamma)

    def __getstate__(self):
        state = VariationalBayes.__getstate__(self)      # (reads _gamma: the minibatches' rows are in the host copy now)
        state["_batch_corpora"] = {}
        state["_batch_gamma_newer"] = set()
        return state

    def _check_batches(self):
        if self._batches > self._number_of_documents:
            raise ValueError("batches=%d exceeds the corpus' %d documents: a minibatch would be empty"
                             % (self._batches, self._number_of_documents))

    def _initialize(self, corpus, vocab, number_of_topics, alpha_alpha, alpha_beta):
        VariationalBayes._initialize(self, corpus, vocab, number_of_topics, alpha_alpha, alpha_beta)
        self._batch_corpora = {}
        self._check_batches()

    def _initialize_parsed(self, doc_ptr, term_id, term_ct, number_of_types, number_of_topics,
                           alpha_alpha, alpha_beta, eta=None):
        VariationalBayes._initialize_parsed(self, doc_ptr, term_id, term_ct, number_of_types, number_of_topics,
                                            alpha_alpha, alpha_beta, eta=eta)
        self._batch_corpora = {}
        # the whole corpus is not needed on the device (a public e_step() uploads it again)
        self._train_corpus.close()
        self._train_corpus = None
        self._check_batches()

    def _batch_corpus(self, batch):
        corpus = self._batch_corpora.get(batch)
        if corpus is None:
            csr = self._reference_csr()
            corpus = self._context().corpus(*batch_csr(csr[0], csr[1], csr[2], self._batches, batch))
            self._batch_corpora[batch] = corpus
        return corpus

    def e_step(self, parsed_corpus=None, local_parameter_iteration=50, local_parameter_converge_threshold=1e-6):
        """VariationalBayes.e_step; in training mode (the whole corpus) its gamma replaces every minibatch's."""
        if parsed_corpus is None:
            self._batch_gamma_newer.clear()
        return VariationalBayes.e_step(self, parsed_corpus, local_parameter_iteration, local_parameter_converge_threshold)

    # -------------------------------------------------------------- learning
    def learning(self):
        """One online step; returns scale * document_log_likelihood(minibatch) + topic_log_likelihood(eta before it)."""
        step = self._counter
        self._counter += 1
        batch = step % self._batches
        rho = step_size(self._tau0, self._kappa, step)
        if self._gamma_host_stale:
            self._get_gamma()                # a whole-corpus e_step() came first: its gamma goes under this visit's rows
        ctx = self._context()
        self._push_model()
        corpus = self._batch_corpus(batch)
        scale = float(self._number_of_documents) / float(corpus.D)
        timed = self._verbose
        if timed:
            ctx.mark_time(0)
        ctx.estep(corpus, 50, 1e-6, False)
        self._reference_side_effects(corpus.D)
        if timed:
            ctx.mark_time(1)
        ctx.mstep_online_enqueue(corpus, self._alpha_beta, rho, scale)
        if timed:
            ctx.mark_time(2)
        document_log_likelihood, _, _, topic_log_likelihood, _, _ = ctx.outer_fetch()      # the ONE wait of a step
        self._eta_device_newer = True
        self._batch_gamma_newer.add(batch)
        joint_log_likelihood = scale * document_log_likelihood + topic_log_likelihood
        if self._verbose:
            print("e_step and m_step of iteration %d finished in %d and %d seconds respectively "
                  "with log likelihood %g" % (self._counter, ctx.elapsed_ms(0, 1) * 1e-3, ctx.elapsed_ms(1, 2) * 1e-3,
                                              joint_log_likelihood))
        return joint_log_likelihood

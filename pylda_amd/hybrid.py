"""Hybrid: PyLDA's hybrid engine (reference hybrid.py; Mimno, Hoffman & Blei 2012) with the E-step on an MI355X.

Per document a collapsed Gibbs sampler over its tokens runs inside the variational outer loop; the M-step, the alpha
update, the exports and the snapshots are VariationalBayes' own, unchanged (the reference's Hybrid inherits them too,
hybrid.py:23).  The sampler is a HIP kernel (pylda_amd/csrc/estep_hybrid.h) reached through the C ABI; there is no CPU
implementation of it in this package.

Random numbers are counter-based (Philox4x32-10): every draw is a function of (seed, stream, global document index,
sweep, token position), so results do not depend on the launch shape, the document order or a sharding over GPUs.
The reference draws from numpy's global stream instead; a run of this class therefore follows the same distribution as
a reference run, not the same sample path.  DESIGN.md ("Hybrid E-step") lists every difference.
"""
import os

import numpy

from pylda_amd.corpus import grouped_csr
from pylda_amd.variational_bayes import VariationalBayes

# stream numbers of held-out calls (training calls use the iteration counter, which stays below this)
HELDOUT_STREAM_BASE = 1 << 31


_grouped_csr = grouped_csr       # (the name it had while it lived here)


class Hybrid(VariationalBayes):
    def __init__(self, hyper_parameter_optimize_interval=1, device=0, process_group=None, seed=None):
        VariationalBayes.__init__(self, hyper_parameter_optimize_interval, device=device, process_group=process_group)
        if seed is None:
            seed = os.environ.get("PYLDA_SEED")
        if seed is None:
            seed = numpy.random.randint(0, 2 ** 62)      # (a numpy-seeded driver stays reproducible)
        self._sampler_seed = int(seed) & (2 ** 64 - 1)
        self._first_document = 0                          # global index of this shard's first document
        self._heldout_calls = 0
        self._number_of_samples = 10                      # hybrid.py:85 defaults, used by learning()
        self._burn_in_samples = 5

    def parse_data(self, corpus):
        """hybrid.py:53-83: per document the list of its in-vocabulary token ids, in text order (repeats kept);
        documents left empty are dropped with the reference's warning."""
        word_idss = []
        for document_line in corpus:
            word_ids = [self._type_to_index[token] for token in document_line.split() if token in self._type_to_index]
            if len(word_ids) == 0:
                import sys
                sys.stderr.write("warning: document collapsed during parsing")
                continue
            word_idss.append(word_ids)
            if len(word_idss) % 10000 == 0 and self._verbose:
                print("successfully parse %d documents..." % len(word_idss))
        if self._verbose:
            print("successfully parse %d documents..." % len(word_idss))
        return word_idss

    def _hybrid_call(self, ctx, corpus, number_of_samples, burn_in_samples, heldout):
        if heldout:
            stream = HELDOUT_STREAM_BASE + self._heldout_calls
            self._heldout_calls += 1
        else:
            stream = self._counter
        ctx.hybrid_estep(corpus, number_of_samples, burn_in_samples, self._sampler_seed, stream,
                         0 if heldout else self._first_document, heldout)

    def e_step(self, parsed_corpus=None, number_of_samples=10, burn_in_samples=5):
        """hybrid.py:85-171 on the GPU.

        Training mode (parsed_corpus is None): returns (document_log_likelihood, phi_sufficient_statistics (K, V))
        and sets self._gamma.  Held-out mode (the reference's token lists, or the CSR triple of parse_to_csr):
        returns (words_log_likelihood, gamma_values (D, K)); self._gamma is left untouched."""
        ctx = self._context()
        self._push_model()
        if parsed_corpus is None:
            corpus = self._training_corpus()
            self._hybrid_call(ctx, corpus, number_of_samples, burn_in_samples, False)
            ctx.hybrid_scale_sstats(number_of_samples - burn_in_samples)
            document_log_likelihood, _, _ = ctx.estep_results(corpus)
            self._gamma_host_stale = self._gamma_on_device = True
            return document_log_likelihood, ctx.get_sstats()
        if isinstance(parsed_corpus, tuple) and len(parsed_corpus) == 3 and isinstance(parsed_corpus[0], numpy.ndarray):
            csr = parsed_corpus
        else:
            csr = grouped_csr(parsed_corpus)
        corpus = ctx.corpus(*csr)
        try:
            self._hybrid_call(ctx, corpus, number_of_samples, burn_in_samples, True)
            _, words_log_likelihood, _ = ctx.estep_results(corpus)
            gamma_values = ctx.get_gamma(corpus)
        finally:
            corpus.close()
        return words_log_likelihood, gamma_values

    def document_completion(self, corpus, number_of_samples=10, burn_in_samples=5):
        """VariationalBayes.document_completion with this engine's sampler on the observed halves; consumes one held-out
        stream number, as inference() does."""
        def fit(ctx, observed):
            self._hybrid_call(ctx, observed, number_of_samples, burn_in_samples, True)
        return self._document_completion(self.parse_to_csr(corpus), fit)

    # learning() is VariationalBayes' device-resident iteration with this E-step in place of the variational one:
    # hybrid E-step -> [all-reduce of the raw counts] -> scale -> device M-step -> one read-back.
    def _enqueue_e_step(self, ctx, corpus, group):
        self._hybrid_call(ctx, corpus, self._number_of_samples, self._burn_in_samples, False)
        if group is not None:
            from pylda_amd import distributed
            distributed.allreduce_sstats(ctx, group)       # exact: integer counts
        ctx.hybrid_scale_sstats(self._number_of_samples - self._burn_in_samples)

    def _seam_is_overridden(self):
        cls = type(self)
        return cls.e_step is not Hybrid.e_step or cls.m_step is not VariationalBayes.m_step or \
            "e_step" in self.__dict__ or "m_step" in self.__dict__

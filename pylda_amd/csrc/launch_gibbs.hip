// libpylda_hip.so - the collapsed Gibbs engine (monte_carlo.py of the reference): initial assignment, sweeps of
// block-synchronous rounds, the log posterior, and the count tables in and out; and the same rounds sharded over several
// ranks, where the table's changes travel as move records (gibbs_exchange.h).
// (host side of the C ABI declared in include/pylda_hip.h; the kernels and the chain's specification: estep_gibbs.h)
#include "sampler_host.h"
#include "estep_gibbs.h"
#include "gibbs_exchange.h"

namespace {

// The engine's buffers of a corpus, allocated by its first call: token offsets and state words (sampler_host.h), the
// word-major int32 table, n_k, the priors and the posterior's partial sums.
int prepare_gibbs(pylda_ctx* ctx, pylda_corpus* c)
{
    if (c->d_gibbs_table) return PYLDA_OK;
    if (c->tokens >= ((int64_t)1 << 31))
        return fail(ctx, PYLDA_ERR_INVALID, "gibbs: %lld tokens (the count tables are int32: fewer than 2^31)", (long long)c->tokens);
    const size_t need = (size_t)ctx->V * ctx->ldk * sizeof(int32_t) + (size_t)ctx->K * (sizeof(int32_t) + sizeof(double)) +
                        ((size_t)ctx->V * 2 + 2) * sizeof(double) + token_state_bytes(c);
    int rc = check_device_room(ctx, "gibbs", "the count table and the token states", need);
    if (rc != PYLDA_OK || (rc = ensure_token_state(ctx, c, "gibbs")) != PYLDA_OK) return rc;
    FirstError A{ctx, "gibbs"};
    A(dev_alloc(ctx, &c->d_gibbs_nk, (size_t)ctx->K));
    A(dev_alloc(ctx, &c->d_gibbs_alpha, (size_t)ctx->K));
    A(dev_alloc(ctx, &c->d_gibbs_beta, (size_t)ctx->V));
    A(dev_alloc(ctx, &c->d_gibbs_words, (size_t)ctx->V + 2));      // (+ the posterior's one or two totals)
    A(dev_alloc(ctx, &c->d_gibbs_table, (size_t)ctx->V * ctx->ldk));
    if (A.rc != PYLDA_OK) {
        dev_free(c->d_gibbs_nk); dev_free(c->d_gibbs_alpha); dev_free(c->d_gibbs_beta); dev_free(c->d_gibbs_words);
        dev_free(c->d_gibbs_table);
    }
    return A.rc;
}

// the priors on the device; copied only when they differ from what it holds (a sweep stays asynchronous)
int upload_priors(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, const double* beta_v)
{
    const size_t K = (size_t)ctx->K, V = (size_t)ctx->V;
    if (c->h_gibbs_alpha.size() != K || memcmp(c->h_gibbs_alpha.data(), alpha_k, K * sizeof(double)) != 0) {
        c->h_gibbs_alpha.assign(alpha_k, alpha_k + K);
        HIP_TRY(ctx, hipMemcpyAsync(c->d_gibbs_alpha, alpha_k, K * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    if (c->h_gibbs_beta.size() != V || memcmp(c->h_gibbs_beta.data(), beta_v, V * sizeof(double)) != 0) {
        c->h_gibbs_beta.assign(beta_v, beta_v + V);
        HIP_TRY(ctx, hipMemcpyAsync(c->d_gibbs_beta, beta_v, V * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    return PYLDA_OK;
}

GibbsParams gibbs_params(const pylda_ctx* ctx, const pylda_corpus* c)
{
    GibbsParams p{};
    p.K = ctx->K;
    p.V = ctx->V;
    p.ldk = ctx->ldk;
    p.bits = sampler_bits(ctx->K);
    p.doc_ptr = c->d_doc_ptr;
    p.term_id = c->d_term_id;
    p.term_ct = c->d_term_ct;
    p.tok_off = c->d_tok_off;
    p.state = c->d_hyb_state;
    p.n_dk = c->d_gamma;
    p.table = c->d_gibbs_table;
    p.n_k = c->d_gibbs_nk;
    p.alpha = c->d_gibbs_alpha;
    p.beta = c->d_gibbs_beta;
    p.D = c->D;
    return p;
}

hipError_t launch_sampler(const GibbsParams& p, hipStream_t st)
{
    return with_sampler_slots(p.K, [&](auto S) {
        return launch_kernel(gibbs_sample_kernel<decltype(S)::value>, dim3((unsigned)((p.count + 3) / 4)), dim3(256), 0, st, p);
    });
}

// one round: the block's documents are sampled against the frozen table, then their changes go into it
hipError_t launch_round(const GibbsParams& p, hipStream_t st)
{
    const hipError_t e = launch_sampler(p, st);
    if (e != hipSuccess) return e;
    return launch_kernel(gibbs_apply_kernel, dim3((unsigned)((p.count + 3) / 4)), dim3(256), (size_t)p.K * sizeof(int), st, p);
}

// first local document and number of documents of round g's block (global index = g modulo blocks)
void round_block(const pylda_corpus* c, int64_t blocks, int64_t first_document, int64_t g, int64_t* first, int64_t* count)
{
    *first = ((g - first_document) % blocks + blocks) % blocks;
    *count = *first < c->D ? (c->D - *first + blocks - 1) / blocks : 0;
}

// tokens of every document (D), read back from the corpus' CSR
int document_tokens(pylda_ctx* ctx, const pylda_corpus* c, std::vector<int64_t>* tokens)
{
    std::vector<int64_t> ptr((size_t)c->D + 1, 0);
    std::vector<int32_t> cts((size_t)c->nnz);
    HIP_TRY(ctx, hipMemcpy(ptr.data(), c->d_doc_ptr, ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (c->nnz) HIP_TRY(ctx, hipMemcpy(cts.data(), c->d_term_ct, cts.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    tokens->assign((size_t)c->D, 0);
    for (int64_t d = 0; d < c->D; ++d)
        for (int64_t q = ptr[(size_t)d]; q < ptr[(size_t)d + 1]; ++q) (*tokens)[(size_t)d] += cts[(size_t)q];
    return PYLDA_OK;
}

int check_blocks(pylda_ctx* ctx, const char* what, int64_t blocks)
{
    if (blocks < 1) return fail(ctx, PYLDA_ERR_INVALID, "%s: blocks=%lld (at least 1)", what, (long long)blocks);
    // (the host keeps two entries per round; more rounds than the corpus has documents are the chain of blocks = that count)
    if (blocks > ((int64_t)1 << 24))
        return fail(ctx, PYLDA_ERR_INVALID, "%s: blocks=%lld (at most 2^24; above the global document count pass that count)", what, (long long)blocks);
    return PYLDA_OK;
}

// What the log posterior's entry points share, up to their sum kernel: the checks, the priors on the device, the scalar
// terms on the host in the reference's order of summation (monte_carlo.py:222-243), and the two term kernels, which leave
// the documents' terms in d_doc_ll and the words' in d_gibbs_words.
struct PosteriorScalars {
    double alpha_sum = 0.0, beta_sum = 0.0, alpha_lg = 0.0, beta_lg = 0.0;
};

int posterior_terms(pylda_ctx* ctx, pylda_corpus* c, const char* what, const double* alpha_k, const double* beta_v, bool has_out,
                    PosteriorScalars* h)
{
    int rc = check_sampler_call(ctx, c, what, 0);
    if (rc != PYLDA_OK) return rc;
    if (!c->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "%s: gibbs_init or gibbs_set_state must be called first", what);
    if (!alpha_k || !beta_v || !has_out) return fail(ctx, PYLDA_ERR_INVALID, "%s: alpha, beta or out is NULL", what);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = upload_priors(ctx, c, alpha_k, beta_v)) != PYLDA_OK) return rc;
    for (int k = 0; k < ctx->K; ++k) { h->alpha_sum += alpha_k[k]; h->alpha_lg += std::lgamma(alpha_k[k]); }
    for (int v = 0; v < ctx->V; ++v) { h->beta_sum += beta_v[v]; h->beta_lg += std::lgamma(beta_v[v]); }
    if (c->D > 0)
        HIP_TRY(ctx, launch_kernel(gibbs_doc_posterior_kernel, dim3((unsigned)((c->D + 3) / 4)), dim3(256), 0, ctx->stream,
                                   c->d_gamma, c->d_gibbs_alpha, h->alpha_sum, ctx->K, c->D, c->d_doc_ll));
    HIP_TRY(ctx, launch_kernel(gibbs_word_posterior_kernel, dim3((unsigned)ctx->V), dim3(256), 0, ctx->stream, c->d_gibbs_table,
                               c->d_gibbs_beta, ctx->K, ctx->ldk, c->d_gibbs_words));
    return PYLDA_OK;
}

}  // namespace

extern "C" {

int pylda_gibbs_init(pylda_ctx* ctx, pylda_corpus* c, uint64_t seed, int64_t first_document)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "gibbs_init", first_document);
    if (rc != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = prepare_gibbs(ctx, c)) != PYLDA_OK) return rc;
    GibbsParams p = gibbs_params(ctx, c);
    p.first_document = (uint32_t)first_document;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);
    HIP_TRY(ctx, hipMemsetAsync(c->d_gibbs_table, 0, (size_t)ctx->V * ctx->ldk * sizeof(int32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(c->d_gibbs_nk, 0, (size_t)ctx->K * sizeof(int32_t), ctx->stream));
    if (c->D > 0)
        HIP_TRY(ctx, launch_kernel(gibbs_init_kernel, dim3((unsigned)((c->D + 3) / 4)), dim3(256), (size_t)4 * ctx->K * sizeof(int),
                                   ctx->stream, p));
    c->gibbs_ready = true;
    c->estep_done = true;           // (pylda_get_gamma hands out n_dk)
    return PYLDA_OK;
}

int pylda_gibbs_sweep(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, const double* beta_v, double beta_sum, int64_t blocks,
                      uint64_t seed, uint64_t stream, int64_t first_document)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "gibbs_sweep", first_document);
    if (rc != PYLDA_OK) return rc;
    if (!c->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "gibbs_sweep: gibbs_init or gibbs_set_state must be called first");
    if (!alpha_k || !beta_v || !(beta_sum > 0.0)) return fail(ctx, PYLDA_ERR_INVALID, "gibbs_sweep: alpha, beta or beta_sum missing");
    if (blocks < 1) return fail(ctx, PYLDA_ERR_INVALID, "gibbs_sweep: blocks=%lld (at least 1)", (long long)blocks);
    if (stream > 0xffffffffull) return fail(ctx, PYLDA_ERR_INVALID, "gibbs_sweep: stream %llu >= 2^32", (unsigned long long)stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = upload_priors(ctx, c, alpha_k, beta_v)) != PYLDA_OK) return rc;
    GibbsParams p = gibbs_params(ctx, c);
    p.beta_sum = beta_sum;
    p.first_document = (uint32_t)first_document;
    p.stream = (uint32_t)stream;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);
    p.step = blocks;
    const int bracket = open_bracket(ctx, -1, ctx->stream);
    // block g: the documents whose global index is g modulo blocks; rounds past the last document have no block
    const int64_t g_begin = blocks >= first_document + c->D ? first_document : 0;      // (every document a block of its own)
    for (int64_t g = g_begin; g < std::min<int64_t>(blocks, first_document + c->D); ++g) {
        p.first = ((g - first_document) % blocks + blocks) % blocks;
        p.count = p.first < c->D ? (c->D - p.first + blocks - 1) / blocks : 0;
        if (p.count > 0) HIP_TRY(ctx, launch_round(p, ctx->stream));
    }
    close_bracket(ctx, bracket, ctx->stream);
    return PYLDA_OK;
}

int pylda_gibbs_log_posterior(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, const double* beta_v, double* out)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    PosteriorScalars h;
    const int rc = posterior_terms(ctx, c, "gibbs_log_posterior", alpha_k, beta_v, out != nullptr, &h);
    if (rc != PYLDA_OK) return rc;
    double* d_out = c->d_gibbs_words + ctx->V;
    HIP_TRY(ctx, launch_kernel(gibbs_posterior_sum_kernel, dim3(1), dim3(256), 0, ctx->stream, c->d_doc_ll, c->D, c->d_gibbs_words,
                               ctx->V, c->d_gibbs_nk, ctx->K, h.beta_sum, d_out));
    double device_sum = 0.0;
    HIP_TRY(ctx, hipMemcpyAsync(&device_sum, d_out, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out = (std::lgamma(h.alpha_sum) - h.alpha_lg) * (double)c->D + (std::lgamma(h.beta_sum) - h.beta_lg) * (double)ctx->K + device_sum;
    return PYLDA_OK;
}

int pylda_gibbs_get_counts(pylda_ctx* ctx, pylda_corpus* c, int32_t* n_kv, int32_t* n_k, int32_t* topics)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "gibbs_get_counts", 0);
    if (rc != PYLDA_OK) return rc;
    if (!c->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "gibbs_get_counts: gibbs_init or gibbs_set_state must be called first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int K = ctx->K;
    if (n_kv && (rc = table_to_host(ctx, c->d_gibbs_table, n_kv)) != PYLDA_OK) return rc;
    if (n_k) HIP_TRY(ctx, hipMemcpy(n_k, c->d_gibbs_nk, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (topics && c->tokens) {
        std::vector<uint64_t> state((size_t)c->tokens);
        HIP_TRY(ctx, hipMemcpy(state.data(), c->d_hyb_state, state.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        const uint64_t mask = ((uint64_t)1 << sampler_bits(K)) - 1;
        for (size_t t = 0; t < state.size(); ++t) topics[t] = (int32_t)(state[t] & mask);
    }
    return PYLDA_OK;
}

int pylda_gibbs_set_state(pylda_ctx* ctx, pylda_corpus* c, const int32_t* n_kv, const int32_t* n_k, const int32_t* topics)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "gibbs_set_state", 0);
    if (rc != PYLDA_OK) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool fresh = !c->gibbs_ready;
    if (fresh && (!n_kv || !n_k || !topics))
        return fail(ctx, PYLDA_ERR_STATE, "gibbs_set_state: a corpus without a state needs the table, n_k and the topics");
    if ((rc = prepare_gibbs(ctx, c)) != PYLDA_OK) return rc;
    const int K = ctx->K, bits = sampler_bits(K);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n_kv && (rc = table_from_host(ctx, c->d_gibbs_table, n_kv)) != PYLDA_OK) return rc;
    if (n_k) HIP_TRY(ctx, hipMemcpy(c->d_gibbs_nk, n_k, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice));
    if (topics) {
        std::vector<uint64_t> state((size_t)c->tokens);
        for (size_t t = 0; t < state.size(); ++t) {
            if (topics[t] < 0 || topics[t] >= K) return fail(ctx, PYLDA_ERR_INVALID, "gibbs_set_state: topic %d of token %zu", topics[t], t);
            state[t] = (uint64_t)topics[t] | ((uint64_t)topics[t] << bits);
        }
        if (c->tokens)
            HIP_TRY(ctx, hipMemcpy(c->d_hyb_state, state.data(), state.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        if (c->D > 0)           // n_dk follows from the topics
            HIP_TRY(ctx, launch_kernel(gibbs_recount_kernel, dim3((unsigned)((c->D + 3) / 4)), dim3(256), (size_t)4 * K * sizeof(int),
                                       ctx->stream, gibbs_params(ctx, c)));
    }
    c->gibbs_ready = true;
    c->estep_done = true;
    return PYLDA_OK;
}

// ---- the sweep sharded over several ranks ----
int pylda_gibbs_round_tokens(pylda_ctx* ctx, pylda_corpus* c, int64_t blocks, int64_t first_document, int64_t* tokens)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "gibbs_round_tokens", first_document);
    if (rc != PYLDA_OK) return rc;
    if ((rc = check_blocks(ctx, "gibbs_round_tokens", blocks)) != PYLDA_OK) return rc;
    if (!tokens) return fail(ctx, PYLDA_ERR_INVALID, "gibbs_round_tokens: tokens is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<int64_t> doc_tokens;
    if ((rc = document_tokens(ctx, c, &doc_tokens)) != PYLDA_OK) return rc;
    for (int64_t g = 0; g < blocks; ++g) tokens[g] = 0;
    for (int64_t d = 0; d < c->D; ++d) tokens[(first_document + d) % blocks] += doc_tokens[(size_t)d];
    return PYLDA_OK;
}

int pylda_gibbs_exchange_prepare(pylda_ctx* ctx, pylda_corpus* c, int64_t blocks, int64_t first_document, int world, int rank,
                                 const int64_t* capacity, void** send, void** recv)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "gibbs_exchange_prepare", first_document);
    if (rc != PYLDA_OK) return rc;
    if ((rc = check_blocks(ctx, "gibbs_exchange_prepare", blocks)) != PYLDA_OK) return rc;
    if (!capacity || !send || !recv) return fail(ctx, PYLDA_ERR_INVALID, "gibbs_exchange_prepare: capacity, send or recv is NULL");
    if (world < 1 || rank < 0 || rank >= world)
        return fail(ctx, PYLDA_ERR_INVALID, "gibbs_exchange_prepare: rank %d of %d", rank, world);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<int64_t> doc_tokens;
    if ((rc = document_tokens(ctx, c, &doc_tokens)) != PYLDA_OK) return rc;
    // a document's first record: the tokens of the documents of its block before it
    std::vector<int64_t> round_tokens((size_t)blocks, 0), rec_off((size_t)c->D, 0);
    for (int64_t d = 0; d < c->D; ++d) {
        int64_t& at = round_tokens[(size_t)((first_document + d) % blocks)];
        rec_off[(size_t)d] = at;
        at += doc_tokens[(size_t)d];
    }
    int64_t widest = 0;
    for (int64_t g = 0; g < blocks; ++g) {
        if (capacity[g] < round_tokens[(size_t)g])
            return fail(ctx, PYLDA_ERR_INVALID, "gibbs_exchange_prepare: capacity[%lld]=%lld, this corpus has %lld tokens in that round",
                        (long long)g, (long long)capacity[g], (long long)round_tokens[(size_t)g]);
        widest = std::max(widest, capacity[g]);
    }
    if (widest >= ((int64_t)1 << 31) / world * 256)         // (the apply pass: one thread per record, a grid below 2^31 workgroups)
        return fail(ctx, PYLDA_ERR_INVALID, "gibbs_exchange_prepare: %lld records per rank and round", (long long)widest);
    // the memory check before anything is given up: a call it refuses leaves the plan before as it was (its buffers,
    // freed below, count as free)
    const size_t need = ((size_t)widest * ((size_t)world + 1) + (size_t)c->D) * sizeof(int64_t);
    size_t held = 0;
    if (c->gibbs_exchange_world) {
        int64_t old_widest = 0;
        for (int64_t cap : c->h_gibbs_capacity) old_widest = std::max(old_widest, cap);
        held = ((size_t)old_widest * ((size_t)c->gibbs_exchange_world + 1) + (size_t)c->D) * sizeof(int64_t);
    }
    size_t free_bytes = 0, total_bytes = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
    if (need + ((size_t)256 << 20) > free_bytes + held)
        return fail(ctx, PYLDA_ERR_OOM, "gibbs_exchange_prepare: the record buffers of %d ranks need %zu MiB, %zu MiB of device memory are free",
                    world, need >> 20, (free_bytes + held) >> 20);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));        // (a round of the plan before may still read its buffers)
    dev_free(c->d_gibbs_send); dev_free(c->d_gibbs_recv); dev_free(c->d_gibbs_rec_off);
    c->gibbs_exchange_world = 0;
    FirstError A{ctx, "gibbs_exchange_prepare"};
    A(dev_alloc(ctx, &c->d_gibbs_send, (size_t)widest));
    A(dev_alloc(ctx, &c->d_gibbs_recv, (size_t)widest * (size_t)world));
    A(dev_alloc(ctx, &c->d_gibbs_rec_off, (size_t)c->D));
    A.h2d(c->d_gibbs_rec_off, rec_off.data(), rec_off.size() * sizeof(int64_t));
    if (A.rc != PYLDA_OK) {
        dev_free(c->d_gibbs_send); dev_free(c->d_gibbs_recv); dev_free(c->d_gibbs_rec_off);
        return A.rc;
    }
    c->h_gibbs_capacity.assign(capacity, capacity + blocks);
    c->h_gibbs_round_tokens.swap(round_tokens);
    c->gibbs_exchange_blocks = blocks;
    c->gibbs_exchange_first = first_document;
    c->gibbs_exchange_world = world;
    *send = c->d_gibbs_send;
    *recv = c->d_gibbs_recv;
    return PYLDA_OK;
}

int pylda_gibbs_round_sample(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, const double* beta_v, double beta_sum, int64_t blocks,
                             int64_t round, uint64_t seed, uint64_t stream, int64_t first_document)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "gibbs_round_sample", first_document);
    if (rc != PYLDA_OK) return rc;
    if (!c->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "gibbs_round_sample: gibbs_init or gibbs_set_state must be called first");
    if (!alpha_k || !beta_v || !(beta_sum > 0.0)) return fail(ctx, PYLDA_ERR_INVALID, "gibbs_round_sample: alpha, beta or beta_sum missing");
    if (blocks < 1) return fail(ctx, PYLDA_ERR_INVALID, "gibbs_round_sample: blocks=%lld (at least 1)", (long long)blocks);
    if (stream > 0xffffffffull) return fail(ctx, PYLDA_ERR_INVALID, "gibbs_round_sample: stream %llu >= 2^32", (unsigned long long)stream);
    if (!c->gibbs_exchange_world) return fail(ctx, PYLDA_ERR_STATE, "gibbs_round_sample: gibbs_exchange_prepare must be called first");
    if (blocks != c->gibbs_exchange_blocks || first_document != c->gibbs_exchange_first)
        return fail(ctx, PYLDA_ERR_STATE, "gibbs_round_sample: blocks=%lld, first_document=%lld; the exchange was prepared for %lld, %lld",
                    (long long)blocks, (long long)first_document, (long long)c->gibbs_exchange_blocks, (long long)c->gibbs_exchange_first);
    if (round < 0 || round >= blocks) return fail(ctx, PYLDA_ERR_STATE, "gibbs_round_sample: round %lld of %lld", (long long)round, (long long)blocks);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((rc = upload_priors(ctx, c, alpha_k, beta_v)) != PYLDA_OK) return rc;
    GibbsParams p = gibbs_params(ctx, c);
    p.beta_sum = beta_sum;
    p.first_document = (uint32_t)first_document;
    p.stream = (uint32_t)stream;
    p.seed_lo = (uint32_t)seed;
    p.seed_hi = (uint32_t)(seed >> 32);
    p.step = blocks;
    round_block(c, blocks, first_document, round, &p.first, &p.count);
    const dim3 grid((unsigned)((p.count + 3) / 4));
    if (p.count > 0) {
        const int bracket = open_bracket(ctx, -1, ctx->stream);
        const hipError_t e = launch_sampler(p, ctx->stream);
        close_bracket(ctx, bracket, ctx->stream);
        HIP_TRY(ctx, e);
    }
    // the segment: a record per token of the block, zeros up to what every rank sends (an empty block: zeros only)
    const int64_t mine = c->h_gibbs_round_tokens[(size_t)round], cap = c->h_gibbs_capacity[(size_t)round];
    const int bracket = open_bracket(ctx, -2, ctx->stream);
    hipError_t e = hipSuccess;
    if (cap > mine) e = hipMemsetAsync(c->d_gibbs_send + mine, 0, (size_t)(cap - mine) * sizeof(uint64_t), ctx->stream);
    if (e == hipSuccess && p.count > 0)
        e = launch_kernel(gibbs_pack_kernel, grid, dim3(256), 0, ctx->stream, p, (const int64_t*)c->d_gibbs_rec_off, c->d_gibbs_send);
    close_bracket(ctx, bracket, ctx->stream);
    HIP_TRY(ctx, e);
    return PYLDA_OK;
}

int pylda_gibbs_round_apply(pylda_ctx* ctx, pylda_corpus* c, int64_t round)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "gibbs_round_apply", 0);
    if (rc != PYLDA_OK) return rc;
    if (!c->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "gibbs_round_apply: gibbs_init or gibbs_set_state must be called first");
    if (!c->gibbs_exchange_world) return fail(ctx, PYLDA_ERR_STATE, "gibbs_round_apply: gibbs_exchange_prepare must be called first");
    if (round < 0 || round >= c->gibbs_exchange_blocks)
        return fail(ctx, PYLDA_ERR_STATE, "gibbs_round_apply: round %lld of %lld", (long long)round, (long long)c->gibbs_exchange_blocks);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t n = c->h_gibbs_capacity[(size_t)round] * c->gibbs_exchange_world;
    if (n == 0) return PYLDA_OK;
    const int bracket = open_bracket(ctx, -2, ctx->stream);
    const hipError_t e = launch_kernel(gibbs_record_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), (size_t)ctx->K * sizeof(int),
                                       ctx->stream, (const uint64_t*)c->d_gibbs_recv, n, c->d_gibbs_table, c->d_gibbs_nk, ctx->K, ctx->V, ctx->ldk);
    close_bracket(ctx, bracket, ctx->stream);
    HIP_TRY(ctx, e);
    return PYLDA_OK;
}

int pylda_gibbs_table_device(pylda_ctx* ctx, pylda_corpus* c, void** table, int64_t* table_elements, void** n_k)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    int rc = check_sampler_call(ctx, c, "gibbs_table_device", 0);
    if (rc != PYLDA_OK) return rc;
    if (!c->gibbs_ready) return fail(ctx, PYLDA_ERR_STATE, "gibbs_table_device: gibbs_init or gibbs_set_state must be called first");
    if (table) *table = c->d_gibbs_table;
    if (table_elements) *table_elements = (int64_t)ctx->V * ctx->ldk;
    if (n_k) *n_k = c->d_gibbs_nk;
    return PYLDA_OK;
}

int pylda_gibbs_log_posterior_parts(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, const double* beta_v, double* out)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    PosteriorScalars h;
    const int rc = posterior_terms(ctx, c, "gibbs_log_posterior_parts", alpha_k, beta_v, out != nullptr, &h);
    if (rc != PYLDA_OK) return rc;
    double* d_out = c->d_gibbs_words + ctx->V;
    HIP_TRY(ctx, launch_kernel(gibbs_posterior_parts_kernel, dim3(1), dim3(256), 0, ctx->stream, c->d_doc_ll, c->D, c->d_gibbs_words,
                               ctx->V, c->d_gibbs_nk, ctx->K, h.beta_sum, d_out));
    double device_sums[2] = {0.0, 0.0};
    HIP_TRY(ctx, hipMemcpyAsync(device_sums, d_out, sizeof(device_sums), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    out[0] = (std::lgamma(h.alpha_sum) - h.alpha_lg) * (double)c->D + device_sums[0];
    out[1] = (std::lgamma(h.beta_sum) - h.beta_lg) * (double)ctx->K + device_sums[1];
    return PYLDA_OK;
}

int pylda_test_gibbs_posterior_terms(pylda_ctx* ctx, pylda_corpus* c, const double* alpha_k, const double* beta_v, double* doc_terms,
                                     double* word_terms, double* sums)
{
    if (!ctx) return PYLDA_ERR_INVALID;
    PosteriorScalars h;
    const int rc = posterior_terms(ctx, c, "test_gibbs_posterior_terms", alpha_k, beta_v, doc_terms && word_terms && sums, &h);
    if (rc != PYLDA_OK) return rc;
    double* d_out = c->d_gibbs_words + ctx->V;
    // the whole, as pylda_gibbs_log_posterior sums it; read back before the parts kernel writes the same two doubles
    HIP_TRY(ctx, launch_kernel(gibbs_posterior_sum_kernel, dim3(1), dim3(256), 0, ctx->stream, c->d_doc_ll, c->D, c->d_gibbs_words,
                               ctx->V, c->d_gibbs_nk, ctx->K, h.beta_sum, d_out));
    HIP_TRY(ctx, hipMemcpyAsync(sums, d_out, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, launch_kernel(gibbs_posterior_parts_kernel, dim3(1), dim3(256), 0, ctx->stream, c->d_doc_ll, c->D, c->d_gibbs_words,
                               ctx->V, c->d_gibbs_nk, ctx->K, h.beta_sum, d_out));
    HIP_TRY(ctx, hipMemcpyAsync(sums + 1, d_out, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (c->D > 0)
        HIP_TRY(ctx, hipMemcpyAsync(doc_terms, c->d_doc_ll, (size_t)c->D * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(word_terms, c->d_gibbs_words, (size_t)ctx->V * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return PYLDA_OK;
}

}  // extern "C"

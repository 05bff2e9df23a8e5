// Sanitizer driver for the packed launch slots of the quad kernel (pylda_amd/csrc/host_plan.cpp quad_slot_layout,
// estep_limits.h quad_slot_term / quad_ids_at): built by tests/test_quad_slots_sanitizers.py with
// g++ -fsanitize=address,undefined and run on the CPU.  Random CSR corpora at the table strides of the quad kernel; the
// packer's index arithmetic fills exactly-sized heap buffers (a write past the end is an ASan error) and the result is
// held against what the kernel's prologue computes without the slots:
//   * every (launch slot, word group gg, word slot s) of a packed class holds wid[s] = term s * 16 + gg of the document
//     (s * 16 + 15 - gg in the streamed slots), -1 beyond the document and in the padding of the stride;
//   * no two launch slots overlap, the classes' parts tile the two arrays, and the bytes are what layout() reports;
//   * the record holds the document, its length, its offset and its token total;
//   * classes of table stride 128 and other kernels have no slots.
#include "../../pylda_amd/csrc/host_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

using namespace pylda_plan;
using namespace pylda;

static uint64_t state = 0xD1B54A32D192ED03ull;
static uint32_t rnd()
{
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return (uint32_t)(state >> 32);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

#define REQUIRE(cond, ...)                                          \
    do {                                                            \
        if (!(cond)) {                                              \
            fprintf(stderr, "quad slots fuzz: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                           \
            fprintf(stderr, "\n");                                  \
            return 1;                                               \
        }                                                           \
    } while (0)

// the kernel's expression for the term of word slot s of group gg (estep_quad.h before the slots), spelled out
static int present_term(int s, int gg, int wpr) { return s * 16 + (s < wpr ? gg : 15 - gg); }

static int check_one()
{
    static const int ks[] = {65, 100, 128, 129, 200, 256, 64, 300};
    PlanConfig cfg;
    cfg.K = ks[rnd() % 8];
    cfg.ldk = table_stride_for(cfg.K);
    cfg.V = rnd_in(300, 5000);
    cfg.lds_limit = 160 * 1024;
    cfg.quad_stream = rnd() % 4 != 0;
    const int64_t D = rnd_in(1, 400);
    static const int edges[] = {1, 15, 16, 17, 128, 129, 159, 160, 161, 175, 176, 177, 191, 192, 193, 207, 208, 209, 223, 224, 225, 239, 240, 241, 255, 256, 257};
    std::vector<int64_t> doc_ptr((size_t)D + 1, 0);
    for (int64_t d = 0; d < D; ++d) {
        const int n = rnd() % 3 ? edges[rnd() % (sizeof edges / sizeof edges[0])] : rnd_in(0, 300);
        doc_ptr[(size_t)d + 1] = doc_ptr[(size_t)d] + std::min(n, cfg.V);
    }
    const int64_t nnz = doc_ptr[(size_t)D];
    std::vector<int32_t> term_id((size_t)nnz), term_ct((size_t)nnz);
    for (int64_t i = 0; i < nnz; ++i) {
        term_id[(size_t)i] = rnd_in(0, cfg.V - 1);
        term_ct[(size_t)i] = rnd_in(1, 9);
    }
    // schedule: longest documents first, stable (estep_api.hip schedule_corpus)
    std::vector<int32_t> order((size_t)D);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return doc_ptr[a + 1] - doc_ptr[a] > doc_ptr[b + 1] - doc_ptr[b]; });
    std::vector<int32_t> sorted((size_t)D);
    for (int64_t i = 0; i < D; ++i) sorted[(size_t)i] = (int32_t)(doc_ptr[order[(size_t)i] + 1] - doc_ptr[order[(size_t)i]]);
    const std::vector<Launch> plan = build_launch_classes(cfg, sorted.data(), D);
    const QuadSlotLayout q = quad_slot_layout(plan);
    REQUIRE(q.rec_first.size() == plan.size() && q.ids_first.size() == plan.size() && q.ids_stride.size() == plan.size(), "sizes");

    // exactly-sized device stand-ins; -2: never written
    QuadSlot* rec = (QuadSlot*)malloc(q.records ? (size_t)q.records * sizeof(QuadSlot) : 1);
    int32_t* ids = (int32_t*)malloc(q.ids ? (size_t)q.ids * sizeof(int32_t) : 1);
    std::vector<char> rec_written((size_t)q.records, 0);
    for (int64_t i = 0; i < q.ids; ++i) ids[i] = -2;
    int rc = 0;
    int64_t records = 0, nids = 0, bytes = 0;
    for (size_t j = 0; j < plan.size() && !rc; ++j) {
        const Launch& L = plan[j];
        const bool packs = L.variant == kQuad && quad_tl_of(L.rn) == 32;
        if (!packs) {
            if (q.rec_first[j] != -1 || q.ids_first[j] != -1 || q.ids_stride[j] != 0) { fprintf(stderr, "class %zu has slots\n", j); rc = 1; }
            continue;
        }
        const int wpr = quad_wpr_of(L.rn), wpg = quad_wpg_of(L.rn), stride = q.ids_stride[j];
        if (q.rec_first[j] != records || q.ids_first[j] != nids || stride < wpg || stride % 4 || stride > 16 || 16 * wpg < L.n_cap) {
            fprintf(stderr, "class %zu: offsets %lld %lld stride %d\n", j, (long long)q.rec_first[j], (long long)q.ids_first[j], stride);
            rc = 1;
            break;
        }
        // the packer (prepare_kernels.h quad_pack_kernel): workgroup i, thread (gg, s)
        for (int64_t i = 0; i < L.count && !rc; ++i) {
            const int doc = order[(size_t)(L.first + i)];
            const int64_t lo = doc_ptr[(size_t)doc];
            const int N = (int)(doc_ptr[(size_t)doc + 1] - lo);
            int64_t tokens = 0;
            for (int n = 0; n < N; ++n) tokens += term_ct[(size_t)(lo + n)];
            if (rec_written[(size_t)(records + i)]++) rc = 1;
            rec[records + i] = QuadSlot{doc, N, lo, (double)tokens, 0};
            for (int gg = 0; gg < 16; ++gg)
                for (int s = 0; s < stride; ++s) {
                    const int n = s < wpg ? quad_slot_term(s, gg, wpr) : N;
                    int32_t* at = ids + nids + quad_ids_at(i, gg, stride) + s;
                    if (*at != -2) { fprintf(stderr, "class %zu slot %lld: id written twice\n", j, (long long)i); rc = 1; }
                    *at = n < N ? term_id[(size_t)(lo + n)] : -1;
                }
        }
        records += L.count;
        nids += L.count * 16 * stride;
        bytes += L.count * (32 + 16 * (int64_t)stride * 4);
    }
    if (!rc && (records != q.records || nids != q.ids || bytes != q.bytes())) { fprintf(stderr, "totals\n"); rc = 1; }
    // what the kernel reads: wid[s] of every lane group of every launch slot, against the present expression
    for (size_t j = 0; j < plan.size() && !rc; ++j) {
        if (q.rec_first[j] < 0) continue;
        const Launch& L = plan[j];
        const int wpr = quad_wpr_of(L.rn), wpg = quad_wpg_of(L.rn), stride = q.ids_stride[j];
        for (int64_t i = 0; i < L.count && !rc; ++i) {
            const QuadSlot& r = rec[q.rec_first[j] + i];
            const int doc = order[(size_t)(L.first + i)];
            if (r.doc != doc || r.lo != doc_ptr[(size_t)doc] || r.N != sorted[(size_t)(L.first + i)]) { fprintf(stderr, "record\n"); rc = 1; }
            for (int gg = 0; gg < 16 && !rc; ++gg)
                for (int s = 0; s < stride; ++s) {
                    const int n = present_term(s, gg, wpr);
                    const int32_t want = s < wpg && n < r.N ? term_id[(size_t)(r.lo + n)] : -1;
                    if (ids[q.ids_first[j] + quad_ids_at(i, gg, stride) + s] != want) {
                        fprintf(stderr, "class %zu (geometry %d) slot %lld gg %d s %d: id differs\n", j, L.rn, (long long)i, gg, s);
                        rc = 1;
                        break;
                    }
                }
        }
    }
    for (int64_t i = 0; i < q.ids && !rc; ++i) REQUIRE(ids[i] != -2, "id %lld never written", (long long)i);
    for (int64_t i = 0; i < q.records && !rc; ++i) REQUIRE(rec_written[(size_t)i] == 1, "record %lld", (long long)i);
    free(rec);
    free(ids);
    return rc;
}

int main(int argc, char** argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 100;
    static_assert(sizeof(QuadSlot) == 32 && alignof(QuadSlot) == 32, "one aligned 32-byte load");
    for (int r = 0; r < rounds; ++r)
        if (check_one()) return 1;
    printf("quad slots sanitizer run: ok (%d corpora)\n", rounds);
    return 0;
}

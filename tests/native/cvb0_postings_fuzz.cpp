// The postings builder of the collapsed variational Bayes engine (host_plan.h: cvb0_block_postings) on random corpora,
// for a build with -fsanitize=address,undefined (tests/test_cvb0_host.py).  Checks what the kernels rely on: every slot
// has exactly one posting, a round's postings ascend by (word, document), a segment holds 1 .. 256 postings of one word,
// a run's segments are those of its word, and the widest round is what the buffers are sized by.
#include "../../pylda_amd/csrc/host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace pylda_plan;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("%s:%d: %s (case %d)\n", __FILE__, __LINE__, #cond, round_); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

static int round_ = 0;

static int one_case(std::mt19937_64& rng)
{
    const int64_t D = (int64_t)(rng() % 40);
    const int V = 1 + (int)(rng() % 30);
    const int64_t blocks = 1 + (int64_t)(rng() % (rng() % 2 ? 5 : 90));
    const int64_t first_document = (int64_t)(rng() % 3 ? rng() % 50 : 0);
    const bool heavy = rng() % 4 == 0;             // many documents that share word 0: segments of 256 and more
    const int64_t documents = heavy ? 300 + (int64_t)(rng() % 600) : D;
    std::vector<int64_t> ptr(1, 0);
    std::vector<int32_t> ids;
    for (int64_t d = 0; d < documents; ++d) {
        std::vector<int32_t> words;
        for (int v = 0; v < V; ++v)
            if ((heavy && v == 0) || rng() % 5 == 0) words.push_back(v);
        for (size_t i = words.size(); i > 1; --i) std::swap(words[i - 1], words[rng() % i]);
        ids.insert(ids.end(), words.begin(), words.end());
        ptr.push_back((int64_t)ids.size());
    }
    const Cvb0Postings p = cvb0_block_postings(ptr.data(), ids.data(), documents, heavy ? 1 + (int64_t)(rng() % 3) : blocks, first_document);
    const int64_t G = heavy ? 0 : blocks;
    const int64_t nnz = (int64_t)ids.size();
    const size_t rounds = p.round_block.size();
    CHECK(p.post_ptr.size() == rounds + 1 && p.seg_ptr.size() == rounds + 1 && p.run_ptr.size() == rounds + 1);
    CHECK((int64_t)p.post_slot.size() == nnz && (int64_t)p.slot_place.size() == nnz && p.post_ptr.back() == nnz);
    CHECK((int64_t)p.seg_begin.size() == p.seg_ptr.back() + 1 && (int64_t)p.run_seg.size() == p.run_ptr.back() + 1);
    CHECK((int64_t)p.run_word.size() == p.run_ptr.back());
    std::vector<int> seen((size_t)nnz, 0);
    std::vector<int64_t> slot_doc((size_t)nnz);
    for (int64_t d = 0; d < documents; ++d)
        for (int64_t q = ptr[(size_t)d]; q < ptr[(size_t)d + 1]; ++q) slot_doc[(size_t)q] = d;
    int64_t widest_postings = 0, widest_segments = 0, covered = 0;
    for (size_t r = 0; r < rounds; ++r) {
        if (r) CHECK(p.round_block[r] > p.round_block[r - 1]);
        if (G) CHECK((first_document + p.round_first[r]) % G == p.round_block[r]);
        covered += p.round_docs[r];
        widest_postings = std::max(widest_postings, p.post_ptr[r + 1] - p.post_ptr[r]);
        widest_segments = std::max(widest_segments, p.seg_ptr[r + 1] - p.seg_ptr[r]);
        for (int64_t at = p.post_ptr[r]; at < p.post_ptr[r + 1]; ++at) {
            const int64_t q = p.post_slot[(size_t)at];
            CHECK(q >= 0 && q < nnz && !seen[(size_t)q]++);
            CHECK(p.slot_place[(size_t)q] == at - p.post_ptr[r]);
            if (at > p.post_ptr[r]) {
                const int64_t before = p.post_slot[(size_t)at - 1];
                CHECK(ids[(size_t)before] < ids[(size_t)q] || (ids[(size_t)before] == ids[(size_t)q] && slot_doc[(size_t)before] < slot_doc[(size_t)q]));
            }
        }
        CHECK(p.seg_begin[(size_t)p.seg_ptr[r]] == p.post_ptr[r] && p.seg_begin[(size_t)p.seg_ptr[r + 1]] == p.post_ptr[r + 1]);
        CHECK(p.run_seg[(size_t)p.run_ptr[r]] == p.seg_ptr[r] && p.run_seg[(size_t)p.run_ptr[r + 1]] == p.seg_ptr[r + 1]);
        for (int64_t u = p.run_ptr[r]; u < p.run_ptr[r + 1]; ++u) {
            CHECK(p.run_seg[(size_t)u + 1] > p.run_seg[(size_t)u]);
            for (int64_t s = p.run_seg[(size_t)u]; s < p.run_seg[(size_t)u + 1]; ++s) {
                const int64_t lo = p.seg_begin[(size_t)s], hi = p.seg_begin[(size_t)s + 1];
                CHECK(hi > lo && hi - lo <= kCvb0Segment);
                if (s + 1 < p.run_seg[(size_t)u + 1]) CHECK(hi - lo == kCvb0Segment);
                for (int64_t at = lo; at < hi; ++at) CHECK(ids[(size_t)p.post_slot[(size_t)at]] == p.run_word[(size_t)u]);
            }
            if (u > p.run_ptr[r]) CHECK(p.run_word[(size_t)u] > p.run_word[(size_t)u - 1]);
        }
    }
    CHECK(covered == documents);
    CHECK(widest_postings == p.widest_postings && widest_segments == p.widest_segments);
    return 0;
}

int main(int argc, char** argv)
{
    const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
    std::mt19937_64 rng(20240611);
    for (round_ = 0; round_ < cases; ++round_)
        if (one_case(rng)) return 1;
    std::printf("cvb0 postings sanitizer run: ok (%d cases)\n", cases);
    return 0;
}

// What every thread of a stride-256 document stores into a column of the hand-over tile (pylda_amd/csrc/estep_limits.h
// quad_pair_store, the function the kernel itself goes by), as a table for tests/test_quad_handover_pairs_host.py:
//     quad_pairs_table WPR WPG      ->  stdout: int16 {term, bytes} for N = 1 .. 256, tid = 0 .. 511, q = 0 .. stores - 1
// Plain C++: built with the host compiler, runs anywhere.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pylda_amd/csrc/estep_limits.h"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const int wpr = std::atoi(argv[1]), wpg = std::atoi(argv[2]);
    const int stores = pylda::quad_pair_stores(wpr, wpg);
    std::vector<int16_t> out;
    out.reserve((size_t)256 * 512 * stores * 2);
    for (int N = 1; N <= 256; ++N)
        for (int tid = 0; tid < 512; ++tid)
            for (int q = 0; q < stores; ++q) {
                const pylda::QuadPairStore w = pylda::quad_pair_store(N, wpr, wpg, tid, q);
                out.push_back((int16_t)w.term);
                out.push_back((int16_t)w.bytes);
            }
    return std::fwrite(out.data(), sizeof(int16_t), out.size(), stdout) == out.size() ? 0 : 1;
}

// A wavefront's sorted list of its best entries, kept in registers: lane j holds entry j of the list as (value, id).
// The order is total - larger value first, among equal values the smaller id - so the first M of any set of entries with
// distinct ids is a set with a position for each member, whatever the order the entries are offered in.
// Shared by the top words of a topic (coherence_kernels.h) and the nearest documents of a query
// (similarity_kernels.h, section 18).
#pragma once
#include "estep_common.h"

namespace pylda {

// a before b: larger value first, among equal values the smaller id
__device__ __forceinline__ bool coherence_before(double av, int ai, double bv, int bi)
{
    return av > bv || (av == bv && ai < bi);
}

// One candidate into the wavefront's sorted list (lane j: entry j).  c_v / c_i are wave-uniform.
__device__ __forceinline__ void coherence_insert(double& lv, int& li, double c_v, int c_i, int lane)
{
    const int rank = __popcll(__ballot(coherence_before(lv, li, c_v, c_i)));    // entries that stay in front of it
    const double up_v = __hiloint2double(__shfl_up(__double2hiint(lv), 1, kWave), __shfl_up(__double2loint(lv), 1, kWave));
    const int up_i = __shfl_up(li, 1, kWave);
    if (lane == rank) {
        lv = c_v;
        li = c_i;
    } else if (lane > rank) {
        lv = up_v;
        li = up_i;
    }
}

// The elements x (word id v; id < 0: none) of the 64 lanes against the list: those before the threshold go in one by one.
__device__ __forceinline__ void coherence_offer(double& lv, int& li, double& thr_v, int& thr_i, double x, int v, int M, int lane)
{
    unsigned long long todo = __ballot(v >= 0 && coherence_before(x, v, thr_v, thr_i));
    while (todo) {                                                      // (wave-uniform)
        const int src = __builtin_ctzll(todo);
        coherence_insert(lv, li, readlane_f64(x, src), __builtin_amdgcn_readlane(v, src), lane);
        thr_v = readlane_f64(lv, M - 1);
        thr_i = __builtin_amdgcn_readlane(li, M - 1);
        todo &= todo - 1;
        todo &= __ballot(v >= 0 && coherence_before(x, v, thr_v, thr_i));   // (the threshold rose: some no longer qualify)
    }
}

}  // namespace pylda

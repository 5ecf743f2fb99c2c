// fp64 sums and lane reads of a wave (64 lanes), shared by csrc/neighbors.hip (LISI) and csrc/tsne.hip (the perplexity solve and the
// sparse rows): every sum over the lanes is one fixed xor tree, so it is the same bits in every lane and from run to run.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ double wave_sum(double v) {     // (a + b and b + a are the same bits: every lane ends with the same sum)
    v += __shfl_xor(v, 32);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}
__device__ __forceinline__ double lane_value(double v, int src) {
    const long long b = __builtin_bit_cast(long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), src);
    return __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
}

}  // namespace

// The search both pair kernels share (csrc/tsne.hip tsne_mutual_kernel, csrc/umap.hip umap_mutual_kernel): is cell i in the list of
// its neighbour j, and with which value.
#pragma once
#include "common.h"

namespace {

// j = idx[i, slot].  Walks list(j) (K entries of idx, nearest first) for i: returns 1 and the value v[j, s] of the first slot s that
// holds i in `other`, else 0 and other = 0.  A j outside [0, N) has no list.
__device__ __forceinline__ int mutual_search(const int32_t* __restrict__ idx, const float* __restrict__ v, long long N, int K,
                                             long long i, long long j, double& other) {
    other = 0.0;
    if (j < 0 || j >= N) return 0;
    for (int s = 0; s < K; ++s)
        if (idx[j * K + s] == i) {
            other = (double)v[j * K + s];
            return 1;
        }
    return 0;
}

}  // namespace

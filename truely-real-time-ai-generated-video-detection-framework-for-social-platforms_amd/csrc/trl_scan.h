// trl_scan.h -- the exclusive scan of one 1,024-thread workgroup's per-thread partial sums (k_cluster_number, k_range_scan).
#pragma once
#include <hip/hip_runtime.h>

// every thread of a 1,024-thread workgroup hands in its partial sum c and gets the sum of the threads below it; thread 1,023's result
// + its c is the total.  Met by all 1,024 threads (barriers), once per kernel (the 1,024 sums live in static LDS).
template <typename T>
__device__ __forceinline__ T trl_scan_1024(T c) {
    __shared__ T part[1024];
    const int t = threadIdx.x;
    part[t] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const T add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    return part[t] - c;
}

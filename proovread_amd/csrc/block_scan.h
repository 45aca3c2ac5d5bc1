// Inclusive prefix sum over a block of BLK threads (device only): every thread calls it with
// its value and the block's int sh[BLK] in LDS; sh[BLK - 1] holds the total until the next call.
#pragma once
#include <hip/hip_runtime.h>

namespace prgpu {

template <int BLK>
__device__ inline int block_scan(int v, int *sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int st = 1; st < BLK; st <<= 1) {
        const int x = tid >= st ? sh[tid - st] : 0;
        __syncthreads();
        sh[tid] += x;
        __syncthreads();
    }
    return sh[tid];
}

}   // namespace prgpu

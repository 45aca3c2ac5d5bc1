// The hand-off's coordinate sort for long reads whose alignments outgrow the LDS sort of
// pipe_sort_kernel (more than handp::LDS_KEYS tasks: handoff_plan.h).  samtools sort and
// bam2cns's per-read region query take any number of records (bin/proovread:1330-1355,
// bin/bam2cns:336-354); here a read's keys go through HBM:
//
//   pipe_big_runs_kernel  : a workgroup per run of LDS_KEYS consecutive tasks: the keys of the
//                           reported ones, (POS << 33 | strand << 32 | task index within the
//                           read) as in pipe_sort_kernel, bitonic-sorted in LDS and written to
//                           the run's slots of the key buffer; the slots of the tasks that are
//                           not reported hold ~0 and sort to the run's end
//   pipe_big_merge_kernel : one pairwise merge pass (runs of `w` keys -> runs of 2w) from one
//                           key buffer to the other; a thread finds where its 8 outputs start
//                           in the two runs by binary search along the merge path's diagonal
//   pipe_big_write_kernel : the consensus-stage alignment arrays of the first cnt keys (the
//                           ~0 slots are last), exactly as pipe_sort_kernel writes them
//
// The task index makes every key unique, so the order is determined: it is the stable coordinate
// order of the LDS path whatever the run boundaries.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "handoff_plan.h"
#include "pipe_dev.h"

namespace prgpu {

constexpr int BIG_SORT_THREADS = 1024;   // 128 KB of keys: one workgroup per CU, 16 waves on it
constexpr int BIG_THREADS = 256;
constexpr int BIG_PER_THREAD = handp::MERGE_TILE / BIG_THREADS;
constexpr unsigned long long BIG_NONE = ~0ULL;   // no key: POS << 33 of a real key leaves index bits < 2^20

// the read of this block row and its slice of the key buffers; false: the host's count differs
// from the device's task_off (flagged, the read is skipped by every kernel)
__device__ inline bool big_read(const PipeDev &P, const PipeBig &G, int b, int &lr, int64_t &t0, int64_t &nt, int64_t &k0) {
    lr = G.lr[b];
    t0 = P.task_off[lr];
    nt = P.task_off[lr + 1] - t0;
    k0 = G.off[b];
    return nt == G.off[b + 1] - k0;
}

__global__ void __launch_bounds__(BIG_SORT_THREADS) pipe_big_runs_kernel(PipeDev P, PipeBig G) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
    __shared__ int s_n;
    for (int b = blockIdx.y; b < G.n_big; b += gridDim.y) {
        int lr;
        int64_t t0, nt, k0;
        if (!big_read(P, G, b, lr, t0, nt, k0)) {
            if (threadIdx.x == 0 && blockIdx.x == 0) P.err[lr] = 3;
            continue;
        }
        unsigned long long *out = G.k0 + k0;
        const int nruns = (int)((nt + handp::LDS_KEYS - 1) / handp::LDS_KEYS);
        for (int run = blockIdx.x; run < nruns; run += gridDim.x) {
            const int64_t i0 = (int64_t)run * handp::LDS_KEYS;
            const int m = (int)(nt - i0 < handp::LDS_KEYS ? nt - i0 : handp::LDS_KEYS);
            if (threadIdx.x == 0) s_n = 0;
            for (int i = threadIdx.x; i < handp::LDS_KEYS; i += BIG_SORT_THREADS) keys[i] = BIG_NONE;
            __syncthreads();
            for (int i = threadIdx.x; i < m; i += BIG_SORT_THREADS) {
                const int64_t t = t0 + i0 + i;
                if (!(P.pass[t] && P.status[t] == 0 && (!P.keep || P.keep[t]))) continue;
                const int slot = atomicAdd(&s_n, 1);
                keys[slot] = ((unsigned long long)(uint32_t)P.pos[t] << 33) |
                             ((unsigned long long)(P.strand[t] & 1u) << 32) | (unsigned long long)(uint32_t)(i0 + i);
            }
            __syncthreads();
            int n2 = 1;
            while (n2 < s_n) n2 <<= 1;
            // bitonic sort ascending (the ~0 padding stays behind the keys)
            for (int k = 2; k <= n2; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = threadIdx.x; i < n2; i += BIG_SORT_THREADS) {
                        const int ixj = i ^ j;
                        if (ixj > i) {
                            const unsigned long long x = keys[i], y = keys[ixj];
                            const bool up = (i & k) == 0;
                            if ((x > y) == up) { keys[i] = y; keys[ixj] = x; }
                        }
                    }
                    __syncthreads();
                }
            }
            for (int i = threadIdx.x; i < m; i += BIG_SORT_THREADS) out[i0 + i] = keys[i];
            __syncthreads();
        }
    }
}

// runs of w keys in src, pairs of them merged into runs of 2w keys in dst (a last run without a
// partner is copied: the merge with an empty second run)
__global__ void __launch_bounds__(BIG_THREADS) pipe_big_merge_kernel(PipeDev P, PipeBig G, const unsigned long long *src,
                                                                     unsigned long long *dst, int64_t w) {
    for (int b = blockIdx.y; b < G.n_big; b += gridDim.y) {
        int lr;
        int64_t t0, n, k0;
        if (!big_read(P, G, b, lr, t0, n, k0)) continue;
        const unsigned long long *rsrc = src + k0;
        unsigned long long *rdst = dst + k0;
        const int64_t ntile = (n + handp::MERGE_TILE - 1) / handp::MERGE_TILE;
        for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
            // this thread's outputs [o0, o1): within one pair of runs (2w is a multiple of the 8)
            const int64_t o0 = tile * handp::MERGE_TILE + (int64_t)threadIdx.x * BIG_PER_THREAD;
            if (o0 >= n) continue;
            const int64_t o1 = o0 + BIG_PER_THREAD < n ? o0 + BIG_PER_THREAD : n;
            const int64_t base = o0 / (2 * w) * (2 * w);
            const int64_t a1 = base + w < n ? base + w : n, b1 = base + 2 * w < n ? base + 2 * w : n;
            const unsigned long long *A = rsrc + base, *B = rsrc + a1;
            const int64_t la = a1 - base, lb = b1 - a1, d = o0 - base;
            // merge path: i = keys of A among the first d outputs (A first on ties), d - i those of B
            int64_t lo = d - lb > 0 ? d - lb : 0, hi = d < la ? d : la;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (A[mid] <= B[d - mid - 1]) lo = mid + 1;
                else hi = mid;
            }
            int64_t i = lo, j = d - lo;
            for (int64_t o = o0; o < o1; ++o) {
                const bool from_a = j >= lb || (i < la && A[i] <= B[j]);
                rdst[o] = from_a ? A[i++] : B[j++];
            }
        }
    }
}

__global__ void __launch_bounds__(BIG_THREADS) pipe_big_write_kernel(PipeDev P, PipeBig G, const unsigned long long *sorted) {
    for (int b = blockIdx.y; b < G.n_big; b += gridDim.y) {
        int lr;
        int64_t t0, nt, k0;
        if (!big_read(P, G, b, lr, t0, nt, k0)) continue;
        const unsigned long long *rs = sorted + k0;
        const int64_t cnt = P.cnt[lr];   // <= nt: pipe_count_kernel's count under the same predicate
        const int64_t a0 = P.aln_off[lr];
        for (int64_t r = (int64_t)blockIdx.x * BIG_THREADS + threadIdx.x; r < cnt && r < nt; r += (int64_t)gridDim.x * BIG_THREADS) {
            const unsigned long long key = rs[r];
            const int64_t i = (int64_t)(key & 0xFFFFFFFFull);
            if (key == BIG_NONE || i >= nt) {   // cannot happen: the first cnt keys are the reported tasks'
                P.err[lr] = 4;
                continue;
            }
            const int64_t t = t0 + i;
            const int64_t g = a0 + r;
            const int sid = P.t_sr[t];
            P.a_pos[g] = P.pos[t] + 1;
            P.a_score[g] = (double)P.score[t];
            P.a_flags[g] = (uint8_t)(1u | (P.strand[t] ? 8u : 0u));   // HAS_SCORE | REVCOMP
            P.a_seq_off[g] = P.sr_off[sid];
            P.a_lseq[g] = (int32_t)(P.sr_off[sid + 1] - P.sr_off[sid]);
            P.a_cig_off[g] = P.cig_at[t];
            P.a_ncig[g] = P.ncig[t];
            P.a_task[g] = (int32_t)i;
        }
    }
}

int pipe_big_launch(const PipeDev &P, const PipeBig &G, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const int lds = handp::LDS_KEYS * 8;
    const unsigned rows = (unsigned)(G.n_big < 65535 ? G.n_big : 65535);   // block rows: the kernels stride over the reads
    hipError_t e = hipFuncSetAttribute((const void *)pipe_big_runs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(pipe_big_runs_kernel, dim3((unsigned)G.max_runs, rows), dim3(BIG_SORT_THREADS), lds, s, P, G);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    int64_t tiles = (G.max_big + handp::MERGE_TILE - 1) / handp::MERGE_TILE;
    tiles = tiles < 512 ? tiles : 512;   // (2^20 keys: 512 tiles; more reads: more block rows)
    const dim3 grid((unsigned)tiles, rows);
    unsigned long long *src = G.k0, *dst = G.k1;
    for (int p = 0; p < G.passes; ++p) {
        hipLaunchKernelGGL(pipe_big_merge_kernel, grid, dim3(BIG_THREADS), 0, s, P, G, (const unsigned long long *)src, dst,
                           (int64_t)handp::LDS_KEYS << p);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        unsigned long long *x = src;
        src = dst;
        dst = x;
    }
    hipLaunchKernelGGL(pipe_big_write_kernel, grid, dim3(BIG_THREADS), 0, s, P, G, (const unsigned long long *)src);
    return (int)hipGetLastError();
}

}  // namespace prgpu

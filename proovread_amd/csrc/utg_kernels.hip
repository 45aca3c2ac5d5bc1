// The unitig consensus on the device (bam2cns --utg-mode), gfx950, wave64.
// Every rule is utg_core.h's; the kernels only spread them:
//   utg_prep_kernel       a thread per alignment: CIGAR checks, trim, op prefixes, length,
//                         score and step 1 (Seq.pm:275-385, 919-927)
//   utg_cov_kernel        a block per read: +1 / -1 at the span ends, a prefix sum over column
//                         tiles for the exact coverage, the runs compacted into the windows of
//                         step 4 and, widened, tested against every alignment for step 2
//                         (Seq.pm:949-999, bam2cns:398-422)
//   utg_contained_kernel  a wave per read: rank sort by length, the pop loop of Seq.pm:1017-1046
//                         kept serial with the range test spread over the lanes; up to
//                         FILTER_LDS alignments in LDS, more through HBM
//   utg_cns_kernel        a block per read: the consensus's and the ranks' alignment lists by
//                         ordered compaction, then a thread per column over tiles of 256; a tile
//                         first lists the alignments that reach it (LDS), a column walks that
//                         list in arrival order; output by block prefix sums
//   utg_pack_kernel       the outputs gathered for one download
// Integer atomics only (the difference array); all stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "utg_dev.h"

namespace prgpu {

using namespace utg;

namespace {

constexpr int BLK = 256;
constexpr int TILE_CAP = 1024;   // alignments a tile lists in LDS; more: the columns walk the read's list

__global__ __launch_bounds__(BLK) void utg_prep_kernel(View V) {
    const int64_t a = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (a >= V.b.n_alns) return;
    const int r = V.aln_read[a];
    if (V.o.status[r]) {
        V.flag[a] = 0;
        V.prep[a] = Prep{0, 0, 0, 0, 0, 0, 0};
        return;
    }
    prep_one(V, a, read_len(V.b, r));
}

__global__ __launch_bounds__(BLK) void utg_cov_kernel(View V) {
    __shared__ int sh[BLK];
    __shared__ int hs[BLK];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (V.o.status[r]) return;
    const pr_utg_batch &b = V.b;
    const int L = read_len(b, r);
    const int64_t a0 = b.aln_off[r];
    const int na = (int)(b.aln_off[r + 1] - a0);
    const bool rep = V.p.has_rep_coverage != 0;
    int bad = 0;
    for (int k = tid; k < na; k += BLK) {
        const int f = V.flag[a0 + k];
        bad |= (f & F_DIV0) != 0;
        if (rep && (f & F_ALIVE1)) bad |= V.prep[a0 + k].use < 0;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) V.o.status[r] = PR_UTG_BAD_ALN;
        return;
    }
    if (!rep) {
        for (int k = tid; k < na; k += BLK)
            if (V.flag[a0 + k] & F_ALIVE1) V.flag[a0 + k] |= F_ALIVE2;
        return;
    }
    int32_t *cov = V.cov + b.read_off[r] + r;
    for (int c = tid; c <= L; c += BLK) cov[c] = 0;
    __threadfence_block();
    __syncthreads();
    for (int k = tid; k < na; k += BLK)
        if ((V.flag[a0 + k] & F_ALIVE1) && V.prep[a0 + k].use == 1) {
            atomicAdd(&cov[V.prep[a0 + k].rpos], 1);
            atomicAdd(&cov[V.span_e[a0 + k]], -1);
        }
    __threadfence_block();
    __syncthreads();
    int32_t *win = V.o.win + 2 * b.win_off[r];
    const int wcap = (int)(b.win_off[r + 1] - b.win_off[r]);
    int carry = 0, prev_high = 0, nw = 0;
    // column L closes a run that reaches the end (bam2cns:421)
    for (int base = 0; base <= L; base += BLK) {
        const int c = base + tid;
        const int cv = carry + block_scan<BLK>(c < L ? cov[c] : 0, sh);
        const int total = sh[BLK - 1];
        const int h = c < L && !(cv < V.p.rep_coverage);
        hs[tid] = h;
        __syncthreads();
        const int prev = tid ? hs[tid - 1] : prev_high;
        const int last = hs[BLK - 1];
        const int st = h && !prev, en = !h && prev && c <= L;
        const int si = nw + block_scan<BLK>(st, sh);   // starts up to and with this column
        const int nst = sh[BLK - 1];
        if (st && si - 1 < wcap) win[2 * (si - 1)] = c;
        if (en && si - 1 < wcap) win[2 * (si - 1) + 1] = c;
        carry += total, prev_high = last, nw += nst;
        __syncthreads();
    }
    if (nw > wcap) nw = wcap;
    __threadfence_block();
    __syncthreads();
    for (int k = tid; k < nw; k += BLK) win[2 * k + 1] -= win[2 * k];
    if (tid == 0) V.o.n_win[r] = nw;
    __threadfence_block();
    __syncthreads();
    for (int k = tid; k < na; k += BLK)
        if ((V.flag[a0 + k] & F_ALIVE1) && !(nw && in_rwins(win, nw, L, b.pos[a0 + k], V.alen[a0 + k]))) V.flag[a0 + k] |= F_ALIVE2;
}

__global__ __launch_bounds__(64) void utg_contained_kernel(View V) {
    __shared__ int32_t s_pos[FILTER_LDS], s_len[FILTER_LDS], s_id[FILTER_LDS];
    __shared__ double s_sc[FILTER_LDS];
    const int r = blockIdx.x, lane = threadIdx.x;
    if (V.o.status[r]) return;
    const pr_utg_batch &b = V.b;
    const int64_t a0 = b.aln_off[r];
    const int na = (int)(b.aln_off[r + 1] - a0);
    // the alignments alive after step 2, in arrival order: members in ulist, lengths in rlist
    int32_t *mem = V.ulist + a0, *lens = V.rlist + a0;
    int n = 0;
    for (int base = 0; base < na; base += 64) {
        const int k = base + lane;
        const bool alive = k < na && (V.flag[a0 + k] & F_ALIVE2);
        const unsigned long long mask = __ballot(alive);
        if (alive) {
            const int at = n + __popcll(mask & ((1ull << lane) - 1ull));
            mem[at] = k, lens[at] = V.alen[a0 + k];
            V.flag[a0 + k] |= F_KEPT;
        }
        n += __popcll(mask);
    }
    __threadfence_block();
    __syncthreads();
    const bool on_chip = n <= FILTER_LDS;
    int32_t *fp = on_chip ? s_pos : V.f_pos + a0, *fl = on_chip ? s_len : V.f_len + a0, *fi = on_chip ? s_id : V.f_id + a0;
    double *fs = on_chip ? s_sc : V.f_sc + a0;
    // descending by length, ties in arrival order
    for (int i = lane; i < n; i += 64) {
        const int li = lens[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const int lj = lens[j];
            rank += lj > li || (lj == li && j < i);
        }
        const int k = mem[i];
        fp[rank] = b.pos[a0 + k], fl[rank] = li, fs[rank] = V.sc[a0 + k], fi[rank] = k;
    }
    __threadfence_block();
    __syncthreads();
    // every lane runs the pop loop on the same values; the lanes share the range test
    contained_pop(
        n, fp, fl, fs, fi,
        [&](long cp, long cl, int m) {
            bool hit = false;
            for (int k = lane; k < m; k += 64) hit |= range_inside(cp, cl, fp[k], fl[k]);
            return __any(hit) != 0;
        },
        [&](int id) {
            if (lane == 0) V.flag[a0 + id] &= (uint8_t)~F_KEPT;
        });
}

__global__ __launch_bounds__(BLK) void utg_cns_kernel(View V) {
    __shared__ int sh_a[BLK], sh_b[BLK];
    __shared__ int32_t tile[TILE_CAP];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (V.o.status[r]) return;
    const pr_utg_batch &b = V.b;
    const int L = read_len(b, r);
    const int64_t a0 = b.aln_off[r];
    const int na = (int)(b.aln_off[r + 1] - a0);
    int32_t *ulist = V.ulist + a0, *rlist = V.rlist + a0;
    int nu = 0, nr = 0, bad = 0;
    for (int base = 0; base < na; base += BLK) {
        const int k = base + tid;
        const int64_t a = a0 + k;
        int u = 0, rk = 0;
        if (k < na) {
            const int kept = (V.flag[a] & F_KEPT) != 0, use = V.prep[a].use;
            V.o.kept[a] = (uint8_t)kept;
            bad |= kept && use < 0;
            u = kept && use == 1, rk = in_rank_pass(V, a) && use == 1;
        }
        const int ui = nu + block_scan<BLK>(u, sh_a), ri = nr + block_scan<BLK>(rk, sh_b);
        if (u) ulist[ui - 1] = (int32_t)a;
        if (rk) rlist[ri - 1] = (int32_t)a;
        nu += sh_a[BLK - 1], nr += sh_b[BLK - 1];
    }
    if (__syncthreads_or(bad)) {
        for (int k = tid; k < na; k += BLK) V.o.kept[a0 + k] = 0;
        if (tid == 0) V.o.status[r] = PR_UTG_BAD_ALN, V.o.n_win[r] = 0;
        return;
    }
    if (tid == 0) V.n_u[r] = nu, V.n_r[r] = nr;
    __threadfence_block();
    __syncthreads();
    const Read ref = ref_of(b, r);
    const int64_t ob = b.out_off[r], cap = b.out_off[r + 1] - ob;
    int seq_base = 0, trace_base = 0;
    for (int base = 0; base < L; base += BLK) {
        // the alignments that reach this tile, still in arrival order
        int mt = 0;
        for (int kb = 0; kb < nu; kb += BLK) {
            const int k = kb + tid;
            const int32_t a = k < nu ? ulist[k] : -1;
            const int ov = a >= 0 && V.prep[a].rpos < base + BLK && V.span_e[a] > base;
            const int at = mt + block_scan<BLK>(ov, sh_a);
            if (ov && at - 1 < TILE_CAP) tile[at - 1] = a;
            mt += sh_a[BLK - 1];
        }
        __syncthreads();
        const OpSrc src = {V, r, mt <= TILE_CAP ? tile : ulist, mt <= TILE_CAP ? mt : nu};
        const int c = base + tid;
        Pick pk = {0, 0, -1, 0.0, 0, 0};
        int nseq = 0, ntrace = 0;
        if (c < L) {
            pk = decide_col(V.sp, ref, c, src);
            pick_len(pk, nseq, ntrace);
        }
        const int so = seq_base + block_scan<BLK>(nseq, sh_a) - nseq, to = trace_base + block_scan<BLK>(ntrace, sh_b) - ntrace;
        if (c < L && so + nseq <= cap && to + ntrace <= cap)
            pick_emit(V.sp, pk, ref, c, src, V.o.seq + ob + so, V.o.qual + ob + so, V.o.trace + ob + to);
        seq_base += sh_a[BLK - 1], trace_base += sh_b[BLK - 1];
        __syncthreads();
    }
    if (tid == 0) V.o.seq_len[r] = seq_base, V.o.trace_len[r] = trace_base;
}

__global__ __launch_bounds__(BLK) void utg_pack_kernel(View V, UtgPackDev P) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const int64_t ob = V.b.out_off[r];
    const int ns = V.o.seq_len[r], nt = V.o.trace_len[r];
    for (int x = tid; x < ns; x += BLK) P.seq[P.seq_at[r] + x] = V.o.seq[ob + x], P.qual[P.seq_at[r] + x] = V.o.qual[ob + x];
    for (int x = tid; x < nt; x += BLK) P.trace[P.trace_at[r] + x] = V.o.trace[ob + x];
}

}   // namespace

int utg_prep_launch(const View &V, void *stream) {
    if (V.b.n_alns <= 0) return (int)hipSuccess;
    hipLaunchKernelGGL(utg_prep_kernel, dim3((unsigned)((V.b.n_alns + BLK - 1) / BLK)), dim3(BLK), 0, (hipStream_t)stream, V);
    return (int)hipGetLastError();
}
int utg_cov_launch(const View &V, void *stream) {
    hipLaunchKernelGGL(utg_cov_kernel, dim3((unsigned)V.b.n_reads), dim3(BLK), 0, (hipStream_t)stream, V);
    return (int)hipGetLastError();
}
int utg_contained_launch(const View &V, void *stream) {
    hipLaunchKernelGGL(utg_contained_kernel, dim3((unsigned)V.b.n_reads), dim3(64), 0, (hipStream_t)stream, V);
    return (int)hipGetLastError();
}
int utg_cns_launch(const View &V, void *stream) {
    hipLaunchKernelGGL(utg_cns_kernel, dim3((unsigned)V.b.n_reads), dim3(BLK), 0, (hipStream_t)stream, V);
    return (int)hipGetLastError();
}
int utg_pack_launch(const View &V, const UtgPackDev &P, void *stream) {
    hipLaunchKernelGGL(utg_pack_kernel, dim3((unsigned)V.b.n_reads), dim3(BLK), 0, (hipStream_t)stream, V, P);
    return (int)hipGetLastError();
}

}   // namespace prgpu

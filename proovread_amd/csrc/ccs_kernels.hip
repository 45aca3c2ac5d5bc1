// ccs-1 on the device (ccs_core.h states the rules).
//
//   ccs_seeds_kernel   one block per (subread, reference): both sequences as nt4 codes in LDS,
//                      one lane per diagonal per step walks its cells for maximal runs >= k;
//                      a run adds its length to its bucket's sum and offers its order key to
//                      the bucket's maximum (integer atomics: the result does not depend on
//                      their order).  The block then reduces the pair sums to the winner.
//   ccs_align_kernel   one wave per pair.  A row of the band is split into runs of consecutive
//                      cells per lane; the previous row's H and E are in LDS.  Gaps open from
//                      the diagonal value only (ksw_global2), so F of a row is a prefix maximum
//                      over values the previous row fixes: each lane scans its run, the lanes'
//                      carries meet in a wave prefix maximum, a second pass fills the cells.
//                      Direction bytes go to the pair's HBM slab.  The traceback is walked by
//                      all lanes alike; a row's bytes are fetched wave-wide into LDS once.
//   ccs_cns_kernel     one block per group.  A thread per alignment trims it (prep_aln) and
//                      lists where every CIGAR op starts; the ops are then expanded op-parallel
//                      into per-column (query offset, state length, weight) maps; a thread per
//                      column adds the weights in arrival order (decide_col) and the states are
//                      written out through a block prefix sum.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "ccs_dev.h"

namespace prgpu {
namespace {

using namespace ccs;

constexpr int SEED_BLOCK = 256, CNS_BLOCK = 256;

__device__ inline Read read_of(const CcsDev &D, int s, int rev) {
    return Read{D.seq + D.off[s], D.qual + D.off[s], (int32_t)(D.off[s + 1] - D.off[s]), rev};
}

__global__ __launch_bounds__(SEED_BLOCK) void ccs_seeds_kernel(CcsDev D, CcsMapDev M) {
    __shared__ uint8_t rc[PR_CCS_MAX_LEN], qc[PR_CCS_MAX_LEN];
    __shared__ PairBest red[SEED_BLOCK];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const Read R = read_of(D, M.pair_ref[pair], 0);
    Read Q = read_of(D, M.pair_sub[pair], 0);
    const int lr = R.len, lq = Q.len, w = D.p.w, k = D.p.k;
    if (lr < 1 || lq < 1 || lr > PR_CCS_MAX_LEN || lq > PR_CCS_MAX_LEN) {
        if (tid == 0) M.centre[pair] = Centre{0, 0, 0};
        return;
    }
    const int nb = n_buckets(lr, lq, w);
    uint32_t *sum = M.bsum + M.b_off[pair];
    uint64_t *key = M.bkey + M.b_off[pair];
    for (int i = tid; i < lr; i += SEED_BLOCK) rc[i] = (uint8_t)code_at(R, i);
    for (int o = 0; o < 2; ++o) {
        Q.rev = o;
        __syncthreads();
        for (int j = tid; j < lq; j += SEED_BLOCK) qc[j] = (uint8_t)code_at(Q, j);
        __syncthreads();
        uint32_t *so = sum + (size_t)o * (nb + 1);
        unsigned long long *ko = (unsigned long long *)(key + (size_t)o * (nb + 1));
        for (int ds = tid; ds < lr + lq - 1; ds += SEED_BLOCK) {
            const int b = ds / w;
            diag_seeds([&](int i) { return (int)rc[i]; }, lr, [&](int j) { return (int)qc[j]; }, lq, ds - (lq - 1), k,
                       [&](int i, int len) {
                           atomicAdd(&so[b], (uint32_t)len);
                           atomicMax(&ko[b], (unsigned long long)seed_key(len, i, ds));
                       });
        }
    }
    __threadfence();
    __syncthreads();
    PairBest best = {0, 0, 0};
    for (int x = tid; x < 2 * nb; x += SEED_BLOCK) {   // ascending (orientation, bucket) per thread
        const int o = x / nb, b = x - o * nb;
        const uint32_t *so = sum + (size_t)o * (nb + 1);
        const PairBest c = {__atomic_load_n(&so[b], __ATOMIC_RELAXED) + __atomic_load_n(&so[b + 1], __ATOMIC_RELAXED), o, b};
        if (c.sum > best.sum) best = c;
    }
    red[tid] = best;
    __syncthreads();
    for (int st = SEED_BLOCK / 2; st > 0; st >>= 1) {
        if (tid < st && red[tid + st].sum && (!red[tid].sum || pair_better(red[tid + st], red[tid]))) red[tid] = red[tid + st];
        __syncthreads();
    }
    if (tid == 0) {
        Centre c = {0, 0, 0};
        best = red[0];
        if (best.sum) {
            const uint64_t *ko = key + (size_t)best.rev * (nb + 1);
            const uint64_t k0 = __atomic_load_n(&ko[best.b], __ATOMIC_RELAXED), k1 = __atomic_load_n(&ko[best.b + 1], __ATOMIC_RELAXED);
            c.found = 1, c.rev = best.rev, c.d0 = key_dshift(k0 > k1 ? k0 : k1) - (lq - 1);
        }
        M.centre[pair] = c;
    }
}

__global__ __launch_bounds__(64) void ccs_align_kernel(CcsDev D, CcsMapDev M) {
    extern __shared__ int32_t sm[];
    const int pair = M.first + blockIdx.x, lane = threadIdx.x;
    const int s = M.pair_sub[pair];
    const Centre ce = M.centre[pair];
    const pr_ccs_params p = D.p;
    const Read R = read_of(D, M.pair_ref[pair], 0), Q = read_of(D, s, ce.rev);
    const int lr = R.len, lq = Q.len, w = p.w, W = 2 * w + 1, d0 = ce.d0;
    const int i0 = row_lo(d0, w), i1 = row_hi(lr, lq, d0, w);
    if (!ce.found || i1 < i0) {
        if (lane == 0) D.mapped[s] = 0, D.strand[s] = 0, D.pos[s] = 0, D.score[s] = 0, D.n_cigar[s] = 0;
        return;
    }
    // H / E of two rows, W + 1 entries each (entry W: the cell right of the band), then a row of directions
    int32_t *Hb = sm, *Eb = sm + 2 * (W + 1);
    uint8_t *rowbuf = (uint8_t *)(sm + 4 * (W + 1));
    uint8_t *dir = M.dir + M.dir_off[pair];
    const int C = (W + 1 + 63) / 64, b0 = lane * C;
    for (int c = 0; c < C; ++c)
        if (b0 + c <= W) Hb[b0 + c] = 0, Eb[b0 + c] = NEG;
    __syncthreads();
    const int oe_ins = p.o_ins + p.e_ins, step = p.e_ins * C;
    int best = 0, bi = 0, bj = 0;
    for (int i = i0; i <= i1; ++i) {
        const int cur = (i - i0) & 1;
        const int32_t *Hp = Hb + cur * (W + 1), *Ep = Eb + cur * (W + 1);
        int32_t *Hn = Hb + (cur ^ 1) * (W + 1), *En = Eb + (cur ^ 1) * (W + 1);
        const int rcode = code_at(R, i), jbase = i - d0 - w;
        // F leaving this lane's run when nothing enters it
        int carry = NEG;
        for (int c = 0; c < C; ++c) {
            const int b = b0 + c, j = jbase + b;
            const int mm = (b < W && j >= 0 && j < lq) ? Hp[b] + score_of(p, rcode, code_at(Q, j)) : NEG;
            const int t = mm - oe_ins;
            carry = carry - p.e_ins > t ? carry - p.e_ins : t;
        }
        // F entering the run: the earlier lanes' carries, each decayed over the runs between
        int v = carry + step * lane;
        for (int sft = 1; sft < 64; sft <<= 1) {
            const int o = __shfl_up(v, sft);
            if (lane >= sft && o > v) v = o;
        }
        const int ex = __shfl_up(v, 1);
        int f = lane ? ex - step * (lane - 1) : NEG;
        for (int c = 0; c < C; ++c) {
            const int b = b0 + c, j = jbase + b;
            if (b < W && j >= 0 && j < lq) {
                const Cell x = dp_cell(p, Hp[b], Ep[b + 1], f, score_of(p, rcode, code_at(Q, j)));
                Hn[b] = x.h, En[b] = x.e, f = x.f;
                dir[(size_t)(i - i0) * W + b] = x.d;
                if (x.h > best) best = x.h, bi = i, bj = j;
            } else if (b <= W) {
                const int t = NEG - oe_ins;
                Hn[b] = 0, En[b] = NEG;
                f = f - p.e_ins > t ? f - p.e_ins : t;
            }
        }
        __syncthreads();
    }
    // the first maximal cell in (i, j) order
    for (int sft = 32; sft > 0; sft >>= 1) {
        const int ob = __shfl_xor(best, sft), oi = __shfl_xor(bi, sft), oj = __shfl_xor(bj, sft);
        if (ob > best || (ob == best && (oi < bi || (oi == bi && oj < bj)))) best = ob, bi = oi, bj = oj;
    }
    if (best <= 0) {
        if (lane == 0) D.mapped[s] = 0, D.strand[s] = 0, D.pos[s] = 0, D.score[s] = 0, D.n_cigar[s] = 0;
        return;
    }
    __threadfence();
    __syncthreads();
    uint32_t *cig = D.cigar + D.cig_off[s];
    const int64_t cap = D.cig_off[s + 1] - D.cig_off[s];
    int n = 0, cop = -1, clen = 0;
    auto push = [&](int op, int len) {
        if (op == cop) {
            clen += len;
            return;
        }
        if (cop >= 0 && lane == 0 && n < cap) cig[n] = (uint32_t)clen << 4 | (uint32_t)cop;
        n += cop >= 0;
        cop = op, clen = len;
    };
    if (lq - 1 - bj > 0) push(OP_S, lq - 1 - bj);
    int i = bi, j = bj, state = 0, row = -1;
    while (i >= i0 && j >= 0) {
        const int b = j - (i - d0 - w);
        if (b < 0 || b >= W) break;
        if (i != row) {
            __syncthreads();
            for (int x = lane; x < W; x += 64) rowbuf[x] = dir[(size_t)(i - i0) * W + x];
            __syncthreads();
            row = i;
        }
        const int op = tb_step(state, rowbuf[b]);
        if (op < 0) break;
        push(op, 1);
        if (op != OP_I) --i;
        if (op != OP_D) --j;
    }
    if (j + 1 > 0) push(OP_S, j + 1);
    push(-2, 0);   // flush
    if (n > cap) n = (int)cap;
    __threadfence();
    __syncthreads();
    for (int x = lane; x < n / 2; x += 64) {
        const uint32_t a = cig[x], b = cig[n - 1 - x];
        cig[x] = b, cig[n - 1 - x] = a;
    }
    if (lane == 0) D.mapped[s] = 1, D.strand[s] = ce.rev, D.pos[s] = i + 1, D.score[s] = best, D.n_cigar[s] = n;
}

__global__ __launch_bounds__(CNS_BLOCK) void ccs_cns_kernel(CcsDev D, CcsCnsDev C) {
    __shared__ Read reads[PR_CCS_MAX_SUBREADS];
    __shared__ Prep preps[PR_CCS_MAX_SUBREADS];
    __shared__ int32_t subs[PR_CCS_MAX_SUBREADS];
    __shared__ int32_t scan_a[CNS_BLOCK], scan_b[CNS_BLOCK];
    __shared__ int32_t m_sh, bad_sh;
    const int g = C.glist[blockIdx.x], tid = threadIdx.x;
    const Params p = sm_params(D.p);
    const int s0 = D.grp_off[g], ns = D.grp_off[g + 1] - s0, r = D.grp_ref[g];
    const Read ref = read_of(D, r, 0);
    const int L = ref.len;
    ColEnt *slab = C.slab + C.slab_off[blockIdx.x];
    auto view_of = [&](int s) {
        return AlnView{read_of(D, s, D.strand[s]), D.pos[s], D.cigar + D.cig_off[s], D.n_cigar[s]};
    };
    // every subread's alignment trimmed, then the kept ones listed in arrival order
    if (tid < ns && tid < PR_CCS_MAX_SUBREADS) {
        const int s = s0 + tid;
        Prep pr = {0, 0, 0, 0, 0, 0, 0};
        if (s != r && D.mapped[s]) pr = prep_aln(p, view_of(s), L);
        preps[tid] = pr;
    }
    __syncthreads();
    if (tid == 0) {
        int m = 0, bad = 0;
        for (int t = 0; t < ns && t < PR_CCS_MAX_SUBREADS; ++t) {
            const Prep pr = preps[t];
            bad |= pr.use < 0;
            if (pr.use == 1) preps[m] = pr, subs[m] = s0 + t, ++m;   // m <= t: in place
        }
        m_sh = m, bad_sh = bad;
    }
    __syncthreads();
    const int m = m_sh;
    if (bad_sh) {
        if (tid == 0) C.status[g] = PR_CCS_BAD_ALN, C.seq_len[g] = 0, C.trace_len[g] = 0;
        return;
    }
    if (tid < m) {
        const int s = subs[tid];
        const AlnView a = view_of(s);
        reads[tid] = a.q;
        const Prep pr = preps[tid];
        int rr = pr.rpos, q = 0;
        for (int i = pr.cb; i < pr.ce; ++i) {
            C.op_r[D.cig_off[s] + i] = rr, C.op_q[D.cig_off[s] + i] = q;
            advance_op(a, pr, i, rr, q);
        }
    }
    for (int64_t x = tid; x < (int64_t)m * L; x += CNS_BLOCK) slab[x] = ColEnt{-1, -1, 0.0};
    __threadfence_block();
    __syncthreads();
    for (int a = 0; a < m; ++a) {
        const int s = subs[a];
        const AlnView v = view_of(s);
        const Prep pr = preps[a];
        for (int i = pr.cb + tid; i < pr.ce; i += CNS_BLOCK)
            fill_op(p, v, pr, i, C.op_r[D.cig_off[s] + i], C.op_q[D.cig_off[s] + i], slab + (size_t)a * L);
    }
    __threadfence_block();
    __syncthreads();
    const int64_t ob = C.out_off[g], cap = C.out_off[g + 1] - ob;
    const SlabSrc src = {slab, L, m, reads};
    int seq_base = 0, trace_base = 0;
    for (int base = 0; base < L; base += CNS_BLOCK) {
        const int c = base + tid;
        Pick pk = {0, 0, -1, 0.0, 0, 0};
        int nseq = 0, ntrace = 0;
        if (c < L) {
            pk = decide_col(p, ref, c, src);
            pick_len(pk, nseq, ntrace);
        }
        const int so = seq_base + block_scan<CNS_BLOCK>(nseq, scan_a) - nseq;
        const int to = trace_base + block_scan<CNS_BLOCK>(ntrace, scan_b) - ntrace;
        if (c < L && so + nseq <= cap && to + ntrace <= cap)
            pick_emit(p, pk, ref, c, src, C.seq + ob + so, C.qual + ob + so, C.trace + ob + to);
        seq_base += scan_a[CNS_BLOCK - 1], trace_base += scan_b[CNS_BLOCK - 1];
        __syncthreads();
    }
    if (tid == 0) C.status[g] = 0, C.seq_len[g] = seq_base, C.trace_len[g] = trace_base;
}

}   // namespace

int ccs_seeds_launch(const CcsDev &D, const CcsMapDev &M, void *stream) {
    if (M.n_pairs <= 0) return (int)hipSuccess;
    hipLaunchKernelGGL(ccs_seeds_kernel, dim3((unsigned)M.n_pairs), dim3(SEED_BLOCK), 0, (hipStream_t)stream, D, M);
    return (int)hipGetLastError();
}

int ccs_align_launch(const CcsDev &D, const CcsMapDev &M, void *stream) {
    if (M.count <= 0) return (int)hipSuccess;
    const int W = 2 * D.p.w + 1;
    const size_t lds = (size_t)4 * (W + 1) * sizeof(int32_t) + (size_t)((W + 15) / 16) * 16;
    hipLaunchKernelGGL(ccs_align_kernel, dim3((unsigned)M.count), dim3(64), lds, (hipStream_t)stream, D, M);
    return (int)hipGetLastError();
}

int ccs_cns_launch(const CcsDev &D, const CcsCnsDev &C, void *stream) {
    if (C.n <= 0) return (int)hipSuccess;
    hipLaunchKernelGGL(ccs_cns_kernel, dim3((unsigned)C.n), dim3(CNS_BLOCK), 0, (hipStream_t)stream, D, C);
    return (int)hipGetLastError();
}

}   // namespace prgpu

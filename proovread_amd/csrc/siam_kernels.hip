// siamaera's self-alignments on the device (siam_core.h states the rules).
//
//   siam_seeds_kernel   one block per read: the read's bit planes (siam_core.h) are built
//                       into scratch, then one lane per anti-diagonal tests 64 cells per
//                       step with one AND per base; neighbouring lanes read the same plane
//                       words (their shifts differ by one bit), and only a window that holds
//                       a run of word cells is looked at cell by cell.
//   siam_reads_kernel   one wave per read: the seeds in LDS, the next seed by a wave-wide
//                       minimum of the order key, left and right extension by wave_extend,
//                       seeds inside the new alignment's box struck out by all lanes.
//   wave_extend         ksw_extend2 with counts, one lane per column of the band.  The band
//                       is at most 2 w + 1 <= 63 columns, so column j lives in lane j & 63
//                       for the whole extension (eh[j] of the oracle in registers, no LDS
//                       row): F is a prefix maximum of (value << 6 | column) over the lanes,
//                       which also names the source column whose counts are fetched; the row
//                       maximum is a wave maximum of the same kind of key (last column on
//                       ties); the beg / end pruning is a ballot.
#include <hip/hip_runtime.h>

#include "siam_dev.h"

namespace prgpu {
namespace {

using siam::Ext;
using siam::Seed;

// base k of a sequence read forwards or backwards from `base`, complemented or not
struct Src {
    const uint8_t *p;
    int64_t base;
    int dir, len, cmp;
};
__device__ inline int fetch(const Src &s, int k) {
    const int c = s.p[s.base + (int64_t)s.dir * k];
    return s.cmp ? siam::comp(c) : c;
}

__device__ Ext wave_extend(const pr_siam_aligner &al, const Src &Q, const Src &T, int h0) {
    Ext res = {h0, 0, 0, 0, 0};
    const int qlen = Q.len, tlen = T.len;
    if (qlen <= 0 || tlen <= 0) return res;
    const int lane = threadIdx.x & 63;
    const int oe = al.o + al.e, ge = al.e;
    const int w = siam::band(al, qlen);   // <= 31 (checked by the host)
    // eh[j] of the column this lane holds: h = H(i-1, j-1), e = E(i, j), each with counts
    int Hv = 0, Hm = 0, Hc = 0, Ev = 0, Em = 0, Ec = 0;
    if (lane <= w && lane <= qlen) {   // the first row, columns 0 .. w
        Hv = siam::first_row(h0, oe, ge, lane);
        Hc = lane;
    }
    int max = h0, max_i = -1, max_j = -1, bm = 0, bc = 0, beg = 0, end = qlen;
    int curj = -1, qb = 4;
    for (int i = 0; i < tlen; ++i) {
        // column i + w + 1 enters the band's reach: its lane's previous column (64 lower) is
        // below every later beg
        const int cnew = i + w + 1;
        if (cnew <= qlen && lane == (cnew & 63)) {
            Hv = siam::first_row(h0, oe, ge, cnew);
            Hm = 0, Hc = cnew, Ev = 0, Em = 0, Ec = 0;
        }
        const int tb = fetch(T, i);
        if (beg < i - w) beg = i - w;
        if (end > i + w + 1) end = i + w + 1;
        if (end > qlen) end = qlen;
        const int n = end - beg;
        const int r = (lane - beg) & 63, j = beg + r;
        const bool act = r < n;
        if (act && j != curj) {
            curj = j;
            qb = fetch(Q, j);
        }
        int Mv = 0, Mm = 0, Mc = 0;
        if (act && Hv) {
            Mv = Hv + siam::sc(al, qb, tb);
            Mm = Hm + siam::is_match(qb, tb);
            Mc = Hc + 1;
        }
        int t = Mv - oe;
        t = t > 0 ? t : 0;
        // F(i, j) = max over k < j of t_k - (j - 1 - k) e; ties go to the largest k
        int key = act ? ((t + r * ge) << 6 | r) : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl(key, (lane - d) & 63, 64);
            if (r >= d && o > key) key = o;
        }
        const int fk = __shfl(key, (lane - 1) & 63, 64);
        const int srcr = fk & 63, srcl = (beg + srcr) & 63;
        const int sm = __shfl(Mm, srcl, 64), sc_ = __shfl(Mc, srcl, 64);
        int Fv = 0, Fm = 0, Fc = 0;
        if (act && r >= 1) {
            Fv = (fk >> 6) - (r - 1) * ge;
            Fm = sm;
            Fc = sc_ + (r - srcr);
        }
        int hv, hm, hc;
        if (Mv > Ev) hv = Mv, hm = Mm, hc = Mc; else hv = Ev, hm = Em, hc = Ec;
        if (!(hv > Fv)) hv = Fv, hm = Fm, hc = Fc;
        // the row maximum, the last column on ties
        int hk = act ? (hv << 6 | r) : -1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int o = __shfl_xor(hk, d, 64);
            hk = o > hk ? o : hk;
        }
        const int mm = hk < 0 ? 0 : hk >> 6;
        const int mj = beg + (hk & 63);
        if (act) {   // E(i+1, j)
            const int ev2 = Ev - ge;
            if (ev2 > t) Ev = ev2, Ec += 1; else Ev = t, Em = Mm, Ec = Mc + 1;
        }
        // eh[j+1].h = H(i, j); eh[beg].h = the first column; eh[end].e = 0
        const int pv = __shfl(hv, (lane - 1) & 63, 64), pm = __shfl(hm, (lane - 1) & 63, 64),
                  pc = __shfl(hc, (lane - 1) & 63, 64);
        if (r == 0) {
            Hv = beg == 0 ? siam::first_col(h0, al.o, al.e, i) : 0;
            Hm = 0, Hc = i + 1;
        } else if (r <= n) {
            Hv = pv, Hm = pm, Hc = pc;
        }
        if (r == n) Ev = 0;
        if (mm == 0) break;
        if (mm > max) {
            max = mm, max_i = i, max_j = mj;
            bm = __shfl(hm, mj & 63, 64);
            bc = __shfl(hc, mj & 63, 64);
        } else if (al.zdrop > 0) {
            if (i - max_i > mj - max_j) {
                if (max - mm - ((i - max_i) - (mj - max_j)) * ge > al.zdrop) break;
            } else {
                if (max - mm - ((mj - max_j) - (i - max_i)) * ge > al.zdrop) break;
            }
        }
        // drop the zero cells at both ends of [beg, end]
        const uint64_t nz = __ballot(Hv != 0 || Ev != 0);
        const int b = beg & 63;
        const uint64_t rot = b ? (nz >> b | nz << (64 - b)) : nz;   // bit r = column beg + r
        const uint64_t low = rot & ((1ull << n) - 1);
        const int br = low ? __builtin_ctzll(low) : n;
        const uint64_t valid = n >= 63 ? ~0ull : ((1ull << (n + 1)) - 1);
        const uint64_t rng = rot & valid & ~((1ull << br) - 1);
        const int jr = rng ? 63 - __builtin_clzll(rng) : br - 1;
        end = beg + jr + 2 < qlen ? beg + jr + 2 : qlen;
        beg += br;
    }
    res.score = max, res.qle = max_j + 1, res.tle = max_i + 1, res.m = bm, res.c = bc;
    return res;
}

__global__ void __launch_bounds__(256) siam_seeds_kernel(SiamDev D) {
    const int rd = blockIdx.x;
    const int64_t L64 = D.off[rd + 1] - D.off[rd];
    if (L64 > PR_SIAM_MAX_LEN || L64 < D.al.word) return;
    const int L = (int)L64, word = D.al.word;
    const uint8_t *s = D.seq + D.off[rd];
    uint64_t *pl = D.planes + D.plane_off[rd];
    const int nw = siam::plane_words(L);
    for (int w = threadIdx.x; w < nw; w += blockDim.x) siam::build_plane_word(s, L, nw, w, pl);
    __syncthreads();   // the planes are read by every lane of the block
    Seed *out = D.seeds + (int64_t)rd * PR_SIAM_MAX_SEEDS;
    int32_t *cnt = D.n_seeds + rd;
    for (int k = threadIdx.x; k < 2 * L - 1; k += blockDim.x)
        siam::seeds_of_diagonal(s, L, pl, nw, k - (L - 1), word, [&](int i, int p, int len) {
            const int q = atomicAdd(cnt, 1);
            if (q < PR_SIAM_MAX_SEEDS) out[q] = Seed{i, p, len};
        });
}

__device__ inline uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
        const uint64_t o = (uint64_t)hi << 32 | lo;
        v = o < v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(64) siam_reads_kernel(SiamDev D) {
    __shared__ Seed sd[PR_SIAM_MAX_SEEDS];
    const int rd = blockIdx.x, lane = threadIdx.x;
    const int64_t L64 = D.off[rd + 1] - D.off[rd];
    int status = 0, nh = 0;
    const int ns = D.n_seeds[rd];
    if (L64 > PR_SIAM_MAX_LEN) status = PR_SIAM_TOO_LONG;
    else if (ns > PR_SIAM_MAX_SEEDS) status = PR_SIAM_SEED_OVERFLOW;
    if (status == 0 && ns > 0) {
        const int L = (int)L64;
        const uint8_t *s = D.seq + D.off[rd];
        const Seed *in = D.seeds + (int64_t)rd * PR_SIAM_MAX_SEEDS;
        for (int k = lane; k < ns; k += 64) sd[k] = in[k];
        __syncthreads();
        pr_siam_hsp *out = D.hsps + (int64_t)rd * PR_SIAM_MAX_HSPS;
        for (;;) {
            uint64_t best = ~0ull;
            for (int k = lane; k < ns; k += 64) {
                if (sd[k].len > 0) {
                    const uint64_t key = siam::seed_key(sd[k].i, sd[k].p, sd[k].len);
                    best = key < best ? key : best;
                }
            }
            best = wave_min_u64(best);
            if (best == ~0ull) break;
            if (nh == PR_SIAM_MAX_HSPS) {
                status = PR_SIAM_HSP_OVERFLOW;
                nh = 0;
                break;
            }
            const int len = 0x3FFFF - (int)(best >> 36), i = (int)(best >> 18) & 0x3FFFF, p = (int)best & 0x3FFFF;
            const Src ql = {s, (int64_t)i - 1, -1, i, 0}, tl = {s, (int64_t)p + 1, 1, L - 1 - p, 1};
            const Ext el = wave_extend(D.al, ql, tl, len * D.al.a);
            const Src qr = {s, (int64_t)i + len, 1, L - i - len, 0}, tr = {s, (int64_t)p - len, -1, p - len + 1, 1};
            const Ext er = wave_extend(D.al, qr, tr, el.score);
            const pr_siam_hsp h = siam::make_hsp(rd, i, p, len, el, er);
            if (lane == 0) out[nh] = h;
            ++nh;
            for (int k = lane; k < ns; k += 64)
                if (sd[k].len > 0 && siam::seed_inside(h, sd[k].i, sd[k].p, sd[k].len)) sd[k].len = 0;
            __syncthreads();
        }
    }
    if (lane == 0) {
        D.n_hsps[rd] = nh;
        D.status[rd] = status;
    }
}

__global__ void __launch_bounds__(64) siam_pairs_kernel(SiamPairs D) {
    const int k = blockIdx.x;
    const Src q = {D.q, D.q_off[k], 1, (int)(D.q_off[k + 1] - D.q_off[k]), 0};
    const Src t = {D.t, D.t_off[k], 1, (int)(D.t_off[k + 1] - D.t_off[k]), 0};
    const Ext e = wave_extend(D.al, q, t, D.h0[k]);
    if (threadIdx.x == 0) {
        int32_t *o = D.out + 5 * (int64_t)k;
        o[0] = e.score, o[1] = e.qle, o[2] = e.tle, o[3] = e.m, o[4] = e.c;
    }
}

}   // namespace

int siam_launch(const SiamDev &D, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (D.n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(D.n_seeds, 0, sizeof(int32_t) * (size_t)D.n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(siam_seeds_kernel, dim3((unsigned)D.n), dim3(256), 0, st, D);
    hipLaunchKernelGGL(siam_reads_kernel, dim3((unsigned)D.n), dim3(64), 0, st, D);
    return hipGetLastError();
}

int siam_pairs_launch(const SiamPairs &D, void *stream) {
    if (D.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(siam_pairs_kernel, dim3((unsigned)D.n), dim3(64), 0, (hipStream_t)stream, D);
    return hipGetLastError();
}

}   // namespace prgpu

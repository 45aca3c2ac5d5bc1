// Chaining of one short read by a whole wave with every piece of chaining state on chip
// (seed_chain_kernel in seed_kernels.hip): the part of seed_core.h's map_after_occ that follows
// the SMEMs -- mem_chain, mem_chain_flt and mem_chain2aln's task list -- for the reads where bwa
// skips mem_flt_chained_seeds (seed_flt_min_score < 0: every read of the sr modes).
//
// Pass 1's lane writes the read's selected occurrences (emit_occ: chain_seq's selection, in
// chaining order) into a launch-wide pool; this file's chain_read streams them through LDS,
// chains them there and writes the tasks to the read's slots of the output slab.
//
// No HIP here.  The code is written as phases: inside SCC_LANES { ... } every lane runs the body
// on its own (LDS atomics only where the order cannot matter), and a phase ends with the wave's
// LDS synchronisation.  On the device `lane` is the thread's lane and a phase runs once; on the
// host `lane` is a loop index, 0 .. 63 one after the other, so a native program runs exactly the
// device's decisions.  Counters every lane adds to live in ChainLds::sv.  Code between the phases is
// run by every lane with the same values (the host: once); values that cross lanes there -- a
// ballot, a scan, one lane's value -- go through scc_ballot / scc_scan / scc_bcast below, and a
// value a lane keeps from one phase to the next is a LaneReg.
//
// Chains of different (long read, strand) ranges never interact (seed_core.h chain_seq): the
// ranges are dealt to lanes by a hash of their key and every lane chains its ranges' occurrences
// in stream order (as chain_wave in seed_kernels.hip).  A chain's place in creation order -- the
// chain sort's last tie-break -- is the stream index of the occurrence that opened it, so no
// shared counter decides an order.
#pragma once
#include "seed_core.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define SCC_SYNC()                                              \
    do {                                                        \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
        __builtin_amdgcn_wave_barrier();                        \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
    } while (0)
#define SCC_LANES \
    for (int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), go_ = 1; go_; go_ = 0)
#define SCC_END SCC_SYNC()
#define SCC_ADD(p, v) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define SCC_OR(p, v) __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
namespace prgpu {
namespace seedc {
template <class T> __device__ inline T scc_cas(T *p, T c, T v) {   // -> the value found
    __hip_atomic_compare_exchange_strong(p, &c, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return c;
}
}  // namespace seedc
}  // namespace prgpu
#define SCC_CAS(p, c, v) ::prgpu::seedc::scc_cas(p, c, v)
#define SCC_NOW() __builtin_amdgcn_s_memrealtime()
#define SCC_STAT(L, k) ((void)0)
// Cross-lane values.  A LaneReg is a value of each lane that lives across phases (a register; the
// host keeps all 64), read and written as r.at(lane) inside SCC_LANES.  The operations below are
// called between phases, by every lane (the host: once), with the lane's value as a function of
// the lane; what they return is the same in every lane unless it is written to a LaneReg.
namespace prgpu {
namespace seedc {
__device__ inline int scc_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
template <class T> struct LaneReg {
    T v;
    __device__ T &at(int) { return v; }
    __device__ const T &at(int) const { return v; }
};
// bit l: f(l) != 0
template <class F> __device__ inline uint64_t scc_ballot(F f) { return __builtin_amdgcn_ballot_w64(f(scc_lane()) ? true : false); }
// lane src's value (src the same in every lane)
__device__ inline int scc_bcast(const LaneReg<int> &r, int src) { return __builtin_amdgcn_readlane(r.v, src); }
__device__ inline uint64_t scc_bcast(const LaneReg<uint64_t> &r, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)r.v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(r.v >> 32), src);
    return (uint64_t)hi << 32 | lo;
}
// ex.at(l) = f(0) + .. + f(l - 1); -> the sum over all lanes
template <class F> __device__ inline int scc_scan(LaneReg<int> &ex, F f) {
    const int lane = scc_lane(), v = f(lane);
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __builtin_amdgcn_ds_bpermute((lane - d) << 2, x);   // (lane - d's x)
        if (lane >= d) x += y;
    }
    ex.v = x - v;
    return __builtin_amdgcn_readlane(x, 63);
}
}  // namespace seedc
}  // namespace prgpu
#else
// host only: how often a case occurred in the read (ChainLds::sv, SV_TIES ..), for the tests
#define SCC_STAT(L, k) (++(L).sv[k])
#define SCC_LANES for (int lane = 0; lane < 64; ++lane)
#define SCC_END ((void)0)
namespace prgpu {
namespace seedc {
template <class T> inline T scc_add(T *p, T v) { const T o = *p; *p = (T)(o + v); return o; }
template <class T> inline T scc_or(T *p, T v) { const T o = *p; *p = (T)(o | v); return o; }
template <class T> inline T scc_cas(T *p, T c, T v) { const T o = *p; if (o == c) *p = v; return o; }
// the cross-lane values' host twins: every lane's value before any lane uses the result
template <class T> struct LaneReg {
    T v[64];
    T &at(int lane) { return v[lane]; }
    const T &at(int lane) const { return v[lane]; }
};
template <class F> inline uint64_t scc_ballot(F f) {
    uint64_t m = 0;
    for (int lane = 0; lane < 64; ++lane) m |= f(lane) ? 1ull << lane : 0ull;
    return m;
}
inline int scc_bcast(const LaneReg<int> &r, int src) { return r.v[src & 63]; }
inline uint64_t scc_bcast(const LaneReg<uint64_t> &r, int src) { return r.v[src & 63]; }
template <class F> inline int scc_scan(LaneReg<int> &ex, F f) {
    int v[64], x = 0;
    for (int lane = 0; lane < 64; ++lane) v[lane] = f(lane);   // (f may read ex)
    for (int lane = 0; lane < 64; ++lane) ex.v[lane] = x, x += v[lane];
    return x;
}
}  // namespace seedc
}  // namespace prgpu
#define SCC_ADD(p, v) ::prgpu::seedc::scc_add(p, v)
#define SCC_OR(p, v) ::prgpu::seedc::scc_or(p, v)
#define SCC_CAS(p, c, v) ::prgpu::seedc::scc_cas(p, c, v)
#define SCC_NOW() 0ULL
#endif

namespace prgpu {
namespace seedc {

// ---------------------------------------------------------------- the hand-over list
// The reads' occurrence lists lie in one pool of 8-byte words shared by the launch; a read takes
// the words it needs from the pool's cursor before it writes (the count follows from the SMEMs'
// occurrence counts alone): n packed coordinates (Scratch.hfr's values), then n times
// qbeg | len << 16.  The list's first word goes to the head of the read's output slots, its
// length to the read's task count, until seed_chain_kernel replaces both.
constexpr int32_t OCC_MAX = 16384;   // occurrences a read may hand over (stream indices are 16-bit on chip)
struct OccPool {
    uint64_t *w;                 // the pool
    unsigned long long *cursor;  // words taken
    int64_t cap;                 // words
};
SC_HD constexpr int64_t occ_words(int n) { return (int64_t)n + (n + 1) / 2; }
SC_HD const uint32_t *occ_ql(const uint64_t *hfr, int n) { return reinterpret_cast<const uint32_t *>(hfr + n); }
// pool words per read the driver allows for (seed_plan.h occ_pool_words; 1.5 words an
// occurrence): the eager tasks' noisy mapping hands over ~500 occurrences a read on raw long
// reads and ~1,100 on a masked stand-in text, the finish task's ~50
SC_HD int32_t occ_words_per_read(bool lazy) { return lazy ? 384 : 3072; }

// the occurrences mem_chain takes of an SMEM with np of them (chain_seq's selection: every
// step-th in text order, at most max_occ)
SC_HD int occ_taken(const pr_seed_opts &O, int64_t np) {
    const int64_t step = np > O.max_occ ? np / O.max_occ : 1;
    const int64_t c = (np + step - 1) / step;
    return (int)(c < O.max_occ ? c : O.max_occ);
}

// The occurrences mem_chain would chain (seed_core.h chain_seq's selection: ml >= slen, every
// step-th of them, at most max_occ an SMEM) of the SMEMs S.mems[0, nm), SMEM by SMEM, into words
// of the pool; nothing is read back.  *first: the list's first word, *n_occ its length.  0,
// SC_OVER_HITS (a lazy start that was never materialized, as chain_seq) or SC_OVER_SEEDS (more
// than OCC_MAX occurrences, or the pool is full).
template <bool LZ>
SC_HD int emit_occ(const pr_seed_opts &O, const Scratch &S, int nm, const OccPool &P, int64_t *first, int *n_occ) {
    *n_occ = 0;
    *first = 0;
    int64_t tot = 0;
    for (int mi = 0; mi < nm; ++mi) {
        if (LZ && !S.ready[S.mems[mi].start]) return SC_OVER_HITS;
        tot += occ_taken(O, S.mems[mi].occ);
    }
    if (tot > OCC_MAX) return SC_OVER_SEEDS;
    if (tot == 0) return 0;
    const int64_t words = occ_words((int)tot);
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t w0 = (int64_t)__hip_atomic_fetch_add(P.cursor, (unsigned long long)words, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
#else
    const int64_t w0 = (int64_t)__atomic_fetch_add(P.cursor, (unsigned long long)words, __ATOMIC_RELAXED);
#endif
    if (w0 + words > P.cap) return SC_OVER_SEEDS;
    uint64_t *hfr = P.w + w0;
    uint32_t *qlv = reinterpret_cast<uint32_t *>(hfr + tot);
    int32_t n = 0;
    for (int mi = 0; mi < nm; ++mi) {
        const Iv p = S.mems[mi];
        const int slen = p.end - p.start;
        const int32_t h0 = S.hoff[p.start], h1 = LZ ? S.hend[p.start] : S.hoff[p.start + 1];
        const int64_t np = p.occ;
        const int64_t step = np > O.max_occ ? np / O.max_occ : 1;
        const uint32_t ql = (uint32_t)(uint16_t)p.start | ((uint32_t)slen << 16);
        int64_t fidx = 0, take = 0, count = 0;
        int32_t k = h0;
        while (k < h1 && count < O.max_occ) {
            // the start's match lengths 8 at a time (independent loads), then in order; the
            // selected hits' coordinates loaded together, then stored one after the other
            uint16_t ml[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) ml[u] = k + u < h1 ? S.hml[k + u] : (uint16_t)0;
            int32_t sel[8];
            int nsel = 0;
            for (int u = 0; u < 8 && k < h1 && count < O.max_occ; ++u, ++k) {
                if (ml[u] < slen) continue;
                const bool use = fidx == take;
                ++fidx;
                if (!use) continue;
                take += step;
                ++count;
                sel[nsel++] = k;
            }
            if (n + nsel > tot) return SC_OVER_SEEDS;   // (never: an SMEM's count is its qualifying hits)
            uint64_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = u < nsel ? S.hfr[sel[u]] : 0ull;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (u < nsel) {
                    hfr[n + u] = v[u];
                    qlv[n + u] = ql;
                }
            }
            n += nsel;
        }
    }
    if (n != tot) return SC_OVER_SEEDS;   // (never, as above: the list's layout depends on it)
    *first = w0;
    *n_occ = n;
    return 0;
}

// ---------------------------------------------------------------- on-chip state
// S: seeds (and chains) a read may have; HT: entries of the range table (a power of two), at most
// HT / 2 ranges; CH: occurrences streamed through at a time.  A read beyond S or HT / 2 leaves
// with SC_OVER_SEEDS / SC_OVER_CHAINS.  Seed and chain slots are handed out by a counter in any
// order: nothing depends on a slot's number, a chain's place in creation order is the stream
// index of the occurrence that opened it (cidx).
template <int S, int HT, int CH>
struct ChainLds {
    static_assert(S % 8 == 0 && S < 32768 && CH % 64 == 0 && (HT & (HT - 1)) == 0, "slot indices are int16");
    static constexpr int SEEDS = S, RANGES = HT / 2;
    uint64_t hfr[S];   // seeds: coordinate << 24 | long read
    uint32_t ql[S];    //        qbeg | len << 16
    int16_t nx[S];     //        the next seed of its chain (-1: the last)
    int16_t chead[S], ctail[S], cn[S];   // chains: first and last seed, seeds
    int16_t cnx[S];    //        the next chain of its range; after the chaining the chain's weight
    uint16_t cidx[S];  //        the stream index of the occurrence that opened it
    int16_t ts[S];     // output: a task's seed; before the sort: the weights by pl index
    union {
        struct {
            int32_t key[HT];   // rid * 2 + strand (-1: free)
            int16_t head[HT], tail[HT];   // the range's chain list
            uint64_t hfr[CH];  // the occurrences being chained
            uint32_t ql[CH];
            int16_t idx[CH];   // the lanes' lists of them
        } ch;
        struct {
            int16_t pl[S];     // the chains past -W, any order; after the sort a task's chain
            int16_t sch[S];    // the same sorted (weight desc, pos, cidx)
            int16_t kept[S];   // by sorted index
            int16_t fm[S];     // kept list from its 64th entry: the first chain it shadowed (-1: none)
            int16_t kb[S], ke[S], kw[S];   // after the sort: the chains' query intervals and weights by sorted
                                           // index; -D packs the kept list into them in place (entry k <= the
                                           // chain's sorted index; the first 64 entries are kept in registers);
                                           // kb / ke after -D: task base, chain number
        } po;
    } u;
    int32_t cnt[64], cur[64];
    int32_t sv[16];      // wave-uniform values (SV_*)
};
enum {
    SV_ERR = 0, SV_NRG, SV_NP, SV_NS, SV_NC,
    // host build only (SCC_STAT): sort ties that creation order decided, chains opened before the
    // head / between two chains / after the tail of a range that had chains, chains whose
    // reference cover is below their query cover
    SV_TIES, SV_INS_HEAD, SV_INS_MID, SV_INS_TAIL, SV_WR_LT
};

// chain_read's phases (its ticks): the chunks on chip with the lanes' lists, the lane chaining, the
// weights and the list past -W, the rank sort, -D, the tasks' bases, the tasks
enum { CT_LOAD = 0, CT_LANES, CT_WEIGHTS, CT_SORT, CT_DROP, CT_BASE, CT_TASKS, CT_N };

SC_HD uint32_t range_hash(int32_t key) { return (uint32_t)key * 0x9E3779B1u; }

// The tasks of one read from its occurrence list g_hfr / g_ql [0, n).  Every lane of the wave
// calls it (the host: once).  -> 0 or SC_OVER_SEEDS / SC_OVER_CHAINS / SC_OVER_OUT, *n_out the tasks.
// lim_seeds / lim_chains: the capacities of the pass the read comes from (Caps.seeds / .chains),
// which hold here as in its lane chaining: the same reads as before go on to the later passes.
// ticks (device, optional): wall-clock ticks added by the wave, by CT_* below.
template <int S, int HT, int CH>
SC_HD int chain_read(const IndexView &I, const pr_seed_opts &O, ChainLds<S, HT, CH> &L, const uint64_t *g_hfr,
                     const uint32_t *g_ql, int n, int len, int sid, pr_seed_task *out, int cap_out, int *n_out,
                     unsigned long long *ticks = nullptr, int lim_seeds = S, int lim_chains = S) {
    *n_out = 0;
    // (the pass's own capacities below the geometry's: a read beyond them goes on as before)
    lim_seeds = lim_seeds < S ? lim_seeds : S;
    lim_chains = lim_chains < S ? lim_chains : S;
    if (n > OCC_MAX) return SC_OVER_SEEDS;
    if (n <= 0) return 0;
    unsigned long long t_last = ticks ? SCC_NOW() : 0ULL;
    (void)t_last;
#define SCC_TICK(k)                                     \
    do {                                                \
        if (ticks) {                                    \
            const unsigned long long t_ = SCC_NOW();    \
            ticks[k] += t_ - t_last;                    \
            t_last = t_;                                \
        }                                               \
    } while (0)
    const int64_t l_pac = I.l_pac;
    auto rbeg = [&L](int e) -> int64_t { return (int64_t)(L.hfr[e] >> FR_RID_BITS); };
    auto qb = [&L](int e) -> int { return (int)(L.ql[e] & 0xFFFFu); };
    auto sl = [&L](int e) -> int { return (int)(L.ql[e] >> 16); };

    // 0. empty table, counters
    SCC_LANES {
        if (lane < 16) L.sv[lane] = 0;
        for (int k = lane; k < HT; k += 64) L.u.ch.key[k] = -1;
    }
    SCC_END;
    // a chunk's words are loaded while the chunk before it is chained (a lane holds G of each)
    constexpr int G = CH / 64;
    LaneReg<uint64_t> nh[G];
    LaneReg<uint32_t> nq[G];
    auto fetch = [&](int c0) {
        SCC_LANES {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int e = c0 + g * 64 + lane;
                nh[g].at(lane) = e < n ? g_hfr[e] : 0ull;
                nq[g].at(lane) = e < n ? g_ql[e] : 0u;
            }
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < n && !L.sv[SV_ERR]; c0 += CH) {
        const int m = n - c0 < CH ? n - c0 : CH;
        // 1. the chunk on chip, its occurrences' owner lanes
        LaneReg<int> own[G], pos[G], add[G], cur;
        SCC_LANES {
            L.cnt[lane] = 0;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int e = g * 64 + lane;
                own[g].at(lane) = -1;
                pos[g].at(lane) = add[g].at(lane) = 0;
                if (e < m) {
                    const uint64_t v = nh[g].at(lane);
                    L.u.ch.hfr[e] = v;
                    L.u.ch.ql[e] = nq[g].at(lane);
                    const int rid = (int)(v & ((1u << FR_RID_BITS) - 1u));
                    const int32_t key = rid * 2 + ((int64_t)(v >> FR_RID_BITS) >= l_pac ? 1 : 0);
                    own[g].at(lane) = (int)(range_hash(key) >> 26);
                }
            }
        }
        SCC_END;
        if (c0 + CH < n) fetch(c0 + CH);
        // the lanes' lists in stream order, 64 occurrences a step: the lanes with a lane's owner
        // from six ballots; an occurrence's place in its owner's list is the owner's count so far
        // plus the lanes before it with the same owner
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g * 64 >= m) break;
            uint64_t bit[6];
#pragma unroll
            for (int b = 0; b < 6; ++b) bit[b] = scc_ballot([&](int lane) { return (own[g].at(lane) >> b) & 1; });
            const uint64_t valid = scc_ballot([&](int lane) { return own[g].at(lane) >= 0; });
            SCC_LANES {
                const int o = own[g].at(lane);
                if (o >= 0) {
                    uint64_t same = valid;
#pragma unroll
                    for (int b = 0; b < 6; ++b) same &= ((o >> b) & 1) ? bit[b] : ~bit[b];
                    const int before = __builtin_popcountll(same & ((1ull << lane) - 1ull));
                    pos[g].at(lane) = L.cnt[o] + before;
                    add[g].at(lane) = before ? 0 : __builtin_popcountll(same);   // (the first of them counts them)
                }
            }
            SCC_END;
            SCC_LANES {
                if (add[g].at(lane)) L.cnt[own[g].at(lane)] += add[g].at(lane);
            }
            SCC_END;
        }
        scc_scan(cur, [&](int lane) { return (int)L.cnt[lane]; });
        SCC_LANES { L.cur[lane] = cur.at(lane); }
        SCC_END;
        SCC_LANES {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int o = own[g].at(lane);
                if (o >= 0) L.u.ch.idx[L.cur[o] + pos[g].at(lane)] = (int16_t)(g * 64 + lane);
            }
        }
        SCC_END;
        SCC_TICK(CT_LOAD);
        // 2. every lane chains its occurrences in order (chain_seq's decisions)
        SCC_LANES {
            const int first = L.cur[lane], mine = L.cnt[lane];
            for (int t = 0; t < mine; ++t) {
                const int e = L.u.ch.idx[first + t];
                const uint64_t v = L.u.ch.hfr[e];
                const uint32_t qlv = L.u.ch.ql[e];
                const int64_t rb = (int64_t)(v >> FR_RID_BITS);
                const int rid = (int)(v & ((1u << FR_RID_BITS) - 1u));
                const int32_t key = rid * 2 + (rb >= l_pac ? 1 : 0);
                const int qbe = (int)(qlv & 0xFFFFu), sle = (int)(qlv >> 16);
                // the range: probe, claiming a free entry with a CAS (other lanes' keys may share a probe run)
                uint32_t h = range_hash(key) & (uint32_t)(HT - 1);
                bool found = false, claimed = false;
                for (int probe = 0; probe < HT; ++probe) {
                    const int32_t kk = L.u.ch.key[h];
                    if (kk == key) { found = true; break; }
                    if (kk == -1) {
                        const int32_t old = SCC_CAS(&L.u.ch.key[h], (int32_t)-1, key);
                        if (old == -1) { claimed = true; break; }
                        if (old == key) { found = true; break; }
                    }
                    h = (h + 1) & (uint32_t)(HT - 1);
                }
                if (claimed && SCC_ADD(&L.sv[SV_NRG], 1) >= HT / 2) claimed = false;
                if (!found && !claimed) {   // more ranges than the table holds: the read is flagged
                    SCC_OR(&L.sv[SV_ERR], (int32_t)SC_OVER_CHAINS);
                    break;
                }
                int at = -1;
                if (found) {
                    const int tl = L.u.ch.tail[h];
                    if (rbeg(L.chead[tl]) <= rb) {
                        at = tl;
                    } else {
                        for (int x = L.u.ch.head[h]; x >= 0 && rbeg(L.chead[x]) <= rb; x = L.cnx[x]) at = x;
                    }
                }
                bool contained = false, append = false;
                if (at >= 0) {   // test_and_merge with chain `at` (same long read by the key)
                    const int fa = L.chead[at], la = L.ctail[at];
                    const int f_q = qb(fa), l_q = qb(la), l_len = sl(la);
                    const int64_t f_rbeg = rbeg(fa), l_rbeg = rbeg(la);
                    const int64_t qend = l_q + l_len, rend = l_rbeg + l_len;
                    contained = qbe >= f_q && qbe + sle <= qend && rb >= f_rbeg && rb + sle <= rend;
                    if (!contained && !((l_rbeg < l_pac || f_rbeg < l_pac) && rb >= l_pac)) {
                        const int64_t x = qbe - l_q, y = rb - l_rbeg;
                        append = y >= 0 && x - y <= O.w && y - x <= O.w && x - l_len < O.max_chain_gap &&
                                 y - l_len < O.max_chain_gap;
                    }
                }
                if (contained) continue;
                const int sd = SCC_ADD(&L.sv[SV_NS], 1);
                if (sd >= lim_seeds) {
                    SCC_OR(&L.sv[SV_ERR], (int32_t)SC_OVER_SEEDS);
                    break;
                }
                L.hfr[sd] = v;
                L.ql[sd] = qlv;
                L.nx[sd] = -1;
                if (append) {
                    L.nx[L.ctail[at]] = (int16_t)sd;
                    L.ctail[at] = (int16_t)sd;
                    L.cn[at] = (int16_t)(L.cn[at] + 1);
                    continue;
                }
                // a new chain, after `at` and every chain of equal pos
                const int c = SCC_ADD(&L.sv[SV_NC], 1);   // (< S: a chain has a seed)
                if (c >= lim_chains) {
                    SCC_OR(&L.sv[SV_ERR], (int32_t)SC_OVER_CHAINS);
                    break;
                }
                L.chead[c] = L.ctail[c] = (int16_t)sd;
                L.cn[c] = 1;
                L.cidx[c] = (uint16_t)(c0 + e);
                if (!found) {
                    L.u.ch.head[h] = L.u.ch.tail[h] = (int16_t)c;
                    L.cnx[c] = -1;
                } else if (at < 0) {
                    L.cnx[c] = L.u.ch.head[h];
                    L.u.ch.head[h] = (int16_t)c;
                    SCC_STAT(L, SV_INS_HEAD);
                } else {
                    const int nxc = L.cnx[at];
                    L.cnx[c] = (int16_t)nxc;
                    L.cnx[at] = (int16_t)c;
                    if (nxc < 0) {
                        L.u.ch.tail[h] = (int16_t)c;
                        SCC_STAT(L, SV_INS_TAIL);
                    } else {
                        SCC_STAT(L, SV_INS_MID);
                    }
                }
            }
        }
        SCC_END;
        SCC_TICK(CT_LANES);
    }
    if (L.sv[SV_ERR]) return L.sv[SV_ERR];
    const int ncv = L.sv[SV_NC];
    // 3. mem_chain_flt: the weights (seed_core.h chain_weight), the chains past -W listed
    // (any order: the sort's keys are distinct).  The range table is dead from here.
    SCC_LANES {
        for (int c = lane; c < ncv; c += 64) {
            int64_t qe = 0, re = 0;
            int wq = 0, wr = 0;
            for (int k = L.chead[c]; k >= 0; k = L.nx[k]) {
                const int q0 = qb(k), ln = sl(k);
                const int64_t r0 = rbeg(k);
                if (q0 >= qe) wq += ln;
                else if (q0 + ln > qe) wq += (int)(q0 + ln - qe);
                qe = qe > q0 + ln ? qe : q0 + ln;
                if (r0 >= re) wr += ln;
                else if (r0 + ln > re) wr += (int)(r0 + ln - re);
                re = re > r0 + ln ? re : r0 + ln;
            }
            int w = wr < wq ? wr : wq;
            if (wr < wq) SCC_STAT(L, SV_WR_LT);
            w = w < 32767 ? w : 32767;   // (<= the read's length)
            L.cnx[c] = (int16_t)w;
        }
    }
    SCC_END;
    SCC_LANES {
        for (int c = lane; c < ncv; c += 64) {
            const int w = L.cnx[c];
            if (w >= O.min_chain_weight) {
                const int m = SCC_ADD(&L.sv[SV_NP], 1);
                L.u.po.pl[m] = (int16_t)c;
                L.ts[m] = (int16_t)w;
            }
        }
    }
    SCC_END;
    const int nch = L.sv[SV_NP];
    SCC_TICK(CT_WEIGHTS);
    const bool keep_all = O.drop_ratio <= 0;
    // the stable weight sort as ranks: a chain's place is the number of smaller keys
    // ((32767 - weight) << 40 | pos, then cidx).  64 chains a step hold their keys in registers
    // (a lane each) and count the keys below theirs as those come by, a lane after the other
    auto sort_key = [&](int m, uint64_t &a, int &x) {
        a = ~0ull, x = 0;
        if (m < nch) {
            const int c = L.u.po.pl[m];
            a = (uint64_t)(32767 - L.ts[m]) << 40 | (uint64_t)rbeg(L.chead[c]);
            x = L.cidx[c];
        }
    };
    for (int m0 = 0; m0 < nch; m0 += 64) {
        LaneReg<uint64_t> ka, ja;
        LaneReg<int> kx, jx, rk;
        SCC_LANES {
            sort_key(m0 + lane, ka.at(lane), kx.at(lane));
            rk.at(lane) = 0;
        }
        for (int j0 = 0; j0 < nch; j0 += 64) {
            const int mj = nch - j0 < 64 ? nch - j0 : 64;
            SCC_LANES { sort_key(j0 + lane, ja.at(lane), jx.at(lane)); }
            for (int jj = 0; jj < mj; ++jj) {
                const uint64_t a = scc_bcast(ja, jj);
                const int x = scc_bcast(jx, jj);
                SCC_LANES {
                    rk.at(lane) += (a < ka.at(lane) || (a == ka.at(lane) && x < kx.at(lane))) ? 1 : 0;
                    if (a == ka.at(lane) && j0 + jj != m0 + lane) SCC_STAT(L, SV_TIES);
                }
            }
        }
        SCC_LANES {
            const int m = m0 + lane;
            if (m < nch) {
                const int c = L.u.po.pl[m], rank = rk.at(lane);
                L.u.po.sch[rank] = (int16_t)c;
                L.u.po.kept[rank] = keep_all ? 3 : 0;
                if (!keep_all) {   // -D's view of the chain
                    const int tl = L.ctail[c];
                    L.u.po.kb[rank] = (int16_t)qb(L.chead[c]);
                    L.u.po.ke[rank] = (int16_t)(qb(tl) + sl(tl));
                    L.u.po.kw[rank] = L.ts[m];
                }
            }
        }
    }
    SCC_END;
    SCC_TICK(CT_SORT);
    // -D / mask_level (seed_core.h chain_flt) in sorted order.  The chains come 64 at a time into
    // registers (a lane each) and one after the other to every lane; the kept list is tested 64
    // entries a step, entry k by lane k & 63: the first 64 from registers, the later ones from
    // kb / ke / kw [k], where they were packed (k <= the chain's sorted index, which was read
    // before).  The lowest lane that drops the chain is the sequential loop's break.  The kept
    // list's length, `large` and `drop` are the same in every lane: they follow from the ballots.
    if (nch > 0 && !keep_all) {
        LaneReg<int> rb, re, rw, rfm;   // kept entries 0 .. 63: query interval, weight, the first chain it shadowed
        LaneReg<int> cb, ce, cw, cv;    // the step's chains; cv: kept as (0: dropped)
        SCC_LANES { rb.at(lane) = re.at(lane) = rw.at(lane) = 0, rfm.at(lane) = -1; }
        int nk = 0;
        for (int i0 = 0; i0 < nch; i0 += 64) {
            const int mi = nch - i0 < 64 ? nch - i0 : 64;
            SCC_LANES {
                const bool in = lane < mi;
                cb.at(lane) = in ? L.u.po.kb[i0 + lane] : 0;
                ce.at(lane) = in ? L.u.po.ke[i0 + lane] : 0;
                cw.at(lane) = in ? L.u.po.kw[i0 + lane] : 0;
                cv.at(lane) = 0;
            }
            SCC_END;
            for (int j = 0; j < mi; ++j) {
                const int i = i0 + j;
                const int bi = scc_bcast(cb, j), ei = scc_bcast(ce, j), wi = scc_bcast(cw, j);
                bool large = false, drop = false;
                for (int k0 = 0; k0 < nk && !drop; k0 += 64) {
                    LaneReg<int> hit;   // 1: overlaps past mask_level, 2: and drops the chain
                    SCC_LANES {
                        const int k = k0 + lane;
                        int h = 0;
                        if (k < nk) {
                            const int bj = k0 ? L.u.po.kb[k] : rb.at(lane), ej = k0 ? L.u.po.ke[k] : re.at(lane);
                            const int wj = k0 ? L.u.po.kw[k] : rw.at(lane);
                            const int bmax = bj > bi ? bj : bi;
                            const int emin = ej < ei ? ej : ei;
                            if (emin > bmax) {
                                const int li = ei - bi, lj = ej - bj;
                                const int minl = li < lj ? li : lj;
                                if (emin - bmax >= minl * O.mask_level && minl < O.max_chain_gap) {
                                    h = 1;
                                    if (wi < wj * O.drop_ratio && wj - wi >= O.min_seed_len << 1) h = 3;
                                }
                            }
                        }
                        hit.at(lane) = h;
                    }
                    const uint64_t ov = scc_ballot([&](int lane) { return hit.at(lane) & 1; });
                    const uint64_t br = scc_ballot([&](int lane) { return hit.at(lane) & 2; });
                    const int last = br ? ctz64(br) : 63;   // the lanes the sequential loop visits
                    const uint64_t seen = ov & (last >= 63 ? ~0ull : ((2ull << last) - 1ull));
                    SCC_LANES {
                        if ((seen >> lane) & 1ull) {
                            if (k0 == 0) {
                                if (rfm.at(lane) < 0) rfm.at(lane) = i;
                            } else if (L.u.po.fm[k0 + lane] < 0) {
                                L.u.po.fm[k0 + lane] = (int16_t)i;
                            }
                        }
                    }
                    large = large || seen != 0;
                    drop = br != 0;
                }
                if (drop) continue;
                SCC_LANES {
                    if (lane == j) cv.at(lane) = large ? 2 : 3;
                    if (nk < 64) {
                        if (lane == nk) rb.at(lane) = bi, re.at(lane) = ei, rw.at(lane) = wi, rfm.at(lane) = -1;
                    } else if (lane == 0 && nk < S) {   // (always: nk < nch <= S)
                        L.u.po.kb[nk] = (int16_t)bi;
                        L.u.po.ke[nk] = (int16_t)ei;
                        L.u.po.kw[nk] = (int16_t)wi;
                        L.u.po.fm[nk] = -1;
                    }
                }
                if (nk >= 64) SCC_END;
                ++nk;
            }
            SCC_LANES {
                if (lane < mi && cv.at(lane)) L.u.po.kept[i0 + lane] = (int16_t)cv.at(lane);
            }
            SCC_END;
        }
        SCC_LANES {
            if (lane < nk && rfm.at(lane) >= 0) L.u.po.kept[rfm.at(lane)] = 1;
            for (int k = 64 + lane; k < nk && k < S; k += 64)
                if (L.u.po.fm[k] >= 0) L.u.po.kept[L.u.po.fm[k]] = 1;
        }
        SCC_END;
    }
    SCC_TICK(CT_DROP);
    // 4. the tasks (seed_core.h map_output without mem_flt_chained_seeds): a kept chain's tasks
    // start after those of the kept chains before it (a scan over the chains, 64 a step)
    int no = 0, nkept = 0;
    for (int i0 = 0; i0 < nch; i0 += 64) {
        LaneReg<int> ex;
        const int tot = scc_scan(ex, [&](int lane) {
            const int i = i0 + lane;
            return i < nch && L.u.po.kept[i] != 0 ? (int)L.cn[L.u.po.sch[i]] : 0;
        });
        const uint64_t kp = scc_ballot([&](int lane) { return i0 + lane < nch && L.u.po.kept[i0 + lane] != 0; });
        SCC_LANES {
            const int i = i0 + lane;
            if (i < nch) {
                const bool mine = (kp >> lane) & 1ull;
                L.u.po.kb[i] = (int16_t)(mine ? no + ex.at(lane) : -1);
                if (mine) L.u.po.ke[i] = (int16_t)(nkept + __builtin_popcountll(kp & ((1ull << lane) - 1ull)));
            }
        }
        no += tot;
        nkept += __builtin_popcountll(kp);
    }
    SCC_END;
    SCC_TICK(CT_BASE);
    if (no > cap_out) return SC_OVER_OUT;
    // every task's chain and seed, chain list order
    SCC_LANES {
        for (int i = lane; i < nch; i += 64) {
            int t = L.u.po.kb[i];
            if (t < 0) continue;
            for (int k = L.chead[L.u.po.sch[i]]; k >= 0; k = L.nx[k], ++t) {
                L.ts[t] = (int16_t)k;
                L.u.po.pl[t] = (int16_t)i;
            }
        }
    }
    SCC_END;
    // a task per lane: its place among its chain's seeds (length descending, the later first on
    // ties) and the chain's window over all of them (cal_max_gap)
    SCC_LANES {
        for (int t = lane; t < no; t += 64) {
            const int i = L.u.po.pl[t], k = L.ts[t];
            const int c = L.u.po.sch[i], first = L.u.po.kb[i], cnn = L.cn[c];
            const int hd = L.chead[c];
            const int ln = sl(k);
            int rank = 0;
            int64_t r0 = INT64_MAX, r1 = INT64_MIN;
            for (int u = first; u < first + cnn; ++u) {
                const int ku = L.ts[u];
                const int qu = qb(ku), lu = sl(ku);
                const int64_t ru = rbeg(ku);
                rank += (lu > ln || (lu == ln && u > t)) ? 1 : 0;
                const int64_t b = ru - (qu + cal_max_gap(O, qu));
                const int64_t en = ru + lu + ((len - qu - lu) + cal_max_gap(O, len - qu - lu));
                r0 = r0 < b ? r0 : b;
                r1 = r1 > en ? r1 : en;
            }
            const int rid = (int)(L.hfr[hd] & ((1u << FR_RID_BITS) - 1u));
            const bool rev = rbeg(hd) >= l_pac;
            const int64_t lo0 = I.lr_off[rid], lo1 = I.lr_off[rid + 1];
            const int64_t Lr = lo1 - lo0;
            const int64_t cs = rev ? l_pac + (l_pac - lo1) : lo0;
            r0 -= cs;
            r1 -= cs;
            pr_seed_task tk;
            tk.sr = sid;
            tk.lr = rid;
            tk.strand = rev ? 1 : 0;
            tk.qbeg = qb(k);
            tk.rbeg = (int32_t)(rbeg(k) - cs);
            tk.slen = ln;
            tk.rmax0 = (int32_t)(r0 > 0 ? r0 : 0);
            tk.rmax1 = (int32_t)(r1 < Lr ? r1 : Lr);
            tk.chain = L.u.po.ke[i];
            tk.rank = rank;
            out[first + rank] = tk;
        }
    }
    SCC_END;
    SCC_TICK(CT_TASKS);
#undef SCC_TICK
    *n_out = no;
    return 0;
}

// seed_chain_kernel's two geometries: the first for nearly every read, the second (one wave a
// CU) for the reads that outgrow it (the measured distributions)
using ChainLdsSmall = ChainLds<512, 512, 256>;
using ChainLdsLarge = ChainLds<1536, 2048, 256>;

// The device path's routing of one read on the host (pr_seed_map_device_caps): reads that skip
// mem_flt_chained_seeds stop after the SMEMs, hand their occurrences over and are chained by
// chain_read, with the first geometry and then the second; a read that outgrows both takes the
// old path (the later passes' map_read), as does every read of the mr modes.
struct ChainHost {
    ChainLdsSmall a;
    ChainLdsLarge b;
    uint64_t pool[occ_words(OCC_MAX)];
};
template <class LA, class LB>
SC_HD int map_read_chain2(const IndexView &I, const pr_seed_opts &O, Scratch &S, LA &La, LB &Lb, uint64_t *pool,
                          int64_t pool_words, const uint8_t *q, int len, int sid, pr_seed_task *out, int cap_out,
                          int *n_out) {
    *n_out = 0;
    if (seed_flt_min_score(O, len) >= 0) return map_read(I, O, S, q, len, sid, out, cap_out, n_out);
    int err = S.hend ? build_starts(I, S, q, len) : build_occ(I, S, q, len);
    if (err) return err;
    int nm = 0, nocc = 0;
    unsigned long long cursor = 0;
    const OccPool P{pool, &cursor, pool_words};
    int64_t w0 = 0;
    if (S.hend) {
        const OccLazy occ{&I, &S, q, len, nullptr};
        nm = collect_intv(occ, S, O, q, len, err);
        err |= S.lz[1];
        if (!err) err = emit_occ<true>(O, S, nm, P, &w0, &nocc);
        err |= S.lz[1];
    } else {
        const Occ occ{&I, &S, q, len, nullptr};
        nm = collect_intv(occ, S, O, q, len, err);
        if (!err) err = emit_occ<false>(O, S, nm, P, &w0, &nocc);
    }
    if (!err) {
        const uint64_t *hfr = pool + w0;
        err = chain_read(I, O, La, hfr, occ_ql(hfr, nocc), nocc, len, sid, out, cap_out, n_out, nullptr, S.cap_seeds,
                         S.cap_chains);
        if (err & (SC_OVER_SEEDS | SC_OVER_CHAINS))
            err = chain_read(I, O, Lb, hfr, occ_ql(hfr, nocc), nocc, len, sid, out, cap_out, n_out, nullptr, S.cap_seeds,
                             S.cap_chains);
    }
    if (err & (SC_OVER_SEEDS | SC_OVER_CHAINS)) return map_read(I, O, S, q, len, sid, out, cap_out, n_out);
    return err;
}
SC_HD int map_read_chain(const IndexView &I, const pr_seed_opts &O, Scratch &S, ChainHost &H, const uint8_t *q, int len,
                         int sid, pr_seed_task *out, int cap_out, int *n_out) {
    return map_read_chain2(I, O, S, H.a, H.b, H.pool, occ_words(OCC_MAX), q, len, sid, out, cap_out, n_out);
}

}  // namespace seedc
}  // namespace prgpu

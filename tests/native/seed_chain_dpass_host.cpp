// Host build of the on-chip chaining's mem_chain_flt (proovread_amd/csrc/seed_chain.h chain_read:
// rank sort, -D pass, task bases) on directed occurrence lists, next to a plain statement of bwa's
// mem_chain_flt loop written here, for tests/test_seed_chain_dpass_host.py; and the cross-lane
// twins (scc_ballot, scc_scan, scc_bcast) on their own.  Needs no index: the occurrences are made
// up, every one a chain of its own, so a chain's query interval is its seed and its weight the
// seed's length.  -DSC_MAIN: the same as a stand-alone program (the sanitizer run).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../proovread_amd/csrc/seed_chain.h"

using namespace prgpu;
using namespace prgpu::seedc;

namespace {

// the named cases, counted by the plain statement over every read of the run
enum {
    C_OV_EQ = 0,     // overlap == minl * mask_level (counts as overlapping)
    C_OV_OFF,        // overlap one base below it
    C_DR_EQ,         // wi == wj * drop_ratio (not dropped)
    C_DR_OFF,        // wi one below it (dropped)
    C_GAP_EQ,        // wj - wi == 2 * min_seed_len (dropped)
    C_GAP_OFF,       // one below it (not dropped)
    C_MINL_EQ,       // minl == max_chain_gap (not overlapping)
    C_MINL_OFF,      // minl one below it
    C_DROP_AT0, C_DROP_AT63, C_DROP_AT64, C_DROP_AT65,   // the kept index of the entry that dropped a chain
    C_AFTER_SAME,    // an overlapping kept entry after the dropping one, in its step of 64
    C_AFTER_LATER,   // ... in a later step
    C_BEFORE,        // an overlapping kept entry before the dropping one (none: see the Python test)
    C_TWICE,         // a kept entry shadowed again (first stays)
    C_K0, C_K1, C_K2, C_K3,   // chains past -W by their kept value
    C_TIE_POS,       // equal weights, the order decided by pos
    C_TIE_IDX,       // equal weights and pos, decided by the stream index
    C_NK64, C_NK128, // reads whose kept list passes 64 / 128 entries
    C_LIGHT,         // chains below -W
    C_N
};

constexpr int NLR = 128;
constexpr int64_t LR_LEN = 1000000, SLOT = 100000;   // (slots 0 .. 5 of a strand, 2^40 > 2 l_pac)
constexpr int RLEN = 32000;   // the synthetic read: room for every query interval (on-chip positions are int16)

struct Occ1 {
    int qb, len;   // the seed = the chain: query interval [qb, qb + len), weight len
    int key;       // rid = key % NLR, strand = key / NLR % 2, slot = key / (2 NLR): a range holds a chain a slot
    int off;       // offset in its slot of the long read's strand
};

struct Text {
    std::vector<int64_t> lr_off;
    IndexView V;
    Text() {
        for (int r = 0; r <= NLR; ++r) lr_off.push_back(LR_LEN * r);
        V = IndexView{};
        V.lr_off = lr_off.data();
        V.n_lr = NLR;
        V.l_pac = LR_LEN * NLR;
    }
    int64_t cs(int rid, bool rev) const { return rev ? V.l_pac + (V.l_pac - lr_off[(size_t)rid + 1]) : lr_off[(size_t)rid]; }
    int64_t coord(const Occ1 &o) const {
        return cs(o.key % NLR, (o.key / NLR) & 1) + 1000 + (int64_t)(o.key / (2 * NLR)) * SLOT + o.off;
    }
};

pr_seed_opts finish_opts() {   // bwa-sr-finish (-k 17 -W 18 -w 30 -D .75), bwa's mask_level and max_chain_gap
    pr_seed_opts o;
    std::memset(&o, 0, sizeof o);
    o.min_seed_len = 17, o.min_chain_weight = 18, o.w = 30, o.split_factor = 1.5, o.split_width = 10;
    o.max_mem_intv = 20, o.max_occ = 500, o.drop_ratio = 0.75, o.max_chain_gap = 10000, o.mask_level = 0.5;
    o.a = 5, o.o_del = 15, o.e_del = 3, o.o_ins = 19, o.e_ins = 3, o.b = 13;
    return o;
}

// bwa's mem_chain_flt over the chains (bwamem.c: the weight filter, the sort by weight -- here with
// the ties the pos-ordered stable sort leaves: pos, then creation order --, the kept list) -> the
// tasks mem_chain2aln would start from, one a kept chain; kept_of[stream index]: -1 below -W
struct RefChain {
    int w, qb, qe, idx, kept, first;
    int64_t pos;
};
void reference(const Text &T, const pr_seed_opts &O, const std::vector<Occ1> &occ, int sid, std::vector<pr_seed_task> &tasks,
               std::vector<int> &kept_of, int64_t *cnt) {
    std::vector<RefChain> a;
    kept_of.assign(occ.size(), -1);
    for (size_t i = 0; i < occ.size(); ++i) {
        if (occ[i].len < O.min_chain_weight) {
            ++cnt[C_LIGHT];
            continue;
        }
        a.push_back(RefChain{occ[i].len, occ[i].qb, occ[i].qb + occ[i].len, (int)i, 0, -1, T.coord(occ[i])});
    }
    std::sort(a.begin(), a.end(), [](const RefChain &x, const RefChain &y) {
        if (x.w != y.w) return x.w > y.w;
        if (x.pos != y.pos) return x.pos < y.pos;
        return x.idx < y.idx;
    });
    for (size_t i = 1; i < a.size(); ++i)
        if (a[i].w == a[i - 1].w) ++cnt[a[i].pos == a[i - 1].pos ? C_TIE_IDX : C_TIE_POS];
    const int n = (int)a.size();
    std::vector<int> kl;
    auto overlaps = [&](const RefChain &ci, const RefChain &cj) {
        const int bmax = std::max(cj.qb, ci.qb), emin = std::min(cj.qe, ci.qe);
        if (emin <= bmax) return false;
        const int minl = std::min(ci.qe - ci.qb, cj.qe - cj.qb);
        return emin - bmax >= minl * O.mask_level && minl < O.max_chain_gap;
    };
    if (n > 0 && O.drop_ratio > 0) {
        kl.push_back(0);
        a[0].kept = 3;
        for (int i = 1; i < n; ++i) {
            int large = 0;
            size_t k;
            for (k = 0; k < kl.size(); ++k) {
                RefChain &cj = a[(size_t)kl[k]];
                const int bmax = std::max(cj.qb, a[i].qb), emin = std::min(cj.qe, a[i].qe);
                if (emin > bmax) {
                    const int minl = std::min(a[i].qe - a[i].qb, cj.qe - cj.qb);
                    const double need = minl * O.mask_level;
                    if (emin - bmax == need) ++cnt[C_OV_EQ];
                    if (emin - bmax < need && emin - bmax + 1 >= need) ++cnt[C_OV_OFF];
                    if (emin - bmax >= need) cnt[C_MINL_EQ] += minl == O.max_chain_gap, cnt[C_MINL_OFF] += minl == O.max_chain_gap - 1;
                    if (emin - bmax >= need && minl < O.max_chain_gap) {
                        large = 1;
                        if (cj.first < 0) cj.first = i;
                        else ++cnt[C_TWICE];
                        const double lim = cj.w * O.drop_ratio;
                        const bool far = cj.w - a[i].w >= O.min_seed_len << 1;
                        if (far) cnt[C_DR_EQ] += a[i].w == lim, cnt[C_DR_OFF] += a[i].w < lim && a[i].w + 1 >= lim;
                        if (a[i].w < lim) {
                            cnt[C_GAP_EQ] += cj.w - a[i].w == O.min_seed_len << 1;
                            cnt[C_GAP_OFF] += cj.w - a[i].w == (O.min_seed_len << 1) - 1;
                        }
                        if (a[i].w < lim && far) break;
                    }
                }
            }
            if (k == kl.size()) {
                kl.push_back(i);
                a[i].kept = large ? 2 : 3;
            } else {   // dropped by kept entry k: what lies around it (counted only)
                cnt[C_DROP_AT0] += k == 0, cnt[C_DROP_AT63] += k == 63, cnt[C_DROP_AT64] += k == 64, cnt[C_DROP_AT65] += k == 65;
                for (size_t u = 0; u < kl.size(); ++u) {
                    if (u == k || !overlaps(a[i], a[(size_t)kl[u]])) continue;
                    if (u < k) ++cnt[C_BEFORE];
                    else ++cnt[u / 64 == k / 64 ? C_AFTER_SAME : C_AFTER_LATER];
                }
            }
        }
        for (int k : kl)
            if (a[(size_t)k].first >= 0) a[(size_t)a[(size_t)k].first].kept = 1;
    } else {
        for (auto &c : a) c.kept = 3;
    }
    cnt[C_NK64] += kl.size() > 64, cnt[C_NK128] += kl.size() > 128;
    tasks.clear();
    int chain = 0;
    for (const RefChain &c : a) {
        kept_of[(size_t)c.idx] = c.kept;
        ++cnt[C_K0 + c.kept];
        if (!c.kept) continue;
        const Occ1 &o = occ[(size_t)c.idx];
        const int rid = o.key % NLR;
        const bool rev = (o.key / NLR) & 1;
        const int64_t base = T.cs(rid, rev);
        const int64_t r0 = c.pos - (o.qb + cal_max_gap(O, o.qb)) - base;
        const int64_t r1 = c.pos + o.len + ((RLEN - o.qb - o.len) + cal_max_gap(O, RLEN - o.qb - o.len)) - base;
        pr_seed_task t;
        t.sr = sid, t.lr = rid, t.strand = rev ? 1 : 0, t.qbeg = o.qb, t.rbeg = (int32_t)(c.pos - base), t.slen = o.len;
        t.rmax0 = (int32_t)std::max<int64_t>(r0, 0), t.rmax1 = (int32_t)std::min<int64_t>(r1, LR_LEN);
        t.chain = chain++, t.rank = 0;
        tasks.push_back(t);
    }
}

// one read through chain_read with the geometry LDS and through the plain statement -> 0 when the
// tasks and every chain's kept value agree
template <class LDS>
int one_read(const Text &T, const pr_seed_opts &O, const std::vector<Occ1> &occ, int sid, unsigned fill, int64_t *cnt) {
    const int n = (int)occ.size();
    std::vector<uint64_t> w((size_t)occ_words(n) + 1, 0);
    uint32_t *ql = reinterpret_cast<uint32_t *>(w.data() + n);
    for (int e = 0; e < n; ++e) {
        w[(size_t)e] = ((uint64_t)T.coord(occ[(size_t)e]) << FR_RID_BITS) | (uint64_t)(occ[(size_t)e].key % NLR);
        ql[e] = (uint32_t)occ[(size_t)e].qb | ((uint32_t)occ[(size_t)e].len << 16);
    }
    auto L = std::make_unique<LDS>();
    std::memset(L.get(), (int)fill, sizeof *L);   // (LDS is never cleared between reads)
    const int cap = LDS::SEEDS;
    std::vector<pr_seed_task> got((size_t)cap), want;
    std::vector<int> kept_want;
    int nt = -1;
    const int err = chain_read(T.V, O, *L, w.data(), occ_ql(w.data(), n), n, RLEN, sid, got.data(), cap, &nt);
    reference(T, O, occ, sid, want, kept_want, cnt);
    if (err || n == 0) return err || nt != 0 ? 1 : 0;
    if (L->sv[SV_NC] != n) return 2;   // (the directed list: every occurrence a chain of its own)
    if (nt != (int)want.size()) return 3;
    for (int k = 0; k < nt; ++k)
        if (std::memcmp(&got[(size_t)k], &want[(size_t)k], sizeof(pr_seed_task))) return 4;
    int past = 0;
    for (int r = 0; r < L->sv[SV_NP]; ++r, ++past) {   // the chains past -W by sorted index
        const int c = L->u.po.sch[r];
        if (kept_want[(size_t)L->cidx[c]] != L->u.po.kept[r]) return 5;
    }
    for (int k : kept_want) past -= k >= 0;
    return past ? 6 : 0;
}

struct Rng {
    unsigned long long x = 88172645463325252ull;
    unsigned operator()() {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return (unsigned)(x >> 11);
    }
};

// n chains at random: weights 17 .. 216 (17: below -W), intervals over `span` query bases
std::vector<Occ1> random_read(Rng &rnd, int n, int span) {
    std::vector<Occ1> v;
    for (int i = 0; i < n; ++i) {
        const int len = 17 + (int)(rnd() % (i % 5 == 0 ? 12 : 200));
        v.push_back(Occ1{(int)(rnd() % (unsigned)span), len, i, (int)(rnd() % 2000)});
    }
    return v;
}

// A kept list of disjoint entries of weight 100 (ties: pos orders them) in which the entries K,
// K + 1, K + 2 (the same step of 64) and K + 64, K + 66 (a later step) share one interval; a
// chain of weight 20 inside that interval comes last and is dropped by kept entry K, the first
// that overlaps it, whatever follows.  The sharing entries shadow one another (kept 1 and 2,
// entry K shadowed more than once).
std::vector<Occ1> drop_at(int K) {
    std::vector<Occ1> v;
    const int N = K + 70;
    for (int k = 0; k < N; ++k) {
        const bool shared = k == K || k == K + 1 || k == K + 2 || k == K + 64 || k == K + 66;
        v.push_back(Occ1{shared ? 31000 : 200 * k, 100, k, 2 * k});   // (pos_in_list_order: pos grows with k)
    }
    v.push_back(Occ1{31040, 20, N, 0});
    return v;
}

// the sort's order for tied weights is pos: give the chains of a read offsets so that pos grows
// with the list index (forward strand of rid r below that of r + 1; the reverse strands above all
// forward ones, in falling rid order)
void pos_in_list_order(const Text &T, std::vector<Occ1> &v) {
    std::vector<int> keys;
    for (int k = 0; k < 2 * NLR; ++k) keys.push_back(k);
    std::sort(keys.begin(), keys.end(), [&](int x, int y) { return T.coord(Occ1{0, 0, x, 0}) < T.coord(Occ1{0, 0, y, 0}); });
    for (size_t i = 0; i < v.size(); ++i) v[i].key = keys[i % keys.size()] + (int)(i / keys.size()) * 2 * NLR;
}

}  // namespace

// every directed read through both -> the reads that differ; cnt[C_N] the named cases, sizes[8]
// the chain counts past -W of the eight sized reads
extern "C" int dp_run(int64_t *cnt, int32_t *sizes) {
    const Text T;
    pr_seed_opts O = finish_opts();
    for (int k = 0; k < C_N; ++k) cnt[k] = 0;
    Rng rnd;
    int bad = 0, sid = 0;
    auto run = [&](const std::vector<Occ1> &v, const pr_seed_opts &o, bool large = false) {
        const int r = large ? one_read<ChainLdsLarge>(T, o, v, sid, 0xA5, cnt) : one_read<ChainLdsSmall>(T, o, v, sid, 0xA5, cnt);
        if (r) std::fprintf(stderr, "read %d (%zu chains): differs (%d)\n", sid, v.size(), r);
        bad += r != 0;
        ++sid;
    };
    // chain counts (all past -W: weights from 18): 1, 2, 63, 64, 65, 128, 129, the first geometry's
    // 512; sparse intervals, so that the kept lists pass 64 and 128 entries, then dense ones
    const int counts[8] = {1, 2, 63, 64, 65, 128, 129, 512};
    for (int c = 0; c < 8; ++c) {
        for (int dense = 0; dense < 3; ++dense) {
            std::vector<Occ1> v = random_read(rnd, counts[c], dense == 0 ? 31000 : dense == 1 ? 40 * counts[c] + 100 : 1500);
            for (auto &o : v) o.len = o.len < 18 ? 18 : o.len;
            if (dense == 0) sizes[c] = (int32_t)v.size();
            run(v, O);
        }
    }
    for (int k = 0; k < 40; ++k) run(random_read(rnd, 1 + (int)(rnd() % 512), 500 + (int)(rnd() % 30000)), O);
    run(random_read(rnd, 1536, 31000), O, true);   // the second geometry: a kept list over many steps
    run(random_read(rnd, 1200, 4000), O, true);
    // the dropping kept entry at kept index 0, 63, 64 and 65
    for (int K : {0, 63, 64, 65}) {
        std::vector<Occ1> v = drop_at(K);
        pos_in_list_order(T, v);
        run(v, O);
    }
    // the comparisons at equality and one off it: {heavy, light} pairs (a chain's weight is its length)
    auto pair = [&](int qb0, int len0, int qb1, int len1, const pr_seed_opts &o) {
        run(std::vector<Occ1>{Occ1{qb0, len0, 0, 0}, Occ1{qb1, len1, 1, 0}}, o);
    };
    pair(0, 100, 50, 100, O), pair(0, 100, 51, 100, O);   // overlap 50 == 100 * 0.5; 49
    pair(0, 200, 0, 150, O), pair(0, 200, 0, 149, O);     // wi 150 == 200 * 0.75; 149
    pair(0, 100, 0, 66, O), pair(0, 100, 0, 67, O);       // wj - wi == 34; 33
    pr_seed_opts G = O;
    G.max_chain_gap = 60;
    pair(0, 100, 0, 60, G), pair(0, 100, 0, 59, G);       // minl == max_chain_gap; one below
    // weight ties: by pos (two ranges), then by the stream index (one range, one pos, the query
    // intervals too far apart to merge)
    run(std::vector<Occ1>{Occ1{400, 50, 5, 10}, Occ1{100, 50, 4, 10}, Occ1{700, 50, 5, 10}, Occ1{1000, 50, 4, 10}}, O);
    run(std::vector<Occ1>{}, O);
    return bad;
}

// the cross-lane twins on their own -> 0 when all hold
extern "C" int dp_primitives() {
    int bad = 0;
    Rng rnd;
    // a scan over an array, 64 a step with the total carried (as chain_read's task bases)
    for (int n : {0, 1, 63, 64, 65, 513}) {
        std::vector<int> v((size_t)n), ex((size_t)n);
        for (auto &x : v) x = (int)(rnd() % 1000);
        int base = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            LaneReg<int> e;
            const int tot = scc_scan(e, [&](int lane) { return i0 + lane < n ? v[(size_t)(i0 + lane)] : 0; });
            SCC_LANES {
                if (i0 + lane < n) ex[(size_t)(i0 + lane)] = base + e.at(lane);
            }
            base += tot;
        }
        int want = 0;
        for (int i = 0; i < n; ++i) {
            bad += ex[(size_t)i] != want;
            want += v[(size_t)i];
        }
        bad += base != want;
    }
    LaneReg<int> r;
    // a scan may read the register it writes
    SCC_LANES { r.at(lane) = lane + 1; }
    bad += scc_scan(r, [&](int lane) { return r.at(lane); }) != 64 * 65 / 2;
    SCC_LANES { bad += r.at(lane) != lane * (lane + 1) / 2; }
    // ballots: no lane, one lane (every position), all lanes, a pattern
    bad += scc_ballot([](int) { return false; }) != 0ull;
    bad += scc_ballot([](int) { return true; }) != ~0ull;
    for (int one = 0; one < 64; ++one) bad += scc_ballot([&](int lane) { return lane == one; }) != 1ull << one;
    bad += scc_ballot([](int lane) { return lane % 3 == 0; }) != 0x9249249249249249ull;
    // one lane's value
    LaneReg<uint64_t> q;
    SCC_LANES { r.at(lane) = 1000 - lane, q.at(lane) = 0x100000000ull * (unsigned)lane + 7u; }
    for (int s = 0; s < 64; ++s) bad += scc_bcast(r, s) != 1000 - s || scc_bcast(q, s) != 0x100000000ull * (unsigned)s + 7u;
    return bad;
}

extern "C" int dp_count_names(int k, char *buf, int cap) {
    static const char *names[C_N] = {"ov_eq", "ov_off", "dr_eq", "dr_off", "gap_eq", "gap_off", "minl_eq", "minl_off", "drop_at0",
                                     "drop_at63", "drop_at64", "drop_at65", "after_same", "after_later", "before", "twice", "kept0",
                                     "kept1", "kept2", "kept3", "tie_pos", "tie_idx", "nk64", "nk128", "light"};
    if (k < 0 || k >= C_N) return C_N;
    std::snprintf(buf, (size_t)cap, "%s", names[k]);
    return C_N;
}

#ifdef SC_MAIN
int main() {
    int64_t cnt[C_N];
    int32_t sizes[8];
    const int bad = dp_run(cnt, sizes), badp = dp_primitives();
    char nm[32];
    for (int k = 0; k < C_N; ++k) {
        dp_count_names(k, nm, sizeof nm);
        std::printf("%s=%lld ", nm, (long long)cnt[k]);
    }
    std::printf("\n%s\n", bad || badp ? "MISMATCH" : "ok");
    return bad || badp ? 1 : 0;
}
#endif

// Host build of the on-chip chaining (proovread_amd/csrc/seed_chain.h: emit_occ + chain_read, the
// lanes one after the other) next to seed_core.h's map_after_occ on the same reads, for
// tests/test_seed_chain_host.py.  Compiled with proovread_amd/csrc/seed.cpp (the host index).
// -DSC_MAIN: a stand-alone program over random reads (the sanitizer run).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../proovread_amd/csrc/seed_chain.h"
#include "../../proovread_amd/csrc/seed_dev.h"

int pr_set_error(int code, const char *) { return code; }

using namespace prgpu;
using namespace prgpu::seedc;

namespace {

bool same(const pr_seed_task &a, const pr_seed_task &b) { return !std::memcmp(&a, &b, sizeof a); }

constexpr int NRES = 16;   // values a read

// one read through both paths; res[0..7]: occurrences handed over, ranges, chain_read's status
// with the geometry LA, the reference's status, tasks, 1 when the routed result (map_read_chain2:
// LA, then LB, then the old path when the read outgrows both) equals map_read's in status and
// every task, chains, seeds (ranges, chains and seeds: LA's counters, complete when its status is 0);
// res[8..15], when LA's status is 0: sort ties that creation order decided, chains opened before
// the head / between two chains / after the tail of their range, chains whose reference cover is
// below their query cover, chains past -W that -D dropped / kept as 1 / kept as 2
template <class LA, class LB>
void one_read(const IndexView &V, const pr_seed_opts &O, Scratch &S, const uint8_t *q, int len, int sid, int cap_out,
              unsigned fill, int32_t *res) {
    std::vector<pr_seed_task> want((size_t)cap_out), got((size_t)cap_out), slot((size_t)cap_out);
    std::vector<uint64_t> pool((size_t)occ_words(OCC_MAX), 0x0101010101010101ull * (fill & 0xFF));
    auto La = std::make_unique<LA>();
    auto Lb = std::make_unique<LB>();
    std::memset(La.get(), (int)fill, sizeof *La);   // (LDS is never cleared between reads)
    std::memset(Lb.get(), (int)fill, sizeof *Lb);
    int nw = 0, ng = 0;
    const int ew = len > 0 ? map_read(V, O, S, q, len, sid, want.data(), cap_out, &nw) : 0;
    for (int k = 0; k < NRES; ++k) res[k] = 0;
    if (len > 0 && seed_flt_min_score(O, len) < 0) {
        int err = S.hend ? build_starts(V, S, q, len) : build_occ(V, S, q, len);
        int nm = 0, nocc = 0, nt = 0;
        unsigned long long cursor = 0;
        const OccPool P{pool.data(), &cursor, (int64_t)pool.size()};
        int64_t w0 = 0;
        if (!err && S.hend) {
            const OccLazy occ{&V, &S, q, len, nullptr};
            nm = collect_intv(occ, S, O, q, len, err);
            err |= S.lz[1];
            if (!err) err = emit_occ<true>(O, S, nm, P, &w0, &nocc);
        } else if (!err) {
            const Occ occ{&V, &S, q, len, nullptr};
            nm = collect_intv(occ, S, O, q, len, err);
            if (!err) err = emit_occ<false>(O, S, nm, P, &w0, &nocc);
        }
        if (!err) {
            err = chain_read(V, O, *La, pool.data() + w0, occ_ql(pool.data() + w0, nocc), nocc, len, sid, slot.data(), cap_out, &nt);
            if (nocc > 0) {   // (a read without occurrences never touches the on-chip state)
                res[1] = La->sv[SV_NRG];
                res[6] = La->sv[SV_NC];
                res[7] = La->sv[SV_NS];
                if (!err) {
                    res[8] = La->sv[SV_TIES], res[9] = La->sv[SV_INS_HEAD], res[10] = La->sv[SV_INS_MID];
                    res[11] = La->sv[SV_INS_TAIL], res[12] = La->sv[SV_WR_LT];
                    for (int i = 0; i < La->sv[SV_NP]; ++i) {
                        const int kp = La->u.po.kept[i];
                        res[13] += kp == 0, res[14] += kp == 1, res[15] += kp == 2;
                    }
                }
            }
        }
        res[0] = nocc;
        res[2] = err;
    }
    std::memset(La.get(), (int)fill, sizeof *La);
    const int eg = len > 0 ? map_read_chain2(V, O, S, *La, *Lb, pool.data(), (int64_t)pool.size(), q, len, sid, got.data(),
                                             cap_out, &ng)
                           : 0;
    res[3] = ew;
    res[4] = ew ? 0 : nw;
    bool eq = ew == eg && (ew || nw == ng);
    for (int k = 0; eq && !ew && k < nw; ++k) eq = same(want[(size_t)k], got[(size_t)k]);
    res[5] = eq ? 1 : 0;
}

}  // namespace

// geom: 0 the kernel's two geometries, 1 <64 seeds, 32 ranges, 64 at a time> twice, 2 that and the
// kernel's second, 3 <8192, 4096 ranges> with 2,560 output slots (the statistics: nothing the
// device path maps leaves it).  res: 16 values a read (one_read).
extern "C" int sc_chain_compare(const pr_seed_index *h, const pr_seed_opts *o, const uint8_t *sr_seq, const int64_t *sr_off,
                                int n_sr, int geom, int cap_out, int fill, int32_t *res) {
    const IndexView V = seed_index_view(h);
    int qmax = 1;
    for (int i = 0; i < n_sr; ++i) qmax = qmax > (int)(sr_off[i + 1] - sr_off[i]) ? qmax : (int)(sr_off[i + 1] - sr_off[i]);
    Caps caps = device_caps(qmax);
    caps.hi = V.ksplit != nullptr;
    caps.lazy = lazy_occ(*o) ? 1 : 0;
    caps.hits = caps.hits > (1 << 17) ? caps.hits : 1 << 17;   // (repeat families: ~500 hits for every start of a read)
    if (cap_out <= 0) cap_out = geom == 3 ? 2560 : caps.out;
    std::vector<uint64_t> slab((size_t)(scratch_bytes(caps) / 8 + 1), 0x0101010101010101ull * (uint64_t)(fill & 0xFF));
    Scratch S = carve(reinterpret_cast<uint8_t *>(slab.data()), caps);
    for (int k = 0; k < S.hsize; ++k) S.htab[k].key = -1;
    S.htab_clean = true;
    using Tiny = ChainLds<64, 64, 64>;
    using Huge = ChainLds<8192, 8192, 256>;
    for (int i = 0; i < n_sr; ++i) {
        const uint8_t *q = sr_seq + sr_off[i];
        const int len = (int)(sr_off[i + 1] - sr_off[i]);
        int32_t *r = res + NRES * (int64_t)i;
        if (geom == 1) one_read<Tiny, Tiny>(V, *o, S, q, len, i, cap_out, (unsigned)fill, r);
        else if (geom == 2) one_read<Tiny, ChainLdsLarge>(V, *o, S, q, len, i, cap_out, (unsigned)fill, r);
        else if (geom == 3) one_read<Huge, Huge>(V, *o, S, q, len, i, cap_out, (unsigned)fill, r);
        else one_read<ChainLdsSmall, ChainLdsLarge>(V, *o, S, q, len, i, cap_out, (unsigned)fill, r);
    }
    return 0;
}

// chain_read over n copies of one occurrence (position 1000 of long read 0, 20 bases: one chain,
// every other occurrence contained) for n = OCC_MAX - 1, OCC_MAX, OCC_MAX + 1 -> status and tasks
// of each in out6: the most occurrences a read may hand over, at its edge
extern "C" int sc_occ_max_edge(const pr_seed_index *h, const pr_seed_opts *o, int32_t *out6) {
    const IndexView V = seed_index_view(h);
    auto L = std::make_unique<ChainLdsSmall>();
    std::vector<pr_seed_task> slot(384);
    for (int k = 0; k < 3; ++k) {
        const int n = OCC_MAX - 1 + k;
        std::vector<uint64_t> w((size_t)occ_words(n), 0);
        uint32_t *ql = reinterpret_cast<uint32_t *>(w.data() + n);
        for (int e = 0; e < n; ++e) w[(size_t)e] = (1000ull << FR_RID_BITS) | 0ull, ql[e] = 0u | (20u << 16);
        int nt = -1;
        out6[2 * k] = chain_read(V, *o, *L, w.data(), occ_ql(w.data(), n), n, 100, 0, slot.data(), 384, &nt);
        out6[2 * k + 1] = nt;
    }
    return 0;
}

// [seeds, ranges, LDS bytes] of the kernel's first and second geometry, then of `tiny`
extern "C" int sc_chain_geometry(int32_t *out9) {
    out9[0] = ChainLdsSmall::SEEDS, out9[1] = ChainLdsSmall::RANGES, out9[2] = (int32_t)sizeof(ChainLdsSmall);
    out9[3] = ChainLdsLarge::SEEDS, out9[4] = ChainLdsLarge::RANGES, out9[5] = (int32_t)sizeof(ChainLdsLarge);
    out9[6] = 64, out9[7] = 32, out9[8] = OCC_MAX;
    return 0;
}

#ifdef SC_MAIN
// random long reads, short reads cut from them with errors, an N, repeats and empty reads;
// both option sets, every geometry; exit status 1 on any difference
int main() {
    unsigned long long x = 88172645463325252ull;
    auto rnd = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (unsigned)(x >> 11); };
    std::vector<uint8_t> lr;
    std::vector<int64_t> lo{0};
    std::vector<uint8_t> unit(300);
    for (auto &b : unit) b = (uint8_t)(rnd() & 3);
    for (int r = 0; r < 6; ++r) {
        const int n = 1000 + (int)(rnd() % 1000);
        for (int k = 0; k < n; ++k) lr.push_back(r >= 4 ? unit[(size_t)(k % 300)] : (uint8_t)(rnd() & 3));
        lo.push_back((int64_t)lr.size());
    }
    pr_seed_index *h = nullptr;
    if (pr_seed_index_build(lr.data(), lo.data(), (int)lo.size() - 1, &h)) return 2;
    std::vector<uint8_t> sr;
    std::vector<int64_t> so{0};
    for (int i = 0; i < 300; ++i) {
        const int len = i % 37 == 0 ? 0 : i % 11 == 0 ? 5 + (int)(rnd() % 7) : i % 50 == 1 ? 500 : 60 + (int)(rnd() % 120);
        const int64_t p = (int64_t)(rnd() % (unsigned)(lr.size() - 600));
        for (int k = 0; k < len; ++k) {
            uint8_t b = lr[(size_t)(p + k)];
            if (rnd() % 100 < (unsigned)(i % 3 == 0 ? 0 : 8)) b = (uint8_t)(rnd() & 3);
            if (i % 13 == 0 && k == len / 2) b = 4;
            sr.push_back(b);
        }
        so.push_back((int64_t)sr.size());
    }
    const int n = (int)so.size() - 1;
    int bad = 0;
    for (int fin = 0; fin < 2; ++fin) {
        pr_seed_opts o;
        pr_seed_opts_default(&o, fin);
        if (fin) o.drop_ratio = 0.75;
        for (int geom = 0; geom < 3; ++geom) {
            std::vector<int32_t> res((size_t)n * NRES);
            sc_chain_compare(h, &o, sr.data(), so.data(), n, geom, 0, 0xAB, res.data());
            int flagged = 0;
            for (int i = 0; i < n; ++i) {
                bad += res[(size_t)i * NRES + 5] != 1;
                flagged += res[(size_t)i * NRES + 2] != 0;
            }
            std::printf("finish=%d geom=%d reads=%d flagged=%d\n", fin, geom, n, flagged);
        }
    }
    pr_seed_index_free(h);
    std::printf("%s\n", bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
#endif

// Host build of the seeding driver's planning (proovread_amd/csrc/seed_plan.h, and seed_core.h's
// grow_caps) for tests/test_seed_plan.py, next to the arithmetic it replaced: the parent_*
// functions are the expressions pr_seed_gpu_map and pr_seed_map_device_caps had inline before
// the split, copied once, verbatim.  plan_case runs one case through either.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../proovread_amd/csrc/seed_plan.h"

using namespace prgpu;

// --- the parent's inline expressions ---------------------------------------------------------
static int64_t parent_budget(size_t fr, int64_t have) {
    const int64_t budget = std::min<int64_t>((int64_t)40 << 30,
                                             std::max<int64_t>((int64_t)24 << 30, ((int64_t)fr + have) * 15 / 100));
    return budget;
}
static int64_t parent_wmax(int n_cu, int64_t budget, int64_t stride) {
    const int64_t wmax = std::max<int64_t>(n_cu, budget / (64 * stride));
    return wmax;
}
static int64_t parent_waves(int n_sr, int n_cu, const char *wpc, bool balance, int64_t wmax) {
    int64_t waves = (int64_t)n_cu * (wpc ? atoi(wpc) : 16);   // ~98 KB x 64 slices per wave at 150 bp
    const int64_t nbatch = (n_sr + 63) / 64;
    if (waves > nbatch) waves = nbatch;
    if (waves < 1) waves = 1;
    if (balance) {
        const int64_t rounds = (nbatch + waves - 1) / waves;
        waves = (nbatch + rounds - 1) / rounds;
    }
    if (waves > wmax) waves = wmax;
    return waves;
}
static int64_t parent_chunk(int64_t out_budget, int64_t slot_bytes) {
    const int64_t chunk = std::max<int64_t>(64, out_budget / slot_bytes / 64 * 64);
    return chunk;
}
static seedc::Caps parent_cb(const seedc::Caps &small, int32_t fl1, int64_t need_hits) {
    seedc::Caps cb = small;
    if (fl1 & seedc::SC_OVER_HITS) {
        cb.hits = (int32_t)std::min<int64_t>(std::max<int64_t>((int64_t)cb.hits + 512, (need_hits + need_hits / 8 + 511) & ~(int64_t)511),
                                             (int64_t)1 << 20);
        const int64_t f = std::min<int64_t>(16, std::max<int64_t>(1, cb.hits / small.hits));
        cb.chains = (int32_t)(cb.chains * f);
        cb.seeds = (int32_t)(cb.seeds * f);
    }
    if (fl1 & seedc::SC_OVER_IV) cb.iv *= 2;
    if (fl1 & seedc::SC_OVER_MEMS) cb.mems *= 2;
    if (fl1 & seedc::SC_OVER_SEEDS) cb.seeds *= 2;
    if (fl1 & seedc::SC_OVER_CHAINS) cb.chains *= 2;
    return cb;
}
static seedc::Caps parent_cw(const seedc::Caps &caps, const seedc::Caps &cb) {
    seedc::Caps cw = caps;
    cw.hits = std::max(caps.hits, cb.hits);
    cw.iv = std::max(caps.iv, cb.iv);
    cw.mems = std::max(caps.mems, cb.mems);
    cw.seeds = std::max(caps.seeds, cb.seeds);
    cw.chains = std::max(caps.chains, cb.chains);
    return cw;
}
// (the grown buffer's bytes: want, 0 when the parent kept the buffer)
static int64_t parent_scratch_want(int64_t waves, size_t n_redo, int64_t sb, size_t fr, int64_t have) {
    const int64_t budget = parent_budget(fr, have);
    const int64_t want = std::min<int64_t>(waves, ((int64_t)n_redo + 63) / 64) * 64 * sb;
    if (want > have && want <= budget) return want;
    return 0;
}
static int64_t parent_wb(int64_t cap, int64_t sb, size_t n_redo, int64_t waves) {
    int64_t wb = std::min<int64_t>((int64_t)cap / (64 * sb), ((int64_t)n_redo + 63) / 64);
    wb = std::min<int64_t>(wb, waves);   // (the filter rows' area holds `waves` waves)
    return wb;
}
static bool parent_by_wave(const char *p1b, int64_t need_sum, int64_t need_n, const seedc::Caps &small) {
    const bool by_wave = p1b ? !strcmp(p1b, "wave") : need_sum > 4 * (int64_t)small.hits * need_n;
    return by_wave;
}
static int64_t parent_ww(int64_t lanes2, size_t n_redo, int64_t cap, int64_t sw) {
    const int64_t ww = std::min<int64_t>(std::min<int64_t>(lanes2, (int64_t)n_redo), (int64_t)cap / sw);
    return ww;
}
// 0 skip, 1 lane per read, 2 wave per read
static int parent_mode(size_t n_redo, int32_t fl1, bool by_wave, int64_t wb, int64_t ww, int n_cu) {
    if (n_redo > 4096 && !(fl1 & (seedc::SC_OVER_LEN | seedc::SC_OVER_OUT))) {
        if (by_wave && ww >= n_cu) {
            return 2;
        } else if (wb >= n_cu) {
            return 1;
        }
    }
    return 0;
}
// the three growth rules: pass 1b (after its hit tables), the later passes, the host emulation
static seedc::Caps parent_grow_1b(seedc::Caps cb, int32_t fl1) {
    if (fl1 & seedc::SC_OVER_IV) cb.iv *= 2;
    if (fl1 & seedc::SC_OVER_MEMS) cb.mems *= 2;
    if (fl1 & seedc::SC_OVER_SEEDS) cb.seeds *= 2;
    if (fl1 & seedc::SC_OVER_CHAINS) cb.chains *= 2;
    return cb;
}
static seedc::Caps parent_grow_later(seedc::Caps cg, int32_t fl) {
    if (fl & seedc::SC_OVER_HITS) cg.hits *= 4;
    if (fl & seedc::SC_OVER_IV) cg.iv *= 2;
    if (fl & seedc::SC_OVER_MEMS) cg.mems *= 2;
    if (fl & seedc::SC_OVER_SEEDS) cg.seeds *= 2;
    if (fl & seedc::SC_OVER_CHAINS) cg.chains *= 2;
    return cg;
}
static seedc::Caps parent_grow_host(seedc::Caps cg, int err) {
    if (err & seedc::SC_OVER_HITS) cg.hits *= 4;
    if (err & seedc::SC_OVER_IV) cg.iv *= 2;
    if (err & seedc::SC_OVER_MEMS) cg.mems *= 2;
    if (err & seedc::SC_OVER_SEEDS) cg.seeds *= 2;
    if (err & seedc::SC_OVER_CHAINS) cg.chains *= 2;
    return cg;
}

// --- one case through either ------------------------------------------------------------------
enum In { I_QLEN, I_LAZY, I_FLAGS, I_NFLAGGED, I_NEED_MAX, I_NEED_SUM, I_NEED_N, I_FREE, I_HAVE, I_NCU, I_WPC, I_BALANCE,
          I_NSR, I_LANES2, I_FORCE, I_OUT_BUDGET, I_COUNT };
enum Out { O_BUDGET, O_WMAX, O_WAVES, O_CHUNK, O_CB, O_CW = O_CB + 10, O_WANT = O_CW + 10, O_CAP, O_WB, O_WW, O_BY_WAVE,
           O_MODE, O_COUNT };

static void put_caps(int64_t *o, const seedc::Caps &c) {
    const int32_t v[10] = {c.lmax, c.hits, c.iv, c.mems, c.seeds, c.chains, c.out, c.hi, c.nopos, c.lazy};
    for (int k = 0; k < 10; ++k) o[k] = v[k];
}
static void case_caps(const int64_t *in, seedc::Caps &small, seedc::Caps &caps) {
    caps = seedc::device_caps((int)in[I_QLEN]);
    caps.nopos = 1;
    small = seedc::device_caps_small(std::min((int)in[I_QLEN], caps.lmax));
    small.nopos = 1;
    small.lazy = (int32_t)in[I_LAZY];
}

extern "C" int plan_in_count() { return I_COUNT; }
extern "C" int plan_out_count() { return O_COUNT; }

// which: 0 the parent's expressions, 1 seed_plan.h.  keep_scratch: pass 1b's wave counts from the
// buffer as it is (have), whatever the growth decision; else from the buffer after the decision
// (DevBuf::ensure allocates want + 64 bytes).
extern "C" void plan_case(const int64_t *in, int which, int keep_scratch, int64_t *out) {
    seedc::Caps small, caps;
    case_caps(in, small, caps);
    const int64_t stride = seedc::scratch_bytes(small), slot_bytes = (int64_t)caps.out * (int64_t)sizeof(pr_seed_task);
    const int n_cu = (int)in[I_NCU], n_sr = (int)in[I_NSR];
    const int32_t fl = (int32_t)in[I_FLAGS];
    const int64_t fr = in[I_FREE], have = in[I_HAVE], lanes2 = in[I_LANES2], n_fl = in[I_NFLAGGED];
    char wpc[32];
    snprintf(wpc, sizeof wpc, "%d", (int)in[I_WPC]);
    const char *force = in[I_FORCE] == 0 ? nullptr : in[I_FORCE] == 1 ? "lane" : "wave";
    memset(out, 0, sizeof(int64_t) * O_COUNT);
    if (which == 0) {
        out[O_BUDGET] = parent_budget((size_t)fr, have);
        out[O_WMAX] = parent_wmax(n_cu, out[O_BUDGET], stride);
        out[O_WAVES] = parent_waves(n_sr, n_cu, in[I_WPC] ? wpc : nullptr, in[I_BALANCE] != 0, out[O_WMAX]);
        out[O_CHUNK] = parent_chunk(in[I_OUT_BUDGET], slot_bytes);
        const seedc::Caps cb = parent_cb(small, fl, in[I_NEED_MAX]), cw = parent_cw(caps, cb);
        put_caps(out + O_CB, cb);
        put_caps(out + O_CW, cw);
        const int64_t sb = seedc::scratch_bytes(cb), sw = seedc::scratch_bytes(cw);
        out[O_WANT] = parent_scratch_want(out[O_WAVES], (size_t)n_fl, sb, (size_t)fr, have);
        out[O_CAP] = out[O_WANT] && !keep_scratch ? out[O_WANT] + 64 : have;
        out[O_WB] = parent_wb(out[O_CAP], sb, (size_t)n_fl, out[O_WAVES]);
        out[O_BY_WAVE] = parent_by_wave(force, in[I_NEED_SUM], in[I_NEED_N], small);
        out[O_WW] = parent_ww(lanes2, (size_t)n_fl, out[O_CAP], sw);
        out[O_MODE] = parent_mode((size_t)n_fl, fl, out[O_BY_WAVE] != 0, out[O_WB], out[O_WW], n_cu);
        return;
    }
    out[O_BUDGET] = seedp::scratch_budget(fr, have);
    out[O_WMAX] = seedp::pass1_wave_cap(n_cu, out[O_BUDGET], stride);
    out[O_WAVES] = seedp::pass1_waves(n_sr, n_cu, in[I_WPC] ? (int)in[I_WPC] : 16, in[I_BALANCE] != 0, out[O_BUDGET], stride);
    out[O_CHUNK] = seedp::out_chunk(in[I_OUT_BUDGET], slot_bytes);
    seedp::Flagged f;
    f.n = n_fl;
    f.flags = fl;
    f.need_max = in[I_NEED_MAX];
    f.need_sum = in[I_NEED_SUM];
    f.need_n = in[I_NEED_N];
    const seedp::Pass1bCaps p = seedp::pass1b_caps(small, caps, f);
    put_caps(out + O_CB, p.cb);
    put_caps(out + O_CW, p.cw);
    out[O_WANT] = seedp::pass1b_scratch_want(out[O_WAVES], n_fl, p.sb, fr, have);
    out[O_CAP] = out[O_WANT] && !keep_scratch ? out[O_WANT] + 64 : have;
    const seedp::Pass1bRun r = seedp::pass1b_run(p, f, small.hits, (seedp::Pass1bForce)in[I_FORCE], out[O_CAP], out[O_WAVES],
                                                 lanes2, n_cu);
    out[O_WB] = r.wb;
    out[O_WW] = r.ww;
    out[O_BY_WAVE] = r.by_wave;
    out[O_MODE] = r.mode;
}

// Flagged::add over (status, n_out) pairs against the parent's loop: -> n, flags, need_max, need_sum, need_n
extern "C" void flagged_case(const int32_t *st1, const int32_t *no1, int64_t n, int which, int64_t *out5) {
    if (which == 0) {
        int64_t n_redo = 0;
        int32_t fl1 = 0;
        int64_t need_hits = 0;   // the largest hit table a flagged read asked for
        int64_t need_sum = 0, need_n = 0;   // (and their mean)
        for (int64_t i = 0; i < n; ++i)
            if (st1[(size_t)i]) {
                ++n_redo;
                fl1 |= st1[(size_t)i];
                need_hits = std::max<int64_t>(need_hits, -(int64_t)no1[(size_t)i]);
                if (no1[(size_t)i] < 0) need_sum -= no1[(size_t)i], ++need_n;
            }
        const int64_t v[5] = {n_redo, fl1, need_hits, need_sum, need_n};
        memcpy(out5, v, sizeof v);
        return;
    }
    seedp::Flagged f;
    for (int64_t i = 0; i < n; ++i)
        if (st1[i]) f.add(st1[i], no1[i]);
    const int64_t v[5] = {f.n, f.flags, f.need_max, f.need_sum, f.need_n};
    memcpy(out5, v, sizeof v);
}

// grow_caps against the three parent copies: which 0 / 1 / 2 = pass 1b / later passes / host
// emulation, 3 / 4 = grow_caps with the hits factor 1 / 4; caps of read length qlen -> out10
extern "C" void grow_case(int qlen, int small, int32_t flags, int which, int64_t *out10) {
    seedc::Caps c = small ? seedc::device_caps_small(qlen) : seedc::device_caps(qlen);
    c = which == 0 ? parent_grow_1b(c, flags) : which == 1 ? parent_grow_later(c, flags) : which == 2 ? parent_grow_host(c, flags)
        : seedc::grow_caps(c, flags, which == 3 ? 1 : 4);
    put_caps(out10, c);
}

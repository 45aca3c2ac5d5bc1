// Planning of the device seeding's passes (the driver in seed_api.cpp): scratch budget, wave
// counts, chunk size, pass 1b's capacities and its lane / wave / skip decision, as plain
// functions of numbers.  No HIP and no environment here: the driver reads the free memory and
// the tuning hooks and passes them in, and tests/native/seed_plan_host.cpp drives these on the host.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "seed_chain.h"
#include "seed_core.h"

namespace prgpu {
namespace seedp {

// The scratch budget of pass 1's slices: 15 % of the free device memory, between 24 and
// 40 GB (configs[1]'s 16 waves per CU need ~32 GB; long mr reads: fewer waves).  (Round 4
// capped it at 24 GB, which cut configs[1] to ~3,800 of its 4,096 waves.)
// have: the bytes SB_SCRATCH already holds (already ours: counts as free)
inline int64_t scratch_budget(int64_t free_bytes, int64_t have) {
    return std::min<int64_t>((int64_t)40 << 30, std::max<int64_t>((int64_t)24 << 30, (free_bytes + have) * 15 / 100));
}
// Growing SB_SCRATCH for pass 1b is only a speed-up, and the buffer is freed before the larger
// one is allocated, so it may take at most 1/2 of what is then free: the 24 GB floor of the
// budget can lie above the memory a crowded device has, and a failed allocation ends the map.
inline bool scratch_growth_fits(int64_t want, int64_t free_bytes, int64_t have) { return want <= (free_bytes + have) / 2; }

// Pass 1's budget: scratch_budget, or what every resident wave's slices need (`full`: 16 waves per
// CU x 64 slices) where that is more, within the 40 GB ceiling and a quarter of the free memory.
// Inside the correction loop the other stages hold ~130 GB, 15 % of the rest is under the 24 GB
// floor, and the floor holds ~3,700 of configs[1]'s 4,096 waves (they need 26.6 to 28 GB): the
// lane phase is latency-bound and lost ~3 % per launch to the missing waves.
inline int64_t pass1_budget(int64_t free_bytes, int64_t have, int64_t full) {
    const int64_t b = scratch_budget(free_bytes, have);
    return full > b && full <= ((int64_t)40 << 30) && full <= (free_bytes + have) / 4 ? full : b;
}
// waves of pass 1 that the budget holds (64 slices of `stride` bytes each), a wave per CU at least
inline int64_t pass1_wave_cap(int n_cu, int64_t budget, int64_t stride) {
    return std::max<int64_t>(n_cu, budget / (64 * stride));
}
// pass 1's waves: waves_per_cu a CU (16: ~98 KB x 64 slices per wave at 150 bp), no more than
// 64-read batches, within the budget
inline int64_t pass1_waves(int64_t n_sr, int n_cu, int waves_per_cu, bool balance, int64_t budget, int64_t stride) {
    int64_t waves = (int64_t)n_cu * waves_per_cu;
    const int64_t nbatch = (n_sr + 63) / 64;
    if (waves > nbatch) waves = nbatch;
    if (waves < 1) waves = 1;
    // PRGPU_SEED_BALANCE: every wave the same number of 64-read batches (fewer waves; measured
    // slower at configs[1], 357 vs 345 ms: the lane phase wants every wave it can get)
    if (balance) {
        const int64_t rounds = (nbatch + waves - 1) / waves;
        waves = (nbatch + rounds - 1) / rounds;
    }
    return std::min(waves, pass1_wave_cap(n_cu, budget, stride));
}

// Pass 1's hit budget per read when the table is lazy (seed_api.cpp map_plan), 0: none.  Measured at
// configs[1]'s finish task: 1536 - 2048 hits flag 404 - 153 of 914 k reads and gain
// about 1 ms of 93, within the runs' spread; 1024 and below cost more in the next pass than pass 1
// saves.  So none by default; PRGPU_SEED_BUDGET sets one.
constexpr int32_t PASS1_LAZY_BUDGET = 0;

// The budget of a chunk's output slabs: a tenth of the free device memory, between 8 and 16 GB.
// A chunk is a pass-1 launch with its own drain (the last batches run on a mostly idle device),
// status download and compaction, so a task should be one chunk where the memory allows: the
// finish task's 914 k reads of configs[1] need 14 GB and ran as two launches under the fixed 8 GB
// (seeding 107 -> 94 ms); a crowded device keeps the 8 GB.
// have: the bytes SB_OUT already holds
inline int64_t out_budget(int64_t free_bytes, int64_t have) {
    return std::min<int64_t>((int64_t)16 << 30, std::max<int64_t>((int64_t)8 << 30, (free_bytes + have) / 10));
}
// reads per chunk: their output slabs (slot_bytes a read) within out_budget, a multiple of 64
inline int64_t out_chunk(int64_t out_budget, int64_t slot_bytes) {
    return std::max<int64_t>(64, out_budget / slot_bytes / 64 * 64);
}

// The pool of the lane passes' occurrence lists (seed_chain.h), in 8-byte words: what the chunk's
// reads hand over on average with room to spare (occ_words_per_read) plus one read's largest
// list, within 8 GB (configs[1]'s 460 k reads: 2,330 words or 1,550 occurrences a read) and a sixteenth of the free device
// memory, and at least that one list.  A read that finds the pool full is flagged and takes the
// later passes, so a crowded device or a larger sample loses speed only.
// have: the bytes SB_OCC already holds
inline int64_t occ_pool_words(int64_t n_reads, bool lazy, int64_t free_bytes, int64_t have) {
    const int64_t one = seedc::occ_words(seedc::OCC_MAX);
    const int64_t want = n_reads * seedc::occ_words_per_read(lazy) + one;
    const int64_t lim = std::min<int64_t>((int64_t)8 << 30, (free_bytes + have) / 16) / 8;
    return std::max<int64_t>(one, std::min<int64_t>(want, lim));
}

// what pass 1 left of a chunk: the flagged reads, their flags or-ed, and the hit tables they
// asked for (a flagged read's n_out is minus the hits it would need): largest, sum and count
struct Flagged {
    int64_t n = 0;
    int32_t flags = 0;
    int64_t need_max = 0, need_sum = 0, need_n = 0;
    void add(int32_t status, int32_t n_out) {
        ++n;
        flags |= status;
        need_max = std::max<int64_t>(need_max, -(int64_t)n_out);
        if (n_out < 0) need_sum -= n_out, ++need_n;
    }
};

// Pass 1b.  Many flagged reads (the finish task maps to corrected reads at 30x long-read
// coverage: ~140 starts x 30 hits > 4096 for nearly every read): pass 1 again over them with the
// arrays that overflowed grown, instead of pass 2's one wave per read.  Reads too long for any
// slice or with more seeds than output slots stay flagged whatever the scratch.
inline bool pass1b_wanted(const Flagged &f) { return f.n > 4096 && !(f.flags & (seedc::SC_OVER_LEN | seedc::SC_OVER_OUT)); }

struct Pass1bCaps {
    seedc::Caps cb;   // lane per read: pass 1's slices grown
    seedc::Caps cw;   // wave per read: pass 2's slices, no array smaller than cb's
    int64_t sb, sw;   // scratch_bytes of either
};
// small / caps: pass 1's and pass 2's capacities
inline Pass1bCaps pass1b_caps(const seedc::Caps &small, const seedc::Caps &caps, const Flagged &f) {
    Pass1bCaps p;
    p.cb = small;
    // the hit tables sized for the largest flagged read (dense indexes: configs[2] /
    // configs[3], or N > 1 ranks of the exact layout, every read overflows pass 1)
    if (f.flags & seedc::SC_OVER_HITS) {
        // the largest flagged read's hit table (+ 1/8), not a multiple of pass 1's: the finish
        // task's reads need just over pass 1's 4096 hits, and 4x slices cut the waves in flight
        // (the occurrence table is latency-bound: 413 -> measured in DESIGN.md §5 round 6)
        p.cb.hits = (int32_t)std::min<int64_t>(
            std::max<int64_t>((int64_t)p.cb.hits + 512, (f.need_max + f.need_max / 8 + 511) & ~(int64_t)511), (int64_t)1 << 20);
        // their chaining never ran; random 12-mer hits become chains and seeds in
        // proportion to the hits, so those arrays grow by the same factor
        const int64_t g = std::min<int64_t>(16, std::max<int64_t>(1, p.cb.hits / small.hits));
        p.cb.chains = (int32_t)(p.cb.chains * g);
        p.cb.seeds = (int32_t)(p.cb.seeds * g);
    }
    p.cb = seedc::grow_caps(p.cb, f.flags, 1);
    p.cw = caps;
    p.cw.hits = std::max(caps.hits, p.cb.hits);
    p.cw.iv = std::max(caps.iv, p.cb.iv);
    p.cw.mems = std::max(caps.mems, p.cb.mems);
    p.cw.seeds = std::max(caps.seeds, p.cb.seeds);
    p.cw.chains = std::max(caps.chains, p.cb.chains);
    p.sb = seedc::scratch_bytes(p.cb);
    p.sw = seedc::scratch_bytes(p.cw);
    return p;
}
// The bytes to grow SB_SCRATCH to before pass 1b, 0: go on with what it holds.  Room for as many
// waves as pass 1 ran (or the flagged reads' batches), within pass 1's budget and the free memory.
inline int64_t pass1b_scratch_want(int64_t waves, int64_t n_flagged, int64_t sb, int64_t free_bytes, int64_t have) {
    const int64_t want = std::min<int64_t>(waves, (n_flagged + 63) / 64) * 64 * sb;
    return want > have && want <= scratch_budget(free_bytes, have) && scratch_growth_fits(want, free_bytes, have) ? want : 0;
}

enum Pass1bMode { P1B_SKIP, P1B_LANE, P1B_WAVE };
enum Pass1bForce { P1B_AUTO, P1B_FORCE_LANE, P1B_FORCE_WAVE };   // PRGPU_SEED_1B
struct Pass1bRun {
    bool by_wave;
    int64_t wb;   // waves of the lane-per-read launch that the scratch holds
    int64_t ww;   // waves (= reads in flight) of the wave-per-read launch
    Pass1bMode mode;
};
// scratch_cap: SB_SCRATCH's bytes after the growth; waves: pass 1's (the filter rows' area holds
// that many); lanes2: pass 2's resident waves
inline Pass1bRun pass1b_run(const Pass1bCaps &p, const Flagged &f, int32_t small_hits, Pass1bForce force, int64_t scratch_cap,
                            int64_t waves, int64_t lanes2, int n_cu) {
    Pass1bRun r;
    r.wb = std::min<int64_t>(std::min<int64_t>(scratch_cap / (64 * p.sb), (f.n + 63) / 64), waves);
    // reads that need more than 4x pass 1's hits on average (dense indexes: configs[2] / [3]) one wave
    // each (seed_wave_kernel: the chaining over the lanes) with pass 2's slices grown like
    // cb: 64 such slices per wave fit only a few hundred waves in the scratch (a configs[3]
    // rank's seeding 17.4 -> 4.1 s, configs[2] 1.01 -> 0.82 s).  The finish task's reads
    // (just over pass 1's hits, ~30x coverage) stay lane per read (620 vs 724 ms as waves).
    // PRGPU_SEED_1B=wave / lane forces either.
    r.by_wave = force != P1B_AUTO ? force == P1B_FORCE_WAVE : f.need_sum > 4 * (int64_t)small_hits * f.need_n;
    r.ww = std::min<int64_t>(std::min<int64_t>(lanes2, f.n), scratch_cap / p.sw);
    r.mode = !pass1b_wanted(f) ? P1B_SKIP : r.by_wave && r.ww >= n_cu ? P1B_WAVE : r.wb >= n_cu ? P1B_LANE : P1B_SKIP;
    return r;
}

// Pass 1b, lane per read, of a lazy-table task: the reads a wave dequeues at a time (= its slices)
// and the waves.  The flagged reads of a finish task are a heavy minority (a few ten thousand of
// ~900 k): at 64 a wave they fill a few hundred of pass 1's waves and the launch is as long as
// one wave's 64 occurrence tables and its slowest lane on a mostly idle device.  So one batch
// per wave over as many waves as pass 1 ran: n reads -> ceil(n / waves) a wave.  Waves beyond
// the scratch's room (batch slices each) are dropped; the rest then dequeue more than once.
// r: pass1b_run's result (wb: the waves at 64 reads each, the floor when nothing else fits);
// force: PRGPU_SEED_1B_BATCH (0: none)
struct Pass1bBatch {
    int32_t batch;   // 1 .. 64
    int64_t waves;
};
inline Pass1bBatch pass1b_batch(const Pass1bRun &r, int64_t n_flagged, int64_t waves, int64_t scratch_cap, int64_t sb,
                                int force) {
    Pass1bBatch b;
    waves = std::max<int64_t>(waves, 1);
    const int64_t per = force > 0 ? force : (n_flagged + waves - 1) / waves;
    b.batch = (int32_t)std::min<int64_t>(64, std::max<int64_t>(1, per));
    b.waves = std::min<int64_t>(std::min<int64_t>((n_flagged + b.batch - 1) / b.batch, waves), scratch_cap / (b.batch * sb));
    if (b.waves < 1) b.batch = 64, b.waves = r.wb;   // (at 64 a wave the result is wb itself)
    return b;
}

}  // namespace seedp
}  // namespace prgpu

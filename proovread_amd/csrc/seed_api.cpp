// Seeding on the device (seed_kernels.hip over seed_core.h), the pr_seed_gpu_* and pr_srset_*
// entry points of include/prgpu.h: the index copied to or built in HBM, the resident short
// reads, and the map's host driver (its planning arithmetic: seed_plan.h).
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "seed_index_dev.h"
#include "seed_plan.h"

// the index text 16 bases per word (IndexView.text4) for the occurrence table's match lengths
static int seed_text4(pr_ctx *c, seedc::IndexView &v, hipStream_t s) {
    int rc = c->sd[SI_TEXT4].ensure((size_t)ix_pack4_words(v.n_text) * 8);
    if (rc) return rc;
    const int e = ix_pack4_launch(v.text, v.n_text, c->sd[SI_TEXT4].as<uint64_t>(), s);
    if (e) return set_error(PR_ERR_HIP, "text packing: %s", hipGetErrorString((hipError_t)e));
    v.text4 = c->sd[SI_TEXT4].as<uint64_t>();
    // dense indexes (> 64 hits per 12-mer on average: configs[2] / [3] at one rank's share): the
    // by-wave pass walks 16 bases per text round trip (seed_wave_kernel<1>: no 5-word buffers,
    // more waves resident), the others 64 (tools/ab_scale.sh: profiles/r06_walk_ab.txt)
    v.walk_nw = v.n_text > ((int64_t)64 << 24) ? 1 : 4;
    if (const char *w = getenv("PRGPU_SEED_WALK_NW"))   // tuning hook: 1 or 4
        v.walk_nw = atoi(w) == 1 ? 1 : 4;
    return 0;
}

// Per 2^CB_SHIFT text block: the contig at its start, the next two contig starts inside it and
// the coordinate offsets of those contigs (fr = p + delta, seed_core.h text_to_fr), so the
// seeding's hit pass computes a hit's bwa coordinate with one table load instead of the cblk ->
// cstart -> lr_off chain.  cstart / off: host arrays of the index (off rebased to 0).
static int upload_blk_fr(pr_ctx *c, seedc::IndexView &v, const int64_t *cstart, const int64_t *off, int n_lr,
                         int64_t l_pac, int64_t n_text, hipStream_t s) {
    const int64_t nb = (n_text >> seedc::CB_SHIFT) + 1;
    const int nc = 2 * n_lr;
    const int bs = 1 << seedc::CB_SHIFT;
    auto delta = [&](int ci) -> int64_t {
        if (ci < n_lr) return off[ci] - cstart[ci];
        const int rid = 2 * n_lr - 1 - ci;   // the reverse half holds the long reads in reverse order
        return 2 * l_pac - off[rid + 1] - cstart[ci];
    };
    std::vector<seedc::BlkFr> t((size_t)nb);
    int ci = 0;
    for (int64_t b = 0; b < nb; ++b) {
        const int64_t b0 = b << seedc::CB_SHIFT, b1 = b0 + bs;
        while (ci + 1 < nc && cstart[ci + 1] <= b0) ++ci;
        seedc::BlkFr &e = t[(size_t)b];
        e.c0 = ci;
        e.d0 = nc ? delta(ci) : 0;
        e.d1 = ci + 1 < nc ? delta(ci + 1) : 0;
        e.bnd = ci + 1 < nc && cstart[ci + 1] < b1 ? (int32_t)(cstart[ci + 1] - b0) : bs;
        e.bnd2 = ci + 2 < nc && cstart[ci + 2] < b1 ? (int32_t)(cstart[ci + 2] - b0) : bs;
    }
    int rc = c->sd[SI_BLKFR].ensure(t.size() * sizeof(seedc::BlkFr));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->sd[SI_BLKFR].p, t.data(), t.size() * sizeof(seedc::BlkFr), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // (t is a host temporary)
    v.blkfr = c->sd[SI_BLKFR].as<seedc::BlkFr>();
    return 0;
}

extern "C" int pr_seed_gpu_upload(pr_ctx *c, const pr_seed_index *h) {
    if (!c || !h) return set_error(PR_ERR_ARG, "null arg");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const seedc::IndexView hv = seed_index_view(h);
    const SeedIndexSizes z = seed_index_sizes(h);
    DevBuf *D = c->sd;
    int rc;
    if ((rc = upload(D[SI_TEXT], hv.text, (size_t)z.text, s)) || (rc = upload(D[SI_CSTART], hv.cstart, (size_t)z.cstart, s)) ||
        (rc = upload(D[SI_CBLK], hv.cblk, (size_t)z.cblk, s)) || (rc = upload(D[SI_LROFF], hv.lr_off, (size_t)z.lr_off, s)) ||
        (rc = upload(D[SI_KOFF], hv.koff, (size_t)z.koff, s)) || (rc = upload(D[SI_KPOS], hv.kpos, (size_t)z.kpos, s)) ||
        (rc = upload(D[SI_KEXT], hv.kext, (size_t)z.kpos, s)) ||
        (z.ksplit && (rc = upload(D[SI_KSPLIT], hv.ksplit, (size_t)z.ksplit, s))))
        return rc;
    seedc::IndexView v = hv;
    for (int j = 0; j < seedc::KI - 1; ++j) {
        if ((rc = upload(D[SI_CNT0 + j], hv.cnt[j], (size_t)z.cnt[j], s))) return rc;
        v.cnt[j] = D[SI_CNT0 + j].as<uint32_t>();
    }
    v.text = D[SI_TEXT].as<uint8_t>();
    v.cstart = D[SI_CSTART].as<int64_t>();
    v.cblk = D[SI_CBLK].as<int32_t>();
    v.lr_off = D[SI_LROFF].as<int64_t>();
    v.koff = D[SI_KOFF].as<uint64_t>();
    v.kpos = D[SI_KPOS].as<uint32_t>();
    v.kext = D[SI_KEXT].as<uint64_t>();
    v.ksplit = z.ksplit ? D[SI_KSPLIT].as<uint64_t>() : nullptr;
    if ((rc = seed_text4(c, v, s))) return rc;
    if ((rc = upload_blk_fr(c, v, hv.cstart, hv.lr_off, hv.n_lr, hv.l_pac, hv.n_text, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    c->seed_view = v;
    c->seed_loaded = true;
    return 0;
}

// the small host tables of the device build: rebased read offsets, contig starts, 4 KB block -> contig
static void index_host_tables(const int64_t *lr_off, int n_lr, int64_t l_pac, int64_t n_text, std::vector<int64_t> &off,
                              std::vector<int64_t> &cstart, std::vector<int32_t> &cblk) {
    off.assign((size_t)n_lr + 1, 0);
    cstart.assign(2 * (size_t)n_lr, 0);
    for (int i = 0; i <= n_lr; ++i) off[(size_t)i] = lr_off[i] - (n_lr ? lr_off[0] : 0);
    for (int i = 0; i < n_lr; ++i) {
        cstart[(size_t)i] = off[(size_t)i] + i;
        cstart[2 * (size_t)n_lr - 1 - i] = l_pac + n_lr + (l_pac - off[(size_t)i + 1]) + (n_lr - 1 - i);
    }
    const int64_t nb = (n_text >> seedc::CB_SHIFT) + 1;
    cblk.assign((size_t)nb, 0);
    int ci = 0;
    const int nc = 2 * n_lr;
    for (int64_t b = 0; b < nb; ++b) {
        while (ci + 1 < nc && cstart[(size_t)ci + 1] <= (b << seedc::CB_SHIFT)) ++ci;
        cblk[(size_t)b] = ci;
    }
}

// text positions per sort of the device build
static int64_t index_sort_chunk(const DevBuf *D, int64_t n_text) {
    // sorts of up to 2^31 text positions when the device has room for their buffers (~16 bytes a
    // position + rocPRIM's temporaries: configs[2]'s 2.1 G-position text in one sort, 293 -> 151
    // ms), else 2^30 (a divisor of 2^32 either way; PRGPU_INDEX_CHUNK=k: 2^k, a test hook that
    // sends small texts through the chunked build)
    int64_t chunk = (int64_t)1 << 30;
    if (n_text > chunk) {
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        (void)hipGetLastError();
        const int64_t have = (int64_t)(D[SX_KEY0].cap + D[SX_KEY1].cap + D[SX_VAL0].cap + D[SX_VAL1].cap + D[SX_TEMP].cap);
        // (room for the bigger sort buffers with 64 GB to spare for the rest of the task)
        if ((int64_t)fr + have >= ((int64_t)1 << 31) * 20 + ((int64_t)64 << 30)) chunk = (int64_t)1 << 31;
    }
    if (const char *ch = getenv("PRGPU_INDEX_CHUNK")) {
        const int k = atoi(ch);
        if (k >= 16 && k <= 31) chunk = (int64_t)1 << k;
    }
    return chunk;
}

// the build's buffers, the long reads and the host tables on the device -> the kernels' descriptor
static int index_buffers(pr_ctx *c, const uint8_t *lr_seq, const int64_t *lr_off, int n_lr, bool lr_dev, int64_t l_pac,
                         int64_t n_text, int64_t chunk, const std::vector<int64_t> &off, const std::vector<int64_t> &cstart,
                         const std::vector<int32_t> &cblk, SeedIndexBuild &B) {
    hipStream_t s = c->stream;
    DevBuf *D = c->sd;
    const size_t nt = (size_t)(n_text > 0 ? n_text : 1);
    const bool chunked = n_text > chunk;
    const size_t ns = (size_t)(chunked ? chunk : (int64_t)nt);   // sort scratch entries
    const size_t temp = seed_index_temp_bytes((int64_t)ns);
    const size_t nk1 = (size_t)seedc::NK + 1;
    // hits <= 12-mer starts; kpos / kext sized by the text (the count is known after the build)
    int rc;
    if ((rc = upload(D[SX_LRSEQ], lr_dev ? nullptr : (n_lr ? lr_seq + lr_off[0] : lr_seq), (size_t)l_pac, s)) ||
        (rc = upload(D[SI_LROFF], off.data(), off.size(), s)) || (rc = upload(D[SI_CSTART], cstart.data(), cstart.size(), s)) ||
        (rc = upload(D[SI_CBLK], cblk.data(), cblk.size(), s)) || (rc = D[SI_TEXT].ensure(nt)) ||
        (rc = D[SX_KEY0].ensure(ns * 4)) || (rc = D[SX_KEY1].ensure(ns * 4)) || (rc = D[SX_VAL0].ensure(ns * 4)) ||
        (rc = D[SX_KC].ensure(nk1 * 4)) || (rc = D[SI_KOFF].ensure(nk1 * 8)) ||
        (rc = D[SI_KPOS].ensure(nt * 4)) || (rc = D[SI_KEXT].ensure(nt * 8)) || (rc = D[SX_TEMP].ensure(temp)) ||
        (rc = D[SX_CNTPTR].ensure(sizeof(uint32_t *) * (seedc::KI - 1))))
        return rc;
    if (chunked && ((rc = D[SX_VAL1].ensure(ns * 4)) || (rc = D[SX_KCC].ensure(nk1 * 4)) ||
                    (rc = D[SX_KOFFC].ensure(nk1 * 4)) || (rc = D[SX_KCUR].ensure(nk1 * 8))))
        return rc;
    const bool paged = n_text > (int64_t)seedc::POS_PAGE;
    if (paged && (rc = D[SI_KSPLIT].ensure(nk1 * 8))) return rc;
    if (lr_dev && l_pac) HIPCHK(hipMemcpyAsync(D[SX_LRSEQ].p, lr_seq + lr_off[0], (size_t)l_pac, hipMemcpyDeviceToDevice, s));
    uint32_t *cptr[seedc::KI - 1];
    for (int j = 1; j < seedc::KI; ++j) {
        if ((rc = D[SI_CNT0 + j - 1].ensure(((size_t)1 << (2 * j)) * 4))) return rc;
        cptr[j - 1] = B.cnt[j - 1] = D[SI_CNT0 + j - 1].as<uint32_t>();
    }
    HIPCHK(hipMemcpyAsync(D[SX_CNTPTR].p, cptr, sizeof cptr, hipMemcpyHostToDevice, s));
    B.lr_seq = D[SX_LRSEQ].as<uint8_t>();
    B.lr_off = D[SI_LROFF].as<int64_t>();
    B.n_lr = n_lr;
    B.l_pac = l_pac;
    B.cstart = D[SI_CSTART].as<int64_t>();
    B.n_text = n_text;
    B.text = D[SI_TEXT].as<uint8_t>();
    B.chunk = chunk;
    B.key0 = D[SX_KEY0].as<uint32_t>();
    B.key1 = D[SX_KEY1].as<uint32_t>();
    B.val0 = D[SX_VAL0].as<uint32_t>();
    B.val1 = chunked ? D[SX_VAL1].as<uint32_t>() : nullptr;
    B.kc = D[SX_KC].as<uint32_t>();
    B.koff = D[SI_KOFF].as<uint64_t>();
    B.kcc = chunked ? D[SX_KCC].as<uint32_t>() : nullptr;
    B.koffc = chunked ? D[SX_KOFFC].as<uint32_t>() : nullptr;
    B.kcur = chunked ? D[SX_KCUR].as<uint64_t>() : nullptr;
    B.kpos = D[SI_KPOS].as<uint32_t>();
    B.kext = D[SI_KEXT].as<uint64_t>();
    B.ksplit = paged ? D[SI_KSPLIT].as<uint64_t>() : nullptr;
    B.cnt_dev = reinterpret_cast<uint32_t *const *>(D[SX_CNTPTR].p);
    B.temp = D[SX_TEMP].p;
    B.temp_bytes = temp;
    return 0;
}

// the seed index built in HBM (seed_index.hip): the tables of pr_seed_index_build
// lr_dev: lr_seq is a device pointer (the resident long-read set), copied on the device
int index_build(pr_ctx *c, const uint8_t *lr_seq, const int64_t *lr_off, int n_lr, bool lr_dev) {
    if (!c || n_lr < 0 || (n_lr && (!lr_seq || !lr_off))) return set_error(PR_ERR_ARG, "null arg");
    for (int i = 0; i < n_lr; ++i)
        if (lr_off[i + 1] < lr_off[i]) return set_error(PR_ERR_ARG, "lr_off not monotone");
    const int64_t l_pac = n_lr ? lr_off[n_lr] - lr_off[0] : 0;
    if (2 * l_pac + 2 * (int64_t)n_lr > seedc::MAX_TEXT)
        return set_error(PR_ERR_CAPACITY, "long reads beyond the index's 2^33 text positions (l_pac < 4.29 Gb)");
    if ((int64_t)n_lr >= ((int64_t)1 << seedc::FR_RID_BITS))
        return set_error(PR_ERR_CAPACITY, "more than 2^24 long reads in one index");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevBuf *D = c->sd;
    const int64_t n_text = 2 * l_pac + 2 * (int64_t)n_lr;
    std::vector<int64_t> off, cstart;
    std::vector<int32_t> cblk;
    index_host_tables(lr_off, n_lr, l_pac, n_text, off, cstart, cblk);
    SeedIndexBuild B{};
    int rc = index_buffers(c, lr_seq, lr_off, n_lr, lr_dev, l_pac, n_text, index_sort_chunk(D, n_text), off, cstart, cblk, B);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[8], s));
    const int e = seed_index_device_build(B, s);
    if (e) return set_error(PR_ERR_HIP, "seed index build: %s", hipGetErrorString((hipError_t)e));
    HIPCHK(hipEventRecord(c->ev[9], s));
    uint64_t nh = 0;
    HIPCHK(hipMemcpyAsync(&nh, B.koff + seedc::NK, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev[8], c->ev[9]) == hipSuccess) c->ms_index = ms;
    if (n_text > (int64_t)seedc::POS_PAGE) {
        // a build beyond 2^32 positions (configs[3] ranks) gives its sort buffers back (4 x 4-8 GB +
        // rocPRIM's temporaries): there a rank's device memory peaks near the card's 288 GiB later
        // in the task (DESIGN.md current status); smaller texts keep them for the next task's
        // build (no re-allocation inside a timed step)
        for (int id : {(int)SX_KEY0, (int)SX_KEY1, (int)SX_VAL0, (int)SX_VAL1, (int)SX_TEMP}) D[id].release();
    }
    seedc::IndexView v{};
    v.text = B.text;
    v.n_text = n_text;
    v.cstart = B.cstart;
    v.n_contig = 2 * n_lr;
    v.cblk = D[SI_CBLK].as<int32_t>();
    v.lr_off = B.lr_off;
    v.n_lr = n_lr;
    v.l_pac = l_pac;
    v.koff = B.koff;
    v.kpos = B.kpos;
    v.kext = B.kext;
    v.ksplit = B.ksplit;
    for (int j = 0; j < seedc::KI - 1; ++j) v.cnt[j] = B.cnt[j];
    if ((rc = seed_text4(c, v, s))) return rc;
    if ((rc = upload_blk_fr(c, v, cstart.data(), off.data(), n_lr, l_pac, n_text, s))) return rc;
    c->seed_view = v;
    c->seed_loaded = true;
    c->seed_n_text = n_text;
    c->seed_n_hits = nh;
    return 0;
}

extern "C" int pr_seed_gpu_index_build(pr_ctx *c, const uint8_t *lr_seq, const int64_t *lr_off, int n_lr) {
    return index_build(c, lr_seq, lr_off, n_lr, false);
}

// the six digests of pr_seed_index_digest over the device index (test hook)
extern "C" int pr_seed_gpu_index_digest(pr_ctx *c, uint64_t *out6) {
    if (!c || !out6) return set_error(PR_ERR_ARG, "null arg");
    if (!c->seed_loaded || !c->seed_n_text) return set_error(PR_ERR_ARG, "no device-built seed index");
    HIPCHK(hipSetDevice(c->device));
    const seedc::IndexView &v = c->seed_view;
    const size_t nt = (size_t)c->seed_n_text, nh = (size_t)c->seed_n_hits, nk = (size_t)seedc::NK;
    std::vector<uint8_t> text(nt);
    std::vector<uint64_t> koff(nk + 1);
    std::vector<uint32_t> kpos(nh), kc(nk);
    std::vector<uint64_t> kext(nh);
    std::vector<int64_t> cstart((size_t)v.n_contig), lro((size_t)v.n_lr + 1);
    std::vector<int32_t> cblk((size_t)((c->seed_n_text >> seedc::CB_SHIFT) + 1));
    std::vector<std::vector<uint32_t>> cnt(seedc::KI);
    HIPCHK(hipMemcpy(text.data(), v.text, nt, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(koff.data(), v.koff, (nk + 1) * 8, hipMemcpyDeviceToHost));
    if (nh) HIPCHK(hipMemcpy(kpos.data(), v.kpos, nh * 4, hipMemcpyDeviceToHost));
    if (nh) HIPCHK(hipMemcpy(kext.data(), v.kext, nh * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(kc.data(), c->sd[SX_KC].p, nk * 4, hipMemcpyDeviceToHost));
    if (!cstart.empty()) HIPCHK(hipMemcpy(cstart.data(), v.cstart, cstart.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lro.data(), v.lr_off, lro.size() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cblk.data(), v.cblk, cblk.size() * 4, hipMemcpyDeviceToHost));
    for (int j = 0; j < seedc::KI - 1; ++j) {
        cnt[(size_t)j].resize((size_t)1 << (2 * (j + 1)));
        HIPCHK(hipMemcpy(cnt[(size_t)j].data(), v.cnt[j], cnt[(size_t)j].size() * 4, hipMemcpyDeviceToHost));
    }
    cnt[seedc::KI - 1] = std::move(kc);
    std::vector<uint64_t> ksplit(v.ksplit ? nk : 0);
    if (v.ksplit) HIPCHK(hipMemcpy(ksplit.data(), v.ksplit, nk * 8, hipMemcpyDeviceToHost));
    seed_digest_tables(text, koff, kpos, kext, cnt, cstart, cblk, lro, ksplit, out6);
    return 0;
}

extern "C" int pr_seed_gpu_index_koff(pr_ctx *c, uint64_t *koff, uint64_t *ksplit) {
    if (!c || !koff) return set_error(PR_ERR_ARG, "null arg");
    if (!c->seed_loaded) return set_error(PR_ERR_ARG, "no device seed index");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(koff, c->seed_view.koff, ((size_t)seedc::NK + 1) * 8, hipMemcpyDeviceToHost));
    if (ksplit && c->seed_view.ksplit)
        HIPCHK(hipMemcpy(ksplit, c->seed_view.ksplit, (size_t)seedc::NK * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pr_seed_gpu_index_last_ms(pr_ctx *c, double *ms) {
    if (!c || !ms) return set_error(PR_ERR_ARG, "null arg");
    *ms = c->ms_index;
    return 0;
}

// the resident short reads (include/prgpu.h pr_srset_load): the whole short-read input once;
// a task's sample is gathered on the device from its record ranges
extern "C" int pr_srset_load(pr_ctx *c, int64_t n_sr, const int64_t *off, const uint8_t *seq) {
    if (!c || n_sr < 0 || !off || (off[n_sr] && !seq) || off[0] != 0) return set_error(PR_ERR_ARG, "bad arg");
    HIPCHK(hipSetDevice(c->device));
    int rc = upload(c->ls[LS_SRSEQ], seq, (size_t)off[n_sr], c->stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->ss_off.assign(off, off + n_sr + 1);
    c->ss_samp_off.clear();
    c->ls[LS_SRSAMP].release();
    return 0;
}

// The records [ranges[2k], ranges[2k+1]) of the resident short reads: their offsets from 0 ->
// off (at most max_reads reads), their bases gathered on the device into dst (stream-ordered)
static int gather_ranges(pr_ctx *c, const int64_t *ranges, int n_ranges, int64_t max_reads, DevBuf &dst,
                         std::vector<int64_t> &off) {
    if (c->ss_off.empty()) return set_error(PR_ERR_ARG, "no resident short reads (pr_srset_load)");
    const int64_t N = (int64_t)c->ss_off.size() - 1;
    off.assign(1, 0);
    for (int k = 0; k < n_ranges; ++k) {
        const int64_t r0 = ranges[2 * k], r1 = ranges[2 * k + 1];
        if (r0 < 0 || r1 < r0 || r1 > N) return set_error(PR_ERR_ARG, "record range outside the short reads");
        for (int64_t i = r0; i < r1; ++i) off.push_back(off.back() + c->ss_off[(size_t)i + 1] - c->ss_off[(size_t)i]);
    }
    if ((int64_t)off.size() - 1 > max_reads) return set_error(PR_ERR_CAPACITY, "too many short reads in one sample");
    HIPCHK(hipSetDevice(c->device));
    int rc = dst.ensure((size_t)off.back() + 1);
    if (rc) return rc;
    // the ranges' bytes (SeqChunker's chunks: several hundred a task; runs of consecutive chunks
    // merged) copied by one kernel, not one copy each
    std::vector<int64_t> so, dn, ln;
    int64_t at = 0;
    for (int k = 0; k < n_ranges; ++k) {
        const int64_t b0 = c->ss_off[(size_t)ranges[2 * k]], b1 = c->ss_off[(size_t)ranges[2 * k + 1]];
        if (b1 > b0) {
            if (!so.empty() && so.back() + ln.back() == b0) ln.back() += b1 - b0;
            else so.push_back(b0), dn.push_back(at), ln.push_back(b1 - b0);
        }
        at += b1 - b0;
    }
    const int e = sr_gather_launch(c->ls[LS_SRSEQ].as<uint8_t>(), dst.as<uint8_t>(), so.data(), dn.data(), ln.data(),
                                   (int64_t)so.size(), (void *)c->stream);
    if (e) return set_error(PR_ERR_HIP, "short-read gather: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

extern "C" int pr_srset_sample(pr_ctx *c, const int64_t *ranges, int n_ranges) {
    if (!c || n_ranges < 0 || (n_ranges && !ranges)) return set_error(PR_ERR_ARG, "null arg");
    std::vector<int64_t> off;
    int rc = gather_ranges(c, ranges, n_ranges, INT64_MAX, c->ls[LS_SRSAMP], off);
    if (rc) return rc;
    c->ss_samp_off.swap(off);
    return 0;
}

// ---------------------------------------------------------------------------
// pr_seed_gpu_map: the reads in chunks; per chunk pass 1, then for the reads it flagged pass 1b,
// pass 2 and the later passes, then the chunk's seeds compacted (planning: seed_plan.h)
namespace {

struct SeedMap {   // one map call
    pr_ctx *c;
    hipStream_t s;
    DevBuf *D;   // c->sd
    int n_sr;
    int qmax;   // the longest read
    SeedDev K;
    seedc::Caps small, caps;   // pass 1's slices (64 a wave), pass 2's (one a wave)
    int64_t waves;             // pass 1's
    int64_t lanes2;            // pass 2's resident waves
    int64_t chunk;             // reads per chunk
    int32_t budget;            // pass 1's hit budget per read (lazy table; 0: none)
    int64_t chain_waves, chain_waves2;   // seed_chain_kernel's resident waves, first and second geometry
    int64_t occ_words;         // the occurrence pool's words
    bool pool_full_said = false;
    // results so far: seeds per read, status, prefix of the seeds, flagged reads and their flags
    std::vector<int32_t> nout, st;
    std::vector<int64_t> pre;
    int64_t total = 0, bad = 0;
    int32_t bad_flags = 0;
};

// capacities, pass 1's waves, the output chunk: from the reads' lengths, the device and the tuning hooks
void map_plan(SeedMap &M, const pr_seed_opts *o, const int64_t *sr_off) {
    pr_ctx *c = M.c;
    int qmax = 1;
    for (int i = 0; i < M.n_sr; ++i) qmax = std::max<int>(qmax, (int)(sr_off[i + 1] - sr_off[i]));
    M.qmax = qmax;
    seedc::Caps &caps = M.caps, &small = M.small;
    caps = seedc::device_caps(qmax);
    caps.hi = c->seed_view.ksplit != nullptr;   // text beyond 2^32: positions carry bit 32
    caps.nopos = 1;   // the device tables keep the chaining's coordinates only (seed_core.h Caps)
    // pass 1: 64 reads per wave, small slices sized for the batch; pass 2 (flagged reads): the
    // large slices, one wave per read
    small = seedc::device_caps_small(std::min(qmax, caps.lmax));
    small.hi = caps.hi;
    small.nopos = 1;
    // the finish tasks' near-exact mapping: pass 1's occurrence tables lazily, a start's hits on
    // first use (seed_core.h materialize; the later passes build them eagerly, wave-parallel)
    small.lazy = seedc::lazy_occ(*o) ? 1 : 0;
    if (const char *sc = getenv("PRGPU_SEED_SMALL"))   // tuning hook: hits,iv,mems,seeds,chains
        sscanf(sc, "%d,%d,%d,%d,%d", &small.hits, &small.iv, &small.mems, &small.seeds, &small.chains);
    // pass 1's lanes run in lock-step, so a lazy-table read can be handed to the next pass once its
    // pool would pass a budget below the slice's capacity, instead of holding its 63 neighbours up
    // to the slice's last hit (seed_plan.h PASS1_LAZY_BUDGET: none by default, no measurable gain
    // at configs[1]).  PRGPU_SEED_BUDGET: tuning hook, 0: none
    M.budget = small.lazy ? seedp::PASS1_LAZY_BUDGET : 0;
    if (const char *bu = getenv("PRGPU_SEED_BUDGET")) M.budget = small.lazy ? std::max(0, atoi(bu)) : 0;
    SeedDev &K = M.K;
    K = SeedDev{};
    K.V = c->seed_view;
    K.O = *o;
    K.n_sr = M.n_sr;
    K.caps = small;
    K.stride = seedc::scratch_bytes(small);
    // the lane passes stop after the SMEMs and seed_chain_kernel chains their reads on chip;
    // PRGPU_SEED_CHAIN=lane: every read chained by its lane, as before (A/B and test hook)
    const char *chn = getenv("PRGPU_SEED_CHAIN");
    // A text beyond 2^32 positions (configs[3] ranks) keeps the lane chaining: there nearly every
    // read outgrows pass 1's hit table and is mapped by the by-wave passes, and the device memory
    // peaks within a few GB of the card later in the task, so no pool is taken for it
    K.chain = (chn && !strcmp(chn, "lane")) || caps.hi ? 0 : 1;
    M.chain_waves = (int64_t)c->n_cu * seed_chain_waves_per_cu(0);
    M.chain_waves2 = (int64_t)c->n_cu * seed_chain_waves_per_cu(1);
    const char *wpc = getenv("PRGPU_SEED_WAVES_PER_CU");   // tuning hook
    size_t fr = 0, tot = 0;
    (void)hipMemGetInfo(&fr, &tot);
    (void)hipGetLastError();
    // (PRGPU_SEED_BALANCE: seed_plan.h pass1_waves)
    const int per_cu = wpc ? atoi(wpc) : 16;
    // every resident wave's slices where the memory allows (seed_plan.h pass1_budget); a text
    // beyond 2^32 positions (configs[3] ranks) keeps scratch_budget: there the device memory peaks
    // within a few GB of the card later in the task (as index_build gives its sort buffers back)
    const int64_t full = caps.hi ? 0 : (int64_t)c->n_cu * per_cu * 64 * K.stride;
    M.waves = seedp::pass1_waves(M.n_sr, c->n_cu, per_cu, getenv("PRGPU_SEED_BALANCE") != nullptr,
                                 seedp::pass1_budget((int64_t)fr, (int64_t)M.D[SB_SCRATCH].cap, full), K.stride);
    K.n_lanes = M.waves;
    M.lanes2 = (int64_t)c->n_cu * seed_slots_per_cu(c->seed_view.walk_nw);
    // reads are mapped in chunks whose output slabs (caps.out seeds per read) fit a budget
    // (PRGPU_SEED_OUT_MB, default seed_plan.h out_budget: 8 to 16 GB; configs[1]'s 460k reads and
    // its finish task's 914k are one chunk); every chunk's seeds are compacted into the dense
    // list before the next chunk reuses the slab
    const char *ob = getenv("PRGPU_SEED_OUT_MB");
    M.chunk = seedp::out_chunk(ob ? std::max<int64_t>(1, atoll(ob)) << 20
                                  : seedp::out_budget((int64_t)fr, (int64_t)M.D[SB_OUT].cap),
                               (int64_t)caps.out * (int64_t)sizeof(pr_seed_task));
    M.occ_words = K.chain ? seedp::occ_pool_words(std::min<int64_t>(M.chunk, M.n_sr), small.lazy != 0, (int64_t)fr,
                                                  (int64_t)M.D[SB_OCC].cap)
                          : 0;
}

// the call's buffers, the reads on the device (in_sb_seq: SB_SEQ holds them already), K's pointers
int map_buffers(SeedMap &M, const pr_seed_opts *o, const uint8_t *sr_seq, bool in_sb_seq, const int64_t *sr_off) {
    pr_ctx *c = M.c;
    DevBuf *D = M.D;
    SeedDev &K = M.K;
    const int n_sr = M.n_sr;
    hipStream_t s = M.s;
    int rc;
    // mem_flt_chained_seeds' SW rows of pass 1 (reads >= 440 bp), lane-interleaved per wave
    K.dp = nullptr;
    if (seedc::seed_flt_min_score(*o, M.qmax) >= 0) {
        if ((rc = D[SB_DP].ensure((size_t)M.waves * 2 * 201 * 64 * sizeof(int16_t)))) return rc;
        K.dp = D[SB_DP].as<int16_t>();
    }
    const int64_t scratch = std::max<int64_t>(M.waves * 64 * K.stride, M.lanes2 * seedc::scratch_bytes(M.caps));
    const int64_t nb = n_sr ? sr_off[n_sr] : 0;
    const int64_t slot_bytes = (int64_t)M.caps.out * (int64_t)sizeof(pr_seed_task);
    c->seed_sr_bases = nb;
    if ((!in_sb_seq && (rc = upload(D[SB_SEQ], sr_seq, (size_t)nb, s))) || (rc = upload(D[SB_OFF], sr_off, (size_t)n_sr + 1, s)) ||
        (rc = D[SB_SCRATCH].ensure((size_t)scratch)) ||
        (rc = D[SB_OUT].ensure((size_t)(std::min<int64_t>(M.chunk, n_sr) * slot_bytes + 16))) ||
        (rc = D[SB_NOUT].ensure((size_t)n_sr * 4 + 16)) || (rc = D[SB_STATUS].ensure((size_t)n_sr * 4 + 16)) ||
        (rc = D[SB_NEXT].ensure(512)) || (rc = D[SB_PRE].ensure(((size_t)n_sr + 1) * 8)) ||
        (rc = D[SB_DENSE].ensure(sizeof(pr_seed_task))) || (M.occ_words && (rc = D[SB_OCC].ensure((size_t)M.occ_words * 8))))
        return rc;
    K.sr_seq = D[SB_SEQ].as<uint8_t>();
    K.sr_off = D[SB_OFF].as<int64_t>();
    K.out = D[SB_OUT].as<pr_seed_task>();
    K.n_out = D[SB_NOUT].as<int32_t>();
    K.status = D[SB_STATUS].as<int32_t>();
    K.next = D[SB_NEXT].as<int32_t>();
    K.prof = reinterpret_cast<unsigned long long *>(D[SB_NEXT].as<uint8_t>() + 64);
    // (next[1], next[2]: the chaining launches' counters; next[4..5]: the occurrence pool's cursor)
    K.occ = seedc::OccPool{D[SB_OCC].as<uint64_t>(), reinterpret_cast<unsigned long long *>(K.next + 4), M.occ_words};
    HIPCHK(hipMemsetAsync(K.next, 0, 512, s));
    return 0;
}

// pass 1 over the chunk [r0, r1): 64 reads per wave, lane per read -> the reads it flagged and
// what they asked for
int pass1(SeedMap &M, int64_t r0, int64_t r1, std::vector<int32_t> &redo, seedp::Flagged &f) {
    DevBuf *D = M.D;
    SeedDev &K = M.K;
    hipStream_t s = M.s;
    int rc;
    K.caps = M.small;
    K.caps.budget = M.budget;   // (pass 1 only: pass 1b's slices are sized for what the flagged reads need)
    K.stride = seedc::scratch_bytes(M.small);
    K.n_lanes = M.waves;
    K.batch = 64;
    K.scratch = D[SB_SCRATCH].as<uint8_t>();
    K.rlist = nullptr;
    K.n_list = 0;
    K.out0 = r0;
    K.n_sr = r1;
    int32_t start = (int32_t)r0;
    // PRGPU_SEED_LPT=1: the chunk's reads costliest first (seed_order_launch).  Measured at
    // configs[1]: 312.5 against 306.2 ms in read order (the batches' lane phase grew more than
    // the tail shrank), so read order stays the default
    const char *lpt = getenv("PRGPU_SEED_LPT");
    if (lpt && lpt[0] == '1') {
        int32_t *order = nullptr;
        if ((rc = D[SB_ORDER].ensure(seed_order_bytes(r1 - r0)))) return rc;
        int eo = seed_order_launch(K, r0, r1 - r0, D[SB_ORDER].p, &order, (void *)s);
        if (eo) return set_error(PR_ERR_HIP, "seed order: %s", hipGetErrorString((hipError_t)eo));
        K.rlist = order;
        K.n_list = r1 - r0;
        start = 0;
    }
    HIPCHK(hipMemcpyAsync(K.next, &start, 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(K.next + 1, 0, 28, s));
    int e = seed_batch_launch(K, (void *)s);
    if (e) return set_error(PR_ERR_HIP, "seed kernel: %s", hipGetErrorString((hipError_t)e));
    if ((e = seed_chain_launch(K, M.chain_waves, M.chain_waves2, (void *)s)))
        return set_error(PR_ERR_HIP, "seed chaining kernel: %s", hipGetErrorString((hipError_t)e));
    if (r0 == 0) HIPCHK(hipEventRecord(M.c->ev[10], s));
    std::vector<int32_t> st1((size_t)(r1 - r0)), no1((size_t)(r1 - r0));
    if ((rc = download(st1.data(), D[SB_STATUS], (size_t)(r1 - r0), s, (size_t)r0)) ||
        (rc = download(no1.data(), D[SB_NOUT], (size_t)(r1 - r0), s, (size_t)r0)))
        return rc;
    unsigned long long asked = 0;   // the pool words pass 1's reads asked for
    if (K.chain) HIPCHK(hipMemcpyAsync(&asked, K.occ.cursor, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    // a full pool flags the reads beyond it SC_OVER_SEEDS like a true seed overflow: they are
    // mapped by the later passes, exact but slower, so it is said once per map
    if ((int64_t)asked > K.occ.cap && !M.pool_full_said) {
        M.pool_full_said = true;
        std::fprintf(stderr, "[seed] occurrence pool full: %lld reads asked for %llu words of %lld; the reads beyond it take the later passes\n",
                     (long long)(r1 - r0), asked, (long long)K.occ.cap);
    }
    for (int64_t i = r0; i < r1; ++i)
        if (st1[(size_t)(i - r0)]) {
            redo.push_back((int32_t)i);
            f.add(st1[(size_t)(i - r0)], no1[(size_t)(i - r0)]);
        }
    return 0;
}

// One more pass over `reads` of the chunk: the list to SB_PRE, the dequeue counter zeroed, the
// kernel (by_wave: one wave per read, seed_launch; else 64 reads per wave, seed_batch_launch)
// over `lanes` slices of `caps` (by lane: lanes waves of `batch` slices each)
int launch_pass(SeedMap &M, const char *name, bool by_wave, const seedc::Caps &caps, int64_t lanes,
                const std::vector<int32_t> &reads, int batch = 64) {
    SeedDev &K = M.K;
    K.caps = caps;
    K.stride = seedc::scratch_bytes(caps);
    K.n_lanes = lanes;
    K.batch = batch;
    K.scratch = M.D[SB_SCRATCH].as<uint8_t>();
    K.rlist = M.D[SB_PRE].as<int32_t>();
    K.n_list = (int64_t)reads.size();
    HIPCHK(hipMemcpyAsync(M.D[SB_PRE].p, reads.data(), reads.size() * 4, hipMemcpyHostToDevice, M.s));
    HIPCHK(hipMemsetAsync(K.next, 0, 32, M.s));
    int e = by_wave ? seed_launch(K, (void *)M.s) : seed_batch_launch(K, (void *)M.s);
    if (!e && !by_wave) e = seed_chain_launch(K, M.chain_waves, M.chain_waves2, (void *)M.s);
    if (e) return set_error(PR_ERR_HIP, "seed kernel (%s): %s", name, hipGetErrorString((hipError_t)e));
    return 0;
}

// the reads of `reads` (of the chunk [r0, r1)) that the last pass left flagged, and their flags or-ed
int still_flagged(SeedMap &M, int64_t r0, int64_t r1, const std::vector<int32_t> &reads, std::vector<int32_t> &left,
                  int32_t &flags) {
    std::vector<int32_t> st((size_t)(r1 - r0));
    int rc = download(st.data(), M.D[SB_STATUS], (size_t)(r1 - r0), M.s, (size_t)r0);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(M.s));
    left.clear();
    flags = 0;
    for (int32_t i : reads)
        if (st[(size_t)(i - r0)]) left.push_back(i), flags |= st[(size_t)(i - r0)];
    return 0;
}

// Pass 1b (seed_plan.h): many flagged reads again with pass 1's slices grown, lane per read, or
// one wave each; redo becomes the reads it left.  After the by-wave pass, p2caps are its slices
// and pass 2 is skipped: its leftovers overflowed them, the later passes grow from them
int pass1b(SeedMap &M, int64_t r0, int64_t r1, const seedp::Flagged &f, std::vector<int32_t> &redo, seedc::Caps &p2caps,
           bool &p2_ran) {
    if (!seedp::pass1b_wanted(f)) return 0;
    const seedp::Pass1bCaps p = seedp::pass1b_caps(M.small, M.caps, f);
    DevBuf &scr = M.D[SB_SCRATCH];
    int rc;
    size_t fr = 0, tot = 0;
    (void)hipMemGetInfo(&fr, &tot);
    (void)hipGetLastError();
    if (const int64_t want = seedp::pass1b_scratch_want(M.waves, f.n, p.sb, (int64_t)fr, (int64_t)scr.cap)) {
        HIPCHK(hipStreamSynchronize(M.s));
        if ((rc = scr.ensure((size_t)want))) return rc;
    }
    const char *p1b = getenv("PRGPU_SEED_1B");   // wave / lane forces either
    const seedp::Pass1bForce force =
        !p1b ? seedp::P1B_AUTO : !strcmp(p1b, "wave") ? seedp::P1B_FORCE_WAVE : seedp::P1B_FORCE_LANE;
    const seedp::Pass1bRun r =
        seedp::pass1b_run(p, f, M.small.hits, force, (int64_t)scr.cap, M.waves, M.lanes2, M.c->n_cu);
    if (r.mode == seedp::P1B_SKIP) return 0;
    const bool by_wave = r.mode == seedp::P1B_WAVE;
    // lane per read with the lazy table: the flagged reads over all of pass 1's waves (the eager
    // kernel keeps 64 a wave).  PRGPU_SEED_1B_BATCH: tuning hook, the reads a wave takes at a time
    seedp::Pass1bBatch b{64, r.wb};
    if (!by_wave && p.cb.lazy) {
        const char *bb = getenv("PRGPU_SEED_1B_BATCH");
        b = seedp::pass1b_batch(r, f.n, M.waves, (int64_t)scr.cap, p.sb, bb ? atoi(bb) : 0);
    }
    if ((rc = launch_pass(M, by_wave ? "pass 1b, waves" : "pass 1b", by_wave, by_wave ? p.cw : p.cb, by_wave ? r.ww : b.waves,
                          redo, b.batch)))
        return rc;
    M.c->seed_pass_reads[by_wave ? 1 : 0] += (int64_t)redo.size();
    if (by_wave) p2caps = p.cw, p2_ran = true;
    std::vector<int32_t> left;
    int32_t fl;
    if ((rc = still_flagged(M, r0, r1, redo, left, fl))) return rc;
    redo.swap(left);
    M.K.rlist = nullptr;
    M.K.n_list = 0;
    return 0;
}

// Pass 2 over the flagged reads (the large slices, one wave per read; not after a by-wave pass
// 1b), then the later passes: the reads that outgrew the large slices too (e.g. the finish
// task's near-exact reads at 30-60x long-read coverage: every 12-mer hits every copy, > 8192
// hits per read) again, with the arrays that overflowed grown from cg, up to 4 times
int pass2_and_later(SeedMap &M, int64_t r0, int64_t r1, std::vector<int32_t> &redo, seedc::Caps cg, bool p2_ran) {
    if (redo.empty()) return 0;
    int rc;
    if (!p2_ran) {
        if ((rc = launch_pass(M, "pass 2", true, M.caps, std::min<int64_t>(M.lanes2, (int64_t)redo.size()), redo))) return rc;
        HIPCHK(hipStreamSynchronize(M.s));
        M.c->seed_pass_reads[2] += (int64_t)redo.size();
    }
    for (int pass = 3; pass <= 6; ++pass) {
        std::vector<int32_t> again;
        int32_t fl;
        if ((rc = still_flagged(M, r0, r1, redo, again, fl))) return rc;
        if (again.empty() || (fl & (seedc::SC_OVER_LEN | seedc::SC_OVER_OUT))) break;
        cg = seedc::grow_caps(cg, fl, 4);
        redo.swap(again);
        const int64_t lanes = std::min<int64_t>(M.lanes2, (int64_t)redo.size());
        if ((rc = M.D[SB_SCRATCH].ensure((size_t)(lanes * seedc::scratch_bytes(cg))))) return rc;
        char name[16];
        snprintf(name, sizeof name, "pass %d", pass);
        if ((rc = launch_pass(M, name, true, cg, lanes, redo))) return rc;
        HIPCHK(hipStreamSynchronize(M.s));
        M.c->seed_pass_reads[3] += (int64_t)redo.size();
    }
    return 0;
}

// the chunk's seeds: compacted on the device (read order) behind the earlier chunks'
int compact_chunk(SeedMap &M, int64_t r0, int64_t r1) {
    DevBuf *D = M.D;
    hipStream_t s = M.s;
    int rc;
    if ((rc = download(M.nout.data() + r0, D[SB_NOUT], (size_t)(r1 - r0), s, (size_t)r0)) ||
        (rc = download(M.st.data() + r0, D[SB_STATUS], (size_t)(r1 - r0), s, (size_t)r0)))
        return rc;
    HIPCHK(hipStreamSynchronize(s));
    const int64_t t0 = M.total;
    for (int64_t i = r0; i < r1; ++i) {
        if (M.nout[(size_t)i] < 0 || M.nout[(size_t)i] > M.caps.out) return set_error(PR_ERR_HIP, "seed kernel: bad task count");
        M.total += M.nout[(size_t)i];
        M.pre[(size_t)i + 1] = M.total;
        M.bad += M.st[(size_t)i] != 0;
        M.bad_flags |= M.st[(size_t)i];
    }
    if ((rc = upload(D[SB_PRE], M.pre.data() + r0, (size_t)(r1 - r0 + 1), s)) ||
        (rc = D[SB_DENSE].grow_keep(sizeof(pr_seed_task) * (size_t)(M.total > 0 ? M.total : 1),
                                    sizeof(pr_seed_task) * (size_t)t0, s)))
        return rc;
    const int e = seed_compact_launch(D[SB_OUT].as<pr_seed_task>(), D[SB_NOUT].as<int32_t>() + r0, D[SB_PRE].as<int64_t>(),
                                      r1 - r0, M.caps.out, D[SB_DENSE].as<pr_seed_task>(), (void *)s);
    if (e) return set_error(PR_ERR_HIP, "seed compaction: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

// The map of both entry points.  sr_seq: the reads' bases on the host, or null with in_sb_seq:
// SB_SEQ already holds them (pr_seed_gpu_map_sampled gathered them on the device).
int seed_map(pr_ctx *c, const pr_seed_opts *o, const uint8_t *sr_seq, bool in_sb_seq, const int64_t *sr_off, int n_sr,
             pr_seed_tasks *out, int32_t *status) {
    if (!o || n_sr < 0 || (n_sr && ((!sr_seq && !in_sb_seq) || !sr_off))) return set_error(PR_ERR_ARG, "null arg");
    c->seed_pre.clear();
    if (!c->seed_loaded) return set_error(PR_ERR_ARG, "no seed index on the device (pr_seed_gpu_upload)");
    if (o->min_seed_len < seedc::KI) return set_error(PR_ERR_UNSUPPORTED, "min seed length below the 12-mer index");
    if (o->max_occ <= 0 || o->w < 0) return set_error(PR_ERR_ARG, "bad seeding options");
    if (out) out->n = 0, out->t = nullptr;   // (null: the seeds stay in HBM for pr_iter_upload_gpu_seeds)
    if (n_sr && sr_off[0] != 0) return set_error(PR_ERR_ARG, "sr_off must start at 0");
    for (int i = 0; i < n_sr; ++i)
        if (sr_off[i + 1] < sr_off[i]) return set_error(PR_ERR_ARG, "sr_off not monotone");
    HIPCHK(hipSetDevice(c->device));
    SeedMap M;
    M.c = c;
    M.s = c->stream;
    M.D = c->sd;
    M.n_sr = n_sr;
    hipStream_t s = M.s;
    int rc;
    map_plan(M, o, sr_off);
    if ((rc = map_buffers(M, o, sr_seq, in_sb_seq, sr_off))) return rc;
    HIPCHK(hipEventRecord(c->ev[8], s));
    c->seed_pass2 = 0;
    std::fill(c->seed_pass_reads, c->seed_pass_reads + 4, 0);
    M.nout.resize((size_t)n_sr);
    M.st.resize((size_t)n_sr);
    M.pre.assign((size_t)n_sr + 1, 0);
    for (int64_t r0 = 0; r0 < n_sr; r0 += M.chunk) {
        const int64_t r1 = std::min<int64_t>(n_sr, r0 + M.chunk);
        std::vector<int32_t> redo;
        seedp::Flagged f;
        seedc::Caps p2caps = M.caps;   // the slices the later passes grow from
        bool p2_ran = false;
        if ((rc = pass1(M, r0, r1, redo, f)) || (rc = pass1b(M, r0, r1, f, redo, p2caps, p2_ran))) return rc;
        c->seed_pass2 += (int64_t)redo.size();
        if ((rc = pass2_and_later(M, r0, r1, redo, p2caps, p2_ran)) || (rc = compact_chunk(M, r0, r1))) return rc;
    }
    HIPCHK(hipEventRecord(c->ev[9], s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0.f;
    if (n_sr && hipEventElapsedTime(&ms, c->ev[8], c->ev[9]) == hipSuccess) c->ms_seed = ms;
    c->ms_seed_pass2 = 0.f;   // (the passes after the first chunk's pass 1; one chunk at configs[1])
    if (n_sr && hipEventElapsedTime(&ms, c->ev[10], c->ev[9]) == hipSuccess) c->ms_seed_pass2 = ms;
    // an incomplete seed set (flagged reads have no seeds) is never handed to
    // pr_iter_upload_gpu_seeds: it refuses when seed_pre does not match the reads
    if (M.bad) c->seed_pre.clear();
    else c->seed_pre = M.pre;
    if (out) {
        out->t = (pr_seed_task *)std::malloc(sizeof(pr_seed_task) * (size_t)(M.total > 0 ? M.total : 1));
        if (!out->t) return set_error(PR_ERR_ARG, "out of host memory");
        if (M.total && (rc = download(out->t, M.D[SB_DENSE], (size_t)M.total, s))) return rc;
    }
    HIPCHK(hipStreamSynchronize(s));
    if (out) out->n = M.total;
    if (status) std::memcpy(status, M.st.data(), (size_t)n_sr * 4);
    if (M.bad)
        return set_error(PR_ERR_CAPACITY, "%lld reads outgrew the seeding scratch (status flags, or: 0x%x)", (long long)M.bad,
                         M.bad_flags);
    return 0;
}

}   // namespace

extern "C" int pr_seed_gpu_map(pr_ctx *c, const pr_seed_opts *o, const uint8_t *sr_seq, const int64_t *sr_off, int n_sr,
                               pr_seed_tasks *out, int32_t *status) {
    if (!c) return set_error(PR_ERR_ARG, "null arg");
    return seed_map(c, o, sr_seq, false, sr_off, n_sr, out, status);
}

extern "C" int pr_seed_gpu_map_sampled(pr_ctx *c, const pr_seed_opts *o, const int64_t *ranges, int n_ranges,
                                       int32_t *status) {
    if (!c || !o || n_ranges < 0 || (n_ranges && !ranges)) return set_error(PR_ERR_ARG, "null arg");
    std::vector<int64_t> off;
    int rc = gather_ranges(c, ranges, n_ranges, INT32_MAX, c->sd[SB_SEQ], off);
    if (rc) return rc;
    return seed_map(c, o, nullptr, true, off.data(), (int)off.size() - 1, nullptr, status);
}


extern "C" int pr_seed_gpu_seed_count(pr_ctx *c, int64_t *n) {
    if (!c || !n) return set_error(PR_ERR_ARG, "null arg");
    *n = c->seed_pre.empty() ? 0 : c->seed_pre.back();
    return 0;
}

extern "C" int pr_seed_gpu_seeds(pr_ctx *c, pr_seed_tasks *out) {
    if (!c || !out) return set_error(PR_ERR_ARG, "null arg");
    out->n = 0, out->t = nullptr;
    if (c->seed_pre.empty()) return set_error(PR_ERR_ARG, "no complete seed set on the device");
    HIPCHK(hipSetDevice(c->device));
    const int64_t total = c->seed_pre.back();
    out->t = (pr_seed_task *)std::malloc(sizeof(pr_seed_task) * (size_t)(total > 0 ? total : 1));
    if (!out->t) return set_error(PR_ERR_ARG, "out of host memory");
    int rc;
    if (total && (rc = download(out->t, c->sd[SB_DENSE], (size_t)total, c->stream))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    out->n = total;
    return 0;
}

extern "C" int pr_seed_gpu_pass2_reads(pr_ctx *c, int64_t *n) {
    if (!c || !n) return set_error(PR_ERR_ARG, "null arg");
    *n = c->seed_pass2;
    return 0;
}

extern "C" int pr_seed_gpu_pass_reads(pr_ctx *c, int64_t *n4) {
    if (!c || !n4) return set_error(PR_ERR_ARG, "null arg");
    std::copy(c->seed_pass_reads, c->seed_pass_reads + 4, n4);
    return 0;
}

extern "C" int pr_seed_gpu_last_ms(pr_ctx *c, double *ms) {
    if (!c || !ms) return set_error(PR_ERR_ARG, "null arg");
    *ms = c->ms_seed;
    return 0;
}

extern "C" int pr_seed_gpu_pass2_ms(pr_ctx *c, double *ms) {
    if (!c || !ms) return set_error(PR_ERR_ARG, "null arg");
    *ms = c->ms_seed_pass2;   // from pass 1's end to pass 2's (its status download included)
    return 0;
}

extern "C" int pr_seed_gpu_phase_ticks(pr_ctx *c, uint64_t *ticks4) {
    if (!c || !ticks4) return set_error(PR_ERR_ARG, "null arg");
    if (!c->sd[SB_NEXT].p) return set_error(PR_ERR_ARG, "no pr_seed_gpu_map launch yet");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(ticks4, c->sd[SB_NEXT].as<uint8_t>() + 64, 32, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pr_seed_gpu_lane_ticks(pr_ctx *c, uint64_t *ticks6) {
    if (!c || !ticks6) return set_error(PR_ERR_ARG, "null arg");
    if (!c->sd[SB_NEXT].p) return set_error(PR_ERR_ARG, "no pr_seed_gpu_map launch yet");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(ticks6, c->sd[SB_NEXT].as<uint8_t>() + 64 + 4 * 8, 48, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pr_seed_gpu_pass2_ticks(pr_ctx *c, uint64_t *t7) {
    if (!c || !t7) return set_error(PR_ERR_ARG, "null arg");
    if (!c->sd[SB_NEXT].p) return set_error(PR_ERR_ARG, "no pr_seed_gpu_map launch yet");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(t7, c->sd[SB_NEXT].as<uint8_t>() + 64 + 13 * 8, 56, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pr_seed_gpu_chain_ticks(pr_ctx *c, uint64_t *ticks7) {
    if (!c || !ticks7) return set_error(PR_ERR_ARG, "null arg");
    if (!c->sd[SB_NEXT].p) return set_error(PR_ERR_ARG, "no pr_seed_gpu_map launch yet");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(ticks7, c->sd[SB_NEXT].as<uint8_t>() + 64 + 24 * 8, 56, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pr_seed_gpu_occ_ticks(pr_ctx *c, uint64_t *ticks3) {
    if (!c || !ticks3) return set_error(PR_ERR_ARG, "null arg");
    if (!c->sd[SB_NEXT].p) return set_error(PR_ERR_ARG, "no pr_seed_gpu_map launch yet");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(ticks3, c->sd[SB_NEXT].as<uint8_t>() + 64 + 10 * 8, 24, hipMemcpyDeviceToHost));
    return 0;
}

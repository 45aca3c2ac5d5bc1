// One iteration on the device (include/prgpu.h pr_iter_*): SW -> hand-off -> consensus, the
// -b/-l filter, downloads, the hand-off's statistics and timing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "pipe_dev.h"

// the hand-off takes up to handp::MAX_ALNS alignments per long read (what: "tasks" / "alignments")
static int handoff_refused(const handp::Plan &ho, const char *what) {
    if (ho.refused_lr < 0) return 0;
    return set_error(PR_ERR_CAPACITY, "long read %d has %lld %s: more than 2^20 (the consensus kernel's alignment index)",
                     ho.refused_lr, (long long)ho.refused_count, what);
}

// one iteration on the device: SW -> assemble -> consensus (pr_iter_*)
// dev_*: device sources in place of the batch's host pools (the resident long-read set and the
// seeding's copies: pr_iter_upload_lrset)
int iter_upload(pr_ctx *c, const pr_iter_batch *b, bool gpu_seeds, const uint8_t *dev_sr, const uint8_t *dev_lr,
                const uint8_t *dev_ref, const uint8_t *dev_qual) {
    if (!c || !b) return set_error(PR_ERR_ARG, "null arg");
    pr_sw_batch sbv = b->sw;
    if (gpu_seeds) {   // the seeds of the last pr_seed_gpu_map, still in HBM
        if (c->seed_pre.size() != (size_t)sbv.n_sr + 1)
            return set_error(PR_ERR_ARG, "no device seeds for these short reads (pr_seed_gpu_map with out = NULL first)");
        sbv.n_task = c->seed_pre.back();
        sbv.t_sr = sbv.t_lr = sbv.t_qbeg = sbv.t_rbeg = sbv.t_slen = sbv.t_chain = nullptr;
        sbv.t_strand = nullptr;
    }
    const pr_sw_batch &sb = sbv;
    const int n = sb.n_lr;
    const bool bwa = sb.t_chain != nullptr || gpu_seeds;   // seeds in, alignments grouped by long read on the device
    if (!bwa && (!b->task_lr_off || b->task_lr_off[0] != 0 || b->task_lr_off[n] != sb.n_task))
        return set_error(PR_ERR_ARG, "task_lr_off must partition the tasks");
    // the hand-off's sort plan from the tasks per long read (bwa mode: from the alignment counts, at launch)
    std::vector<int64_t> per_lr(bwa ? 0 : (size_t)n);
    for (int i = 0; i < n && !bwa; ++i) {
        if (b->task_lr_off[i + 1] < b->task_lr_off[i]) return set_error(PR_ERR_ARG, "task_lr_off not monotone");
        per_lr[(size_t)i] = b->task_lr_off[i + 1] - b->task_lr_off[i];
    }
    handp::Plan ho = handp::plan(per_lr.data(), (int64_t)per_lr.size());
    int rc = handoff_refused(ho, "tasks");
    if (rc) return rc;
    for (int i = 0; i < n && !bwa; ++i)
        for (int64_t t = b->task_lr_off[i]; t < b->task_lr_off[i + 1]; ++t)
            if (sb.t_lr[t] != i) return set_error(PR_ERR_ARG, "tasks must be grouped by long read");
    const int64_t maxt = ho.max_count > 1 ? ho.max_count : 1;
    rc = gpu_seeds ? sw_upload_device_seeds(c, &sb, c->sd[SB_DENSE].as<pr_seed_task>(), c->seed_pre.data(), dev_sr, dev_lr)
                   : pr_sw_upload(c, &sb);
    if (rc) return rc;
    c->x_ready = c->x_pass = false;   // a new SW batch: no exchange of it yet
    HIPCHK(hipSetDevice(c->device));
    c->cns_launched = false;
    c->iter_masked = false;
    c->own = false;
    ++c->iter_gen;
    for (auto &x : c->eb) x.release();   // a BAM export's pools belong to the batch they were made for
    hipStream_t s = c->stream;
    c->n_lr = n;
    c->n_aln = sb.n_task;
    c->total_cols = sb.lr_off[n];
    c->has_ref = true;
    c->pipe_ref_ascii = b->ref_seq != nullptr || dev_ref != nullptr;
    c->has_qual = b->lr_qual != nullptr || dev_qual != nullptr;
    c->has_ign = false;
    c->lr_off_host.assign(sb.lr_off, sb.lr_off + n + 1);
    c->out_off.assign(n + 1, 0);
    c->chim_off.assign(n + 1, 0);
    cnsp::pipe_caps(sb.lr_off, n, c->out_off.data(), c->chim_off.data());
    c->seq_cap = c->out_off[n];
    c->chim_cap = c->chim_off[n];
    c->alg_bytes = 0;
    c->k_need = maxt;
    c->pipe_sort_cap = ho.sort_cap;
    c->ho = std::move(ho);
    c->ho_done = false;
    DevBuf *B = c->cb;
    const size_t n1 = (size_t)n + 1;
    if ((rc = upload(B[CB_LR_OFF], sb.lr_off, n1, s))) return rc;
    if (b->lr_qual && (rc = upload(B[CB_REF_QUAL], b->lr_qual, (size_t)sb.lr_off[n], s))) return rc;
    if (b->ref_seq && (rc = upload(B[CB_REF_SEQ], b->ref_seq, (size_t)sb.lr_off[n], s))) return rc;
    for (int k = 0; k < 2; ++k) {   // device sources of the reference and its qualities
        const uint8_t *src = k ? dev_qual : dev_ref;
        if (!src) continue;
        DevBuf &dst = B[k ? CB_REF_QUAL : CB_REF_SEQ];
        if ((rc = dst.ensure((size_t)sb.lr_off[n] + 1))) return rc;
        if (sb.lr_off[n]) HIPCHK(hipMemcpyAsync(dst.p, src, (size_t)sb.lr_off[n], hipMemcpyDeviceToDevice, s));
    }
    if (!bwa && (rc = upload(c->pb[PB_TASK_OFF], b->task_lr_off, n1, s))) return rc;
    if ((rc = c->pb[PB_CNT].ensure(n1 * 4)) || (rc = c->pb[PB_ERR].ensure(n1 * 4))) return rc;
    if ((rc = cns_ensure(c, cnsp::ALL))) return rc;
    if ((rc = upload(B[CB_OUT_OFF], c->out_off.data(), n1, s))) return rc;
    if ((rc = upload(B[CB_CHIM_OFF], c->chim_off.data(), n1, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    c->cns_loaded = true;
    c->pipe = true;
    return 0;
}

extern "C" int pr_iter_upload(pr_ctx *c, const pr_iter_batch *b) { return iter_upload(c, b, false); }
extern "C" int pr_iter_upload_gpu_seeds(pr_ctx *c, const pr_iter_batch *b) { return iter_upload(c, b, true); }

// the -b/-l filter's buffers for n_task tasks, its bins per long read against the kernel's LDS
// layout (lr_off: the n_lr long reads' offsets on the host) and the filter fields of P
static int binfilter_setup(pr_ctx *c, PipeDev &P, int64_t n_task, const int64_t *lr_off, int n_lr, int32_t bin_size,
                           int *max_bins_out) {
    int64_t lmax = 0;
    for (int i = 0; i < n_lr; ++i) lmax = std::max(lmax, lr_off[i + 1] - lr_off[i]);
    const int64_t max_bins = (lmax + 1024) / bin_size + 2;
    if ((2 * max_bins + 256) * 4 > 160 * 1024)
        return set_error(PR_ERR_CAPACITY, "-b/-l filter: %lld bins per long read exceed the LDS layout", (long long)max_bins);
    const size_t nt1 = (size_t)n_task + 1;
    DevBuf *F = c->pb;
    int rc;
    if ((rc = F[PB_F_KEEP].ensure(nt1)) || (rc = F[PB_F_SORTED].ensure(nt1 * 4)) || (rc = F[PB_F_BIN].ensure(nt1 * 4)) ||
        (rc = F[PB_F_NC].ensure(nt1 * 8)) || (rc = F[PB_F_LEN].ensure(nt1 * 4)) || (rc = F[PB_F_LST].ensure(nt1 * 8)) ||
        (rc = F[PB_F_LSTI].ensure(nt1 * 4)))
        return rc;
    P.keep = F[PB_F_KEEP].as<uint8_t>();
    P.fsorted = F[PB_F_SORTED].as<int32_t>();
    P.fbin = F[PB_F_BIN].as<int32_t>();
    P.fnc = F[PB_F_NC].as<double>();
    P.flen = F[PB_F_LEN].as<int32_t>();
    P.flst = F[PB_F_LST].as<double>();
    P.flsti = F[PB_F_LSTI].as<int32_t>();
    *max_bins_out = (int)max_bins;
    return 0;
}

extern "C" int pr_iter_launch(pr_ctx *c, const pr_sw_opts *o, const pr_cns_params *p) {
    if (!c || !o || !p) return set_error(PR_ERR_ARG, "null arg");
    if (!c->pipe) return set_error(PR_ERR_ARG, "no resident iteration batch (pr_iter_upload first)");
    ++c->iter_gen;
    int rc;
    SwPtrs sp;
    if (c->own) {   // owned batch: the SW and the exchange ran before (ev[0]: the exchange's start)
        HIPCHK(hipSetDevice(c->device));
        if ((rc = own_group(c, &sp))) return rc;
    } else {
        if ((rc = pr_sw_launch(c, o))) return rc;   // records ev[2], ev[3], ev[0]
        if ((rc = sw_get_pipe_ptrs(c, &sp, true))) return rc;
    }
    if (sp.task_off) {   // bwa mode: the reported alignments grouped by long read on the device
        // (the counts before the -b/-l filter: upper bounds of what the hand-off sorts)
        c->ho = handp::plan(sp.cnt_host, (int64_t)c->n_lr);
        if ((rc = handoff_refused(c->ho, "alignments"))) return rc;
        c->k_need = c->ho.max_count > 1 ? c->ho.max_count : 1;
        c->pipe_sort_cap = c->ho.sort_cap;
    }
    DevBuf *B = c->cb;
    PipeDev P;
    P.n_lr = c->n_lr;
    P.sort_cap = c->pipe_sort_cap;
    P.cig_at = sp.cig_at;
    P.task_off = sp.task_off ? sp.task_off : c->pb[PB_TASK_OFF].as<int64_t>();
    P.t_sr = sp.t_sr;
    P.strand = sp.strand;
    P.pass = sp.pass;
    P.status = sp.status;
    P.pos = sp.pos;
    P.score = sp.score;
    P.ncig = sp.ncig;
    P.sr_off = sp.sr_off;
    P.cnt = c->pb[PB_CNT].as<int32_t>();
    P.aln_off = B[CB_ALN_OFF].as<int64_t>();
    P.err = c->pb[PB_ERR].as<int32_t>();
    P.a_pos = B[CB_POS].as<int32_t>();
    P.a_score = B[CB_SCORE].as<double>();
    P.a_flags = B[CB_AFLAGS].as<uint8_t>();
    P.a_seq_off = B[CB_SEQ_OFF].as<int64_t>();
    P.a_lseq = B[CB_LSEQ].as<int32_t>();
    P.a_cig_off = B[CB_CIG_OFF].as<int64_t>();
    P.a_ncig = B[CB_NCIG].as<int32_t>();
    P.lr_off = B[CB_LR_OFF].as<int64_t>();
    P.cig = sp.cig;
    P.keep = nullptr;
    if (c->n_lr == 0) return 0;
    if ((rc = c->pb[PB_ORDER].ensure(((size_t)c->n_aln + 1) * 4))) return rc;
    P.a_task = c->pb[PB_ORDER].as<int32_t>();
    PipeBig G;
    std::memset(&G, 0, sizeof G);
    const handp::Plan &ho = c->ho;
    if (ho.n_big) {   // reads beyond the LDS sort: their list and the key buffers of the HBM path
        if ((rc = upload(c->pb[PB_BIG_LR], ho.big_lr.data(), ho.big_lr.size(), c->stream)) ||
            (rc = upload(c->pb[PB_BIG_OFF], ho.big_off.data(), ho.big_off.size(), c->stream)) ||
            (rc = c->pb[PB_KEY0].ensure((size_t)ho.scratch_bytes / 2)) || (rc = c->pb[PB_KEY1].ensure((size_t)ho.scratch_bytes / 2)))
            return rc;
        G.n_big = (int)ho.n_big;
        G.passes = ho.passes;
        G.max_runs = ho.max_runs;
        G.max_big = ho.max_big;
        G.lr = c->pb[PB_BIG_LR].as<int32_t>();
        G.off = c->pb[PB_BIG_OFF].as<int64_t>();
        G.k0 = c->pb[PB_KEY0].as<unsigned long long>();
        G.k1 = c->pb[PB_KEY1].as<unsigned long long>();
    }
    const int grid = c->n_lr < c->n_cu * 4 ? c->n_lr : c->n_cu * 4;
    HIPCHK(hipMemsetAsync(c->pb[PB_ERR].p, 0, (size_t)c->n_lr * 4, c->stream));
    if (o->bin_size > 0 && o->bin_length > 0) {   // bwa-proovread -b/-l (bin/proovread:1302-1313)
        int max_bins = 0;
        if ((rc = binfilter_setup(c, P, sp.n_task, c->lr_off_host.data(), c->n_lr, o->bin_size, &max_bins))) return rc;
        // (latency-bound, a few KB of LDS per workgroup: 8 workgroups per CU)
        const int grid_f = c->n_lr < c->n_cu * 8 ? c->n_lr : c->n_cu * 8;
        int e = pipe_binfilter_launch(P, o->bin_size, o->bin_length, max_bins, grid_f, (void *)c->stream);
        if (e) return set_error(PR_ERR_HIP, "-b/-l filter kernel: %s", hipGetErrorString((hipError_t)e));
    }
    c->cns_gathered = false;   // the hand-off writes offsets into the SW / short-read pools
    int e = pipe_launch(P, grid, (void *)c->stream, c->pipe_sort_cap * 8, ho.n_big ? &G : nullptr);
    if (e) return set_error(PR_ERR_HIP, "pipe kernels: %s", hipGetErrorString((hipError_t)e));
    c->ho_done = true;
    c->ho_sw_gen = c->sw.gen;
    return pr_cns_launch(c, p);
}

// bwa-proovread -b/-l on the last bwa-mode SW launch alone (the `mem` drop-in): the hand-off's
// grouping by long read and pipe_binfilter_kernel, as pr_iter_launch runs them
extern "C" int pr_sw_binfilter(pr_ctx *c, int32_t bin_size, double bin_length, uint8_t *keep) {
    if (!c || !keep) return set_error(PR_ERR_ARG, "null arg");
    if (bin_size <= 0 || !(bin_length > 0)) return set_error(PR_ERR_ARG, "-b / -l must be positive");
    HIPCHK(hipSetDevice(c->device));
    SwPtrs sp;
    int rc;
    if ((rc = sw_get_pipe_ptrs(c, &sp, true))) return rc;
    if (!sp.task_off) return set_error(PR_ERR_ARG, "pr_sw_binfilter: bwa mode only");
    const int n_lr = sp.n_lr;
    if (n_lr == 0 || sp.n_task == 0) return 0;
    std::vector<int64_t> lo((size_t)n_lr + 1);
    HIPCHK(hipMemcpyAsync(lo.data(), sp.lr_off, ((size_t)n_lr + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    PipeDev P;
    std::memset(&P, 0, sizeof P);
    P.n_lr = n_lr;
    P.task_off = sp.task_off;
    P.t_sr = sp.t_sr;
    P.strand = sp.strand;
    P.pass = sp.pass;
    P.status = sp.status;
    P.pos = sp.pos;
    P.score = sp.score;
    P.ncig = sp.ncig;
    P.sr_off = sp.sr_off;
    P.cig_at = sp.cig_at;
    P.lr_off = sp.lr_off;
    P.cig = sp.cig;
    int max_bins = 0;
    if ((rc = c->pb[PB_ERR].ensure(((size_t)n_lr + 1) * 4)) ||
        (rc = binfilter_setup(c, P, sp.n_task, lo.data(), n_lr, bin_size, &max_bins)))
        return rc;
    P.err = c->pb[PB_ERR].as<int32_t>();
    HIPCHK(hipMemsetAsync(c->pb[PB_ERR].p, 0, (size_t)n_lr * 4, c->stream));
    const int grid_f = n_lr < c->n_cu * 8 ? n_lr : c->n_cu * 8;
    const int e = pipe_binfilter_launch(P, bin_size, bin_length, max_bins, grid_f, (void *)c->stream);
    if (e) return set_error(PR_ERR_HIP, "-b/-l filter kernel: %s", hipGetErrorString((hipError_t)e));
    std::vector<int32_t> err((size_t)n_lr);
    HIPCHK(hipMemcpyAsync(err.data(), c->pb[PB_ERR].p, (size_t)n_lr * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n_lr; ++i)
        if (err[(size_t)i]) return set_error(PR_ERR_CAPACITY, "-b/-l filter of long read %d failed (code %d)", i, err[(size_t)i]);
    return sw_keep_to_sam(c, c->pb[PB_F_KEEP].as<uint8_t>(), keep);
}

extern "C" int pr_iter_download(pr_ctx *c, pr_cns_out *o) {
    if (!c) return set_error(PR_ERR_ARG, "null ctx");
    int rc = pr_cns_download(c, o);
    if (rc || !c->pipe || !c->n_lr) return rc;
    // the hand-off's per-read error flags (sort capacity, filter bin range): never silent
    std::vector<int32_t> err((size_t)c->n_lr);
    HIPCHK(hipMemcpy(err.data(), c->pb[PB_ERR].p, (size_t)c->n_lr * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < c->n_lr; ++i)
        if (err[(size_t)i]) return set_error(PR_ERR_CAPACITY, "hand-off of long read %d failed (code %d)", i, err[(size_t)i]);
    return 0;
}

extern "C" int pr_iter_download_range(pr_ctx *c, int32_t first, int32_t n, pr_cns_out *o) {
    // reads [first, first + n) of the last launch: the per-read arrays have n entries, out_off /
    // chim_off n + 1 entries counted from the range's first read
    if (!c || !o) return set_error(PR_ERR_ARG, "null arg");
    if (first < 0 || n < 0 || (int64_t)first + n > c->n_lr) return set_error(PR_ERR_ARG, "read range outside the batch");
    if (o->kept || o->bin_bases) return set_error(PR_ERR_ARG, "kept / bin_bases: pr_iter_download");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (!c->cns_launched) return set_error(PR_ERR_ARG, "no consensus launch to download");
    const size_t f = (size_t)first, m = (size_t)n;
    const int64_t o0 = c->out_off[f], o1 = c->out_off[f + m], h0 = c->chim_off[f], h1 = c->chim_off[f + m];
    if (o->out_off)
        for (size_t i = 0; i <= m; ++i) o->out_off[i] = c->out_off[f + i] - o0;
    if (o->chim_off)
        for (size_t i = 0; i <= m; ++i) o->chim_off[i] = c->chim_off[f + i] - h0;
    DevBuf *B = c->cb;
    int rc;
    if ((rc = download(o->status, B[CB_STATUS], m, s, f)) || (rc = download(o->seq_len, B[CB_SEQ_LEN], m, s, f)) ||
        (rc = download(o->trace_len, B[CB_TRACE_LEN], m, s, f)) || (rc = download(o->ncigar, B[CB_NCIGAR], m, s, f)) ||
        (rc = download(o->nchim, B[CB_NCHIM], m, s, f)) || (rc = download(o->seq, B[CB_O_SEQ], (size_t)(o1 - o0), s, (size_t)o0)) ||
        (rc = download(o->qual, B[CB_O_QUAL], (size_t)(o1 - o0), s, (size_t)o0)) ||
        (rc = download(o->trace, B[CB_O_TRACE], (size_t)(o1 - o0), s, (size_t)o0)) ||
        (rc = download(o->cigar, B[CB_O_CIG], (size_t)(o1 - o0), s, (size_t)o0)) ||
        (rc = download(o->chim, B[CB_O_CHIM], (size_t)(h1 - h0) * 4, s, (size_t)h0 * 4)))
        return rc;
    std::vector<int32_t> err(m + 1, 0);
    if (c->pipe && m) HIPCHK(hipMemcpyAsync(err.data(), c->pb[PB_ERR].as<int32_t>() + f, m * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (size_t i = 0; i < m; ++i)
        if (err[i]) return set_error(PR_ERR_CAPACITY, "hand-off of long read %d failed (code %d)", first + (int)i, err[i]);
    return 0;
}

extern "C" int pr_iter_handoff_stats(pr_ctx *c, int64_t *big_reads, int64_t *big_alns, int32_t *max_alns) {
    if (!c) return set_error(PR_ERR_ARG, "null ctx");
    if (!c->pipe || !c->ho_done) return set_error(PR_ERR_ARG, "no hand-off yet (pr_iter_launch first)");
    if (big_reads) *big_reads = c->ho.n_big;   // the host's plan: no device access
    if (!big_alns && !max_alns) return 0;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int32_t> cnt((size_t)c->n_lr + 1, 0);
    if (c->n_lr) HIPCHK(hipMemcpyAsync(cnt.data(), c->pb[PB_CNT].p, (size_t)c->n_lr * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int64_t ba = 0;
    int32_t mx = 0;
    for (int32_t lr : c->ho.big_lr) ba += cnt[(size_t)lr];
    for (int i = 0; i < c->n_lr; ++i) mx = std::max(mx, cnt[(size_t)i]);
    if (big_alns) *big_alns = ba;
    if (max_alns) *max_alns = mx;
    return 0;
}

extern "C" int pr_iter_handoff_order(pr_ctx *c, int32_t lr, int32_t *task_idx, int64_t cap, int64_t *n) {
    if (!c || !n) return set_error(PR_ERR_ARG, "null arg");
    if (!c->pipe || !c->ho_done) return set_error(PR_ERR_ARG, "no hand-off yet (pr_iter_launch first)");
    if (lr < 0 || lr >= c->n_lr) return set_error(PR_ERR_ARG, "long read %d outside the batch", lr);
    HIPCHK(hipSetDevice(c->device));
    int64_t a[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(a, c->cb[CB_ALN_OFF].as<int64_t>() + lr, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n = a[1] - a[0];
    if (!task_idx) return 0;
    if (*n > cap) return set_error(PR_ERR_CAPACITY, "hand-off order: %lld alignments, room for %lld", (long long)*n, (long long)cap);
    if (*n) {
        HIPCHK(hipMemcpyAsync(task_idx, c->pb[PB_ORDER].as<int32_t>() + a[0], (size_t)*n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int pr_iter_last_timing(pr_ctx *c, double *ms_sw_extend, double *ms_sw_global, double *ms_assemble,
                                   double *ms_consensus) {
    // HIP events of the last pr_iter_launch (the caller has synchronised):
    // ev2 | SW extend | ev3 | SW global | ev0 | hand-off | ev4 | consensus | ev5
    if (!c) return set_error(PR_ERR_ARG, "null ctx");
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const int pairs[4][2] = {{2, 3}, {3, 0}, {0, 4}, {4, 5}};
    for (int k = 0; k < 4; ++k)
        if (hipEventElapsedTime(&v[k], c->ev[pairs[k][0]], c->ev[pairs[k][1]]) != hipSuccess) v[k] = 0.f;
    if (ms_sw_extend) *ms_sw_extend = v[0];
    if (ms_sw_global) *ms_sw_global = v[1];
    if (ms_assemble) *ms_assemble = v[2];
    if (ms_consensus) *ms_consensus = v[3];
    return 0;
}

extern "C" int pr_iter_alignment_stats(pr_ctx *c, int64_t *n_aln, int64_t *sum_ncig, int64_t *sum_lseq) {
    // reported alignments of the last iteration (for the SURVEY.md §8d pileup byte model)
    if (!c || !c->pipe) return set_error(PR_ERR_ARG, "no resident iteration batch");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    int64_t na = 0;
    HIPCHK(hipMemcpy(&na, c->cb[CB_ALN_OFF].as<int64_t>() + c->n_lr, 8, hipMemcpyDeviceToHost));
    std::vector<int32_t> v((size_t)na + 1);
    int64_t sc = 0, sl = 0;
    if (na) {
        HIPCHK(hipMemcpy(v.data(), c->cb[CB_NCIG].p, (size_t)na * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < na; ++i) sc += v[i];
        HIPCHK(hipMemcpy(v.data(), c->cb[CB_LSEQ].p, (size_t)na * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < na; ++i) sl += v[i];
    }
    if (n_aln) *n_aln = na;
    if (sum_ncig) *sum_ncig = sc;
    if (sum_lseq) *sum_lseq = sl;
    return 0;
}

extern "C" int pr_iter_bounds(pr_ctx *c, int32_t *n_lr, int64_t *n_task, pr_cns_bounds *bd) {
    if (!c || !c->pipe) return set_error(PR_ERR_ARG, "no resident iteration batch");
    if (n_lr) *n_lr = c->n_lr;
    if (n_task) *n_task = c->n_aln;
    if (bd) { bd->seq_cap = c->seq_cap; bd->chim_cap = c->chim_cap; }
    return 0;
}

extern "C" int pr_iter_stats(pr_ctx *c, int32_t min_phred, int64_t *dev_out) {
    if (!c || !dev_out) return set_error(PR_ERR_ARG, "null arg");
    if (!c->cns_loaded) return set_error(PR_ERR_ARG, "no resident consensus batch");
    HIPCHK(hipSetDevice(c->device));
    DevBuf *B = c->cb;
    int e = iter_stats_launch(B[CB_OUT_OFF].as<int64_t>(), B[CB_STATUS].as<int32_t>(), B[CB_SEQ_LEN].as<int32_t>(),
                              B[CB_O_QUAL].as<uint8_t>(), c->n_lr, min_phred + 33,
                              reinterpret_cast<unsigned long long *>(dev_out), (void *)c->stream);
    if (e) return set_error(PR_ERR_HIP, "stats kernel: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

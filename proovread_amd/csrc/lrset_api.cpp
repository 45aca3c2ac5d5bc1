// The resident long-read set (include/prgpu.h pr_lrset_*): the loop's LR.fq and LR.masked.fa
// between tasks, in HBM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "pipe_dev.h"

extern "C" int pr_lrset_load(pr_ctx *c, int32_t n_lr, const int64_t *off, const uint8_t *seq, const uint8_t *qual) {
    if (!c || n_lr < 0 || !off || (n_lr && (!seq || !qual))) return set_error(PR_ERR_ARG, "null arg");
    if (off[0] != 0) return set_error(PR_ERR_ARG, "offsets must start at 0");
    for (int i = 0; i < n_lr; ++i)
        if (off[i + 1] < off[i]) return set_error(PR_ERR_ARG, "offsets not monotone");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t nb = (size_t)off[n_lr];
    int rc;
    if ((rc = upload(c->ls[LS_SEQ], seq, nb, s)) || (rc = upload(c->ls[LS_QUAL], qual, nb, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    c->ls_off.assign(off, off + n_lr + 1);
    c->ls_n = n_lr;
    c->ls_map_is_reads = true;   // read-long: the mapping reference is the reads themselves
    return 0;
}

extern "C" int pr_lrset_snapshot(pr_ctx *c) {
    if (!c || c->ls_n < 0) return set_error(PR_ERR_ARG, "no resident long-read set (pr_lrset_load)");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t nb = (size_t)c->ls_off.back();
    int rc;
    if ((rc = c->ls[LS_RSEQ].ensure(nb + 1)) || (rc = c->ls[LS_RQUAL].ensure(nb + 1))) return rc;
    if (nb) {
        HIPCHK(hipMemcpyAsync(c->ls[LS_RSEQ].p, c->ls[LS_SEQ].p, nb, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(c->ls[LS_RQUAL].p, c->ls[LS_QUAL].p, nb, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    c->ls_raw_off = c->ls_off;
    return 0;
}

extern "C" int pr_lrset_restore(pr_ctx *c) {
    if (!c || c->ls_n < 0) return set_error(PR_ERR_ARG, "no resident long-read set (pr_lrset_load)");
    if (c->ls_raw_off.empty()) return set_error(PR_ERR_ARG, "no snapshot of the long-read set (pr_lrset_snapshot)");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t nb = (size_t)c->ls_raw_off.back();
    int rc;
    if ((rc = c->ls[LS_SEQ].ensure(nb + 1)) || (rc = c->ls[LS_QUAL].ensure(nb + 1))) return rc;
    if (nb) {   // stream-ordered after every launch that read the set
        HIPCHK(hipMemcpyAsync(c->ls[LS_SEQ].p, c->ls[LS_RSEQ].p, nb, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(c->ls[LS_QUAL].p, c->ls[LS_RQUAL].p, nb, hipMemcpyDeviceToDevice, s));
    }
    c->ls_off = c->ls_raw_off;
    c->ls_n = (int32_t)c->ls_off.size() - 1;
    c->ls_map_is_reads = true;   // read-long: the mapping reference is the reads themselves
    return 0;
}

extern "C" int pr_lrset_info(pr_ctx *c, int32_t *n_lr, int64_t *bases) {
    if (!c || c->ls_n < 0) return set_error(PR_ERR_ARG, "no resident long-read set (pr_lrset_load)");
    if (n_lr) *n_lr = c->ls_n;
    if (bases) *bases = c->ls_off.back();
    return 0;
}

extern "C" int pr_lrset_download(pr_ctx *c, int64_t *off, uint8_t *seq, uint8_t *qual, uint8_t *map) {
    if (!c || c->ls_n < 0) return set_error(PR_ERR_ARG, "no resident long-read set (pr_lrset_load)");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t nb = (size_t)c->ls_off.back();
    if (off) std::memcpy(off, c->ls_off.data(), c->ls_off.size() * 8);
    int rc;
    if ((rc = download(seq, c->ls[LS_SEQ], nb, s)) || (rc = download(qual, c->ls[LS_QUAL], nb, s)) ||
        (rc = download(map, c->ls[c->ls_map_is_reads ? LS_SEQ : LS_MAP], nb, s)))
        return rc;
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int pr_lrset_set_map(pr_ctx *c, const uint8_t *map) {
    if (!c || c->ls_n < 0) return set_error(PR_ERR_ARG, "no resident long-read set (pr_lrset_load)");
    const size_t nb = (size_t)c->ls_off.back();
    if (nb && !map) return set_error(PR_ERR_ARG, "null arg");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    if ((rc = upload(c->ls[LS_MAP], map, nb, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    c->ls_map_is_reads = false;
    return 0;
}

extern "C" int pr_lrset_index(pr_ctx *c, int which) {
    if (!c || c->ls_n < 0) return set_error(PR_ERR_ARG, "no resident long-read set (pr_lrset_load)");
    if (which != PR_LRSET_MAP && which != PR_LRSET_READS) return set_error(PR_ERR_ARG, "which: PR_LRSET_MAP / _READS");
    const int id = which == PR_LRSET_READS || c->ls_map_is_reads ? LS_SEQ : LS_MAP;
    return index_build(c, c->ls[id].as<uint8_t>(), c->ls_off.data(), c->ls_n, true);
}

extern "C" int pr_iter_upload_lrset(pr_ctx *c, const pr_sw_batch *b) {
    if (!c || !b) return set_error(PR_ERR_ARG, "null arg");
    if (c->ls_n < 0) return set_error(PR_ERR_ARG, "no resident long-read set (pr_lrset_load)");
    if (!c->seed_n_text || c->seed_view.n_lr != c->ls_n || c->seed_view.l_pac != c->ls_off.back())
        return set_error(PR_ERR_ARG, "the seed index is not over the long-read set (pr_lrset_index first)");
    if (c->seed_pre.size() != (size_t)b->n_sr + 1)
        return set_error(PR_ERR_ARG, "no device seeds for these short reads (pr_seed_gpu_map with out = NULL first)");
    if (!b->sr_seq && b->n_sr && c->seed_sr_bases != b->sr_off[b->n_sr])
        return set_error(PR_ERR_ARG, "sr_seq NULL: the short reads must be those of the last pr_seed_gpu_map");
    pr_iter_batch ib;
    std::memset(&ib, 0, sizeof ib);
    ib.sw = *b;
    ib.sw.n_lr = c->ls_n;
    ib.sw.lr_off = c->ls_off.data();
    ib.sw.lr_seq = nullptr;
    const int rc = iter_upload(c, &ib, true, b->sr_seq ? nullptr : c->sd[SB_SEQ].as<uint8_t>(),
                               c->sd[SX_LRSEQ].as<uint8_t>(), c->ls[LS_SEQ].as<uint8_t>(), c->ls[LS_QUAL].as<uint8_t>());
    if (!rc && !b->sr_seq) c->seed_sr_bases = -1;   // handed over once (as pr_sw_upload_gpu_seeds)
    return rc;
}

// pr_lrset_commit's checks on this rank: the launch, the masking, every read's hand-off and
// consensus status (as pr_iter_download: never silent); fills the per-read status and length
static int commit_check(pr_ctx *c, int world, bool with_mask, int lr0, int n, std::vector<int32_t> &st,
                        std::vector<int32_t> &len, std::vector<int32_t> &herr) {
    if (!c->cns_launched || !c->pipe) return set_error(PR_ERR_ARG, "no iteration launch to commit");
    if (with_mask && !c->iter_masked) return set_error(PR_ERR_ARG, "with_mask: no pr_iter_mask launch");
    if (world == 1 && (lr0 != 0 || n != c->ls_n)) return set_error(PR_ERR_ARG, "the batch must hold every long read");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    if (with_mask && (rc = mask_check_err(c))) return rc;
    if (n) {
        HIPCHK(hipMemcpyAsync(st.data(), c->cb[CB_STATUS].p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(len.data(), c->cb[CB_SEQ_LEN].p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(herr.data(), c->pb[PB_ERR].p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        if (herr[(size_t)i])
            return set_error(PR_ERR_CAPACITY, "hand-off of long read %d failed (code %d)", lr0 + i, herr[(size_t)i]);
        if (st[(size_t)i]) return set_error(st[(size_t)i], "consensus of long read %d failed (status %d)", lr0 + i, st[(size_t)i]);
    }
    return 0;
}

extern "C" int pr_lrset_commit(pr_ctx *c, pr_comm *comm, int flags) {
    if (!c || c->ls_n < 0) return set_error(PR_ERR_ARG, "no resident long-read set (pr_lrset_load)");
    int rank = 0, world = 1, rc;
    if (comm && (rc = pr_comm_rank(comm, &rank, &world))) return rc;
    if (comm && comm_ctx(comm) != c) return set_error(PR_ERR_ARG, "the communicator belongs to another context");
    const bool dry = (flags & PR_LRSET_COMMIT_DRY) != 0, with_mask = (flags & PR_LRSET_COMMIT_MASK) != 0;
    const int lr0 = c->own ? c->own_lr0 : 0, n = c->n_lr;
    std::vector<int32_t> st((size_t)n + 1, 0), len((size_t)n + 1, 0), herr((size_t)n + 1, 0);
    // local checks first; with ranks, every rank learns whether all passed before any collective
    rc = commit_check(c, world, with_mask, lr0, n, st, len, herr);
    if (world > 1) rc = pr_comm_agree(comm, rc);
    if (rc) return rc;
    hipStream_t s = c->stream;
    std::vector<int64_t> doff((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) doff[(size_t)i + 1] = doff[(size_t)i] + len[(size_t)i];
    const int64_t own = doff[(size_t)n];
    DevBuf *L = c->ls;
    // the compaction's buffers and launch are local too: with ranks, agree again before the
    // first collective so a rank that failed here does not leave the others inside it
    if (!(rc = upload(L[LS_OFF], doff.data(), (size_t)n + 1, s)) && !(rc = L[LS_TSEQ].ensure((size_t)own + 1)) &&
        !(rc = L[LS_TQUAL].ensure((size_t)own + 1)) && !(with_mask && (rc = L[LS_TMAP].ensure((size_t)own + 1)))) {
        const int e = lr_compact_launch(c->cb[CB_OUT_OFF].as<int64_t>(), c->cb[CB_SEQ_LEN].as<int32_t>(),
                                        L[LS_OFF].as<int64_t>(), n, c->cb[CB_O_SEQ].as<uint8_t>(), L[LS_TSEQ].as<uint8_t>(),
                                        c->cb[CB_O_QUAL].as<uint8_t>(), L[LS_TQUAL].as<uint8_t>(),
                                        with_mask ? c->mb[MB_OUT].as<uint8_t>() : nullptr,
                                        with_mask ? L[LS_TMAP].as<uint8_t>() : nullptr, (void *)s);
        if (e) rc = set_error(PR_ERR_HIP, "long-read set compaction: %s", hipGetErrorString((hipError_t)e));
    }
    if (world > 1) rc = pr_comm_agree(comm, rc);
    if (rc) return rc;
    std::vector<int64_t> off((size_t)c->ls_n + 1, 0);
    if (world == 1) {
        if (!dry) {
            std::swap(L[LS_SEQ], L[LS_TSEQ]);
            std::swap(L[LS_QUAL], L[LS_TQUAL]);
            if (with_mask) std::swap(L[LS_MAP], L[LS_TMAP]);
        }
        off = doff;
    } else {
        // every rank's owned reads in rank order (= global order: the owners' ranges ascend):
        // the lengths all-gathered on the host (small), the pools on the device
        std::vector<int64_t> cnt((size_t)world, 0);
        cnt[(size_t)rank] = n;
        if ((rc = pr_comm_allreduce_host(comm, cnt.data(), world, PR_DT_I64, PR_RED_SUM))) return rc;
        int64_t tot_n = 0;
        for (int r = 0; r < world; ++r) tot_n += cnt[(size_t)r];
        if (tot_n != c->ls_n) return set_error(PR_ERR_ARG, "the ranks' owned reads do not make up the set");
        std::vector<int64_t> lens((size_t)c->ls_n, 0), bytes((size_t)world, 0);
        int64_t first = 0;
        for (int r = 0; r < rank; ++r) first += cnt[(size_t)r];
        for (int i = 0; i < n; ++i) lens[(size_t)(first + i)] = len[(size_t)i];
        if ((rc = pr_comm_allreduce_host(comm, lens.data(), c->ls_n, PR_DT_I64, PR_RED_SUM))) return rc;
        for (int i = 0; i < c->ls_n; ++i) off[(size_t)i + 1] = off[(size_t)i] + lens[(size_t)i];
        int64_t k = 0;
        for (int r = 0; r < world; ++r) {
            bytes[(size_t)r] = off[(size_t)(k + cnt[(size_t)r])] - off[(size_t)k];
            k += cnt[(size_t)r];
        }
        const size_t tot = (size_t)off.back();
        // dry: the same all-gathers into scratch pools, the set unchanged
        const int ids[3][2] = {{LS_TSEQ, dry ? LS_GSEQ : LS_SEQ}, {LS_TQUAL, dry ? LS_GQUAL : LS_QUAL},
                               {LS_TMAP, dry ? LS_GMAP : LS_MAP}};
        const int nq = with_mask ? 3 : 2;
        // every gather target first, then one more agreement: no rank enters an all-gather that
        // another cannot reach for want of memory
        for (int q = 0; q < nq && !rc; ++q) rc = L[ids[q][1]].ensure(tot + 1);
        rc = pr_comm_agree(comm, rc);
        for (int q = 0; q < nq && !rc; ++q)
            rc = pr_comm_allgatherv_dev(comm, L[ids[q][0]].p, bytes.data(), L[ids[q][1]].p);
        if (dry) {   // the scratch pools of a dry commit are not kept (configs[3]: ~3 x 2.9 GB)
            HIPCHK(hipStreamSynchronize(s));
            for (int q = 0; q < nq; ++q) L[ids[q][1]].release();
        }
        if (rc) return rc;
    }
    HIPCHK(hipStreamSynchronize(s));
    if (dry) return 0;
    c->ls_off = off;
    if (with_mask) c->ls_map_is_reads = false;
    else c->ls_map_is_reads = true;   // the finish task: the reads are their own mapping reference
    return 0;
}

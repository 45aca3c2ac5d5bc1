// The exact-parity multi-GPU layout's host side (include/prgpu.h: pr_sw_upload_gpu_seeds,
// pr_aln_exchange, pr_iter_upload_owned, then pr_iter_launch on the owned batch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "xchg_dev.h"

extern "C" int pr_sw_upload_gpu_seeds(pr_ctx *c, const pr_sw_batch *b) {
    if (!c || !b) return set_error(PR_ERR_ARG, "null arg");
    if (c->seed_pre.size() != (size_t)b->n_sr + 1)
        return set_error(PR_ERR_ARG, "no device seeds for these short reads (pr_seed_gpu_map with out = NULL first)");
    pr_sw_batch sb = *b;
    sb.n_task = c->seed_pre.back();
    sb.t_sr = sb.t_lr = sb.t_qbeg = sb.t_rbeg = sb.t_slen = sb.t_chain = nullptr;
    sb.t_strand = nullptr;
    // pools left NULL: the device copies the seeding made (no second host upload)
    const uint8_t *dsr = nullptr, *dlr = nullptr;
    if (!b->sr_seq) {
        if (b->n_sr && c->seed_sr_bases != b->sr_off[b->n_sr])
            return set_error(PR_ERR_ARG, "sr_seq NULL: the short reads must be those of the last pr_seed_gpu_map");
        dsr = c->sd[SB_SEQ].as<uint8_t>();
    }
    if (!b->lr_seq) {
        if (!c->seed_n_text || c->seed_view.l_pac != b->lr_off[b->n_lr] || c->seed_view.n_lr != b->n_lr)
            return set_error(PR_ERR_ARG, "lr_seq NULL: the long reads must be those of the last pr_seed_gpu_index_build");
        dlr = c->sd[SX_LRSEQ].as<uint8_t>();
    }
    c->x_ready = c->x_pass = false;   // a new SW batch: no exchange of it yet
    const int rc = sw_upload_device_seeds(c, &sb, c->sd[SB_DENSE].as<pr_seed_task>(), c->seed_pre.data(), dsr, dlr);
    // the seeding's short-read pool is handed over once: a later batch with the same base count
    // (another sample, another shard) must not pick it up silently (the next map sets it again)
    if (!rc && dsr) c->seed_sr_bases = -1;
    return rc;
}

// the sender half of the exchange: the reported alignments of the last bwa-mode pr_sw_launch
// packed by owner into XB_SREC / XB_SCIG; counts (records, ops) per owner into cnt (syncs)
static int xchg_pack(pr_ctx *c, int world, int64_t sr0, const int64_t *lr_bounds, std::vector<int64_t> &n_rec,
                     std::vector<int64_t> &n_ops) {
    if (world < 1 || world > 64) return set_error(PR_ERR_CAPACITY, "1 to 64 ranks");
    if (lr_bounds[0] != 0) return set_error(PR_ERR_ARG, "lr_bounds must start at 0");
    for (int r = 0; r < world; ++r)
        if (lr_bounds[r + 1] < lr_bounds[r]) return set_error(PR_ERR_ARG, "lr_bounds must be ascending");
    XchgSend X;
    std::memset(&X, 0, sizeof X);
    int rc;
    if ((rc = sw_xchg_send(c, &X))) return rc;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevBuf *B = c->xb;
    const size_t n1 = (size_t)X.n + 1;
    if ((rc = upload(B[XB_BOUNDS], lr_bounds, (size_t)world + 1, s)) || (rc = B[XB_KEY0].ensure(n1 * 4)) ||
        (rc = B[XB_KEY1].ensure(n1 * 4)) || (rc = B[XB_IDX0].ensure(n1 * 4)) || (rc = B[XB_IDX1].ensure(n1 * 4)) ||
        (rc = B[XB_CNT].ensure(2 * 65 * 8)) || (rc = B[XB_OPIN].ensure(n1 * 8)) || (rc = B[XB_OPAT].ensure(n1 * 8)) ||
        (rc = B[XB_SREC].ensure(n1 * sizeof(XRec))))
        return rc;
    const size_t tb = xchg_temp_bytes(X.n, 1);
    if ((rc = B[XB_TEMP].ensure(tb))) return rc;
    X.bounds = B[XB_BOUNDS].as<int64_t>();
    X.world = world;
    X.sr0 = sr0;
    X.key0 = B[XB_KEY0].as<int32_t>();
    X.key1 = B[XB_KEY1].as<int32_t>();
    X.idx0 = B[XB_IDX0].as<int32_t>();
    X.idx1 = B[XB_IDX1].as<int32_t>();
    X.cnt = B[XB_CNT].as<unsigned long long>();
    X.op_in = B[XB_OPIN].as<int64_t>();
    X.op_at = B[XB_OPAT].as<int64_t>();
    X.rec = B[XB_SREC].as<XRec>();
    int e = xchg_pack_launch(X, B[XB_TEMP].p, B[XB_TEMP].cap, (void *)s);
    if (e) return set_error(PR_ERR_HIP, "exchange pack: %s", hipGetErrorString((hipError_t)e));
    std::vector<unsigned long long> cnt((size_t)2 * (world + 1), 0ull);
    HIPCHK(hipMemcpyAsync(cnt.data(), X.cnt, cnt.size() * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    n_rec.assign((size_t)world, 0);
    n_ops.assign((size_t)world, 0);
    int64_t ops = 0;
    for (int r = 0; r < world; ++r) {
        n_rec[(size_t)r] = (int64_t)cnt[(size_t)r];
        n_ops[(size_t)r] = (int64_t)cnt[(size_t)world + 1 + r];
        ops += n_ops[(size_t)r];
    }
    if ((rc = B[XB_SCIG].ensure(((size_t)ops + 1) * 4))) return rc;
    X.wcig = B[XB_SCIG].as<uint32_t>();
    if ((e = xchg_write_launch(X, (void *)s))) return set_error(PR_ERR_HIP, "exchange pack: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

static int xchg_recv_buffers(pr_ctx *c, int64_t rec_bytes, int64_t cig_bytes) {
    if (rec_bytes % (int64_t)sizeof(XRec)) return set_error(PR_ERR_ARG, "exchange: ragged record counts");
    c->x_nrecv = rec_bytes / (int64_t)sizeof(XRec);
    c->x_nrcig = cig_bytes / 4;
    int rc;
    if ((rc = c->xb[XB_RREC].ensure((size_t)rec_bytes + sizeof(XRec))) || (rc = c->xb[XB_RCIG].ensure((size_t)cig_bytes + 64)))
        return rc;
    return 0;
}

extern "C" int pr_aln_exchange(pr_ctx *c, pr_comm *comm, int64_t sr0, const int64_t *lr_bounds, int64_t *n_recv) {
    if (!c || !lr_bounds) return set_error(PR_ERR_ARG, "null arg");
    int rank = 0, world = 1, rc;
    if (comm) {
        if (comm_ctx(comm) != c) return set_error(PR_ERR_ARG, "the communicator belongs to another context");
        if ((rc = pr_comm_rank(comm, &rank, &world))) return rc;
    }
    c->x_ready = false;
    c->x_pass = false;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->ev[0], c->stream));   // pr_iter_last_timing: the hand-off includes the exchange
    if (world == 1 && sr0 == 0 && !getenv("PRGPU_XCHG_FORCE")) {
        // one rank holding every short read: it owns every long read, nothing moves -- the owned
        // launch takes the SW output directly (PRGPU_XCHG_FORCE=1: pack and copy anyway, a test hook)
        XchgSend X;
        if ((rc = sw_xchg_send(c, &X))) return rc;
        c->x_pass = true;
        c->x_ready = true;
        c->x_nrecv = X.n;
        c->x_from.assign(1, X.n);
        if (n_recv) *n_recv = X.n;
        return 0;
    }
    std::vector<int64_t> nrec, nops;
    rc = xchg_pack(c, world, sr0, lr_bounds, nrec, nops);
    // the pack is local: every rank learns whether all packed before any data moves
    if (comm) rc = pr_comm_agree(comm, rc);
    if (rc) return rc;
    std::vector<int64_t> sc_rec((size_t)world), sc_cig((size_t)world), rc_rec((size_t)world), rc_cig((size_t)world);
    for (int r = 0; r < world; ++r) {
        sc_rec[(size_t)r] = nrec[(size_t)r] * (int64_t)sizeof(XRec);
        sc_cig[(size_t)r] = nops[(size_t)r] * 4;
    }
    if (comm) {
        if ((rc = pr_comm_alltoall_counts(comm, sc_rec.data(), rc_rec.data())) ||
            (rc = pr_comm_alltoall_counts(comm, sc_cig.data(), rc_cig.data())))
            return rc;
    } else {
        rc_rec = sc_rec;
        rc_cig = sc_cig;
    }
    int64_t nr = 0, nc = 0;
    c->x_from.assign((size_t)world, 0);
    for (int r = 0; r < world; ++r) {
        nr += rc_rec[(size_t)r];
        nc += rc_cig[(size_t)r];
        c->x_from[(size_t)r] = rc_rec[(size_t)r] / (int64_t)sizeof(XRec);
    }
    rc = xchg_recv_buffers(c, nr, nc);
    // the receive buffers are a local allocation: a rank that could not get them must not leave
    // the others inside the all-to-all
    if (comm) rc = pr_comm_agree(comm, rc);
    if (rc) return rc;
    DevBuf *B = c->xb;
    if (comm) {
        if ((rc = pr_comm_alltoallv_dev(comm, B[XB_SREC].p, sc_rec.data(), B[XB_RREC].p, rc_rec.data())) ||
            (rc = pr_comm_alltoallv_dev(comm, B[XB_SCIG].p, sc_cig.data(), B[XB_RCIG].p, rc_cig.data())))
            return rc;
    } else {
        HIPCHK(hipSetDevice(c->device));
        if (nr) HIPCHK(hipMemcpyAsync(B[XB_RREC].p, B[XB_SREC].p, (size_t)nr, hipMemcpyDeviceToDevice, c->stream));
        if (nc) HIPCHK(hipMemcpyAsync(B[XB_RCIG].p, B[XB_SCIG].p, (size_t)nc, hipMemcpyDeviceToDevice, c->stream));
    }
    c->x_ready = true;
    if (n_recv) *n_recv = c->x_nrecv;
    return 0;
}

extern "C" int pr_aln_exchange_local(pr_ctx *const *ctxs, int world, const int64_t *sr0, const int64_t *lr_bounds,
                                     int64_t *n_recv) {
    // the same exchange among `world` contexts of one process (e.g. several shards on one GPU):
    // the packs, then device-to-device block copies in source order instead of RCCL
    if (!ctxs || !sr0 || !lr_bounds || world < 1) return set_error(PR_ERR_ARG, "bad arg");
    std::vector<std::vector<int64_t>> nrec((size_t)world), nops((size_t)world);
    int rc;
    for (int k = 0; k < world; ++k) {
        if (!ctxs[k]) return set_error(PR_ERR_ARG, "null context");
        ctxs[k]->x_ready = false;
        ctxs[k]->x_pass = false;   // the owned launch reads the records copied below
        if ((rc = xchg_pack(ctxs[k], world, sr0[k], lr_bounds, nrec[(size_t)k], nops[(size_t)k]))) return rc;
    }
    for (int k = 0; k < world; ++k) {
        HIPCHK(hipSetDevice(ctxs[k]->device));
        HIPCHK(hipStreamSynchronize(ctxs[k]->stream));
    }
    for (int r = 0; r < world; ++r) {
        pr_ctx *d = ctxs[r];
        int64_t nr = 0, nc = 0;
        d->x_from.assign((size_t)world, 0);
        for (int k = 0; k < world; ++k) {
            nr += nrec[(size_t)k][(size_t)r] * (int64_t)sizeof(XRec);
            nc += nops[(size_t)k][(size_t)r] * 4;
            d->x_from[(size_t)k] = nrec[(size_t)k][(size_t)r];
        }
        if ((rc = xchg_recv_buffers(d, nr, nc))) return rc;
        int64_t ro = 0, co = 0;
        for (int k = 0; k < world; ++k) {
            int64_t so = 0, sco = 0;   // this destination's block in the source's send buffers
            for (int q = 0; q < r; ++q) {
                so += nrec[(size_t)k][(size_t)q] * (int64_t)sizeof(XRec);
                sco += nops[(size_t)k][(size_t)q] * 4;
            }
            const int64_t bn = nrec[(size_t)k][(size_t)r] * (int64_t)sizeof(XRec), bc = nops[(size_t)k][(size_t)r] * 4;
            HIPCHK(hipSetDevice(d->device));
            if (bn) HIPCHK(hipMemcpyAsync((uint8_t *)d->xb[XB_RREC].p + ro, (uint8_t *)ctxs[k]->xb[XB_SREC].p + so,
                                          (size_t)bn, hipMemcpyDeviceToDevice, d->stream));
            if (bc) HIPCHK(hipMemcpyAsync((uint8_t *)d->xb[XB_RCIG].p + co, (uint8_t *)ctxs[k]->xb[XB_SCIG].p + sco,
                                          (size_t)bc, hipMemcpyDeviceToDevice, d->stream));
            ro += bn;
            co += bc;
        }
        HIPCHK(hipStreamSynchronize(d->stream));
        d->x_ready = true;
        if (n_recv) n_recv[r] = d->x_nrecv;
    }
    return 0;
}

extern "C" int pr_aln_exchange_sources(pr_ctx *c, int64_t *per_rank, int cap, int *world) {
    if (!c || (cap && !per_rank)) return set_error(PR_ERR_ARG, "null arg");
    if (!c->x_ready) return set_error(PR_ERR_ARG, "no exchange yet");
    for (int r = 0; r < cap && r < (int)c->x_from.size(); ++r) per_rank[r] = c->x_from[(size_t)r];
    if (world) *world = (int)c->x_from.size();
    return 0;
}

extern "C" int pr_iter_upload_owned(pr_ctx *c, const pr_own_batch *b) {
    if (!c || !b) return set_error(PR_ERR_ARG, "null arg");
    const int n = b->n_lr;
    if (n < 0 || b->n_sr < 0 || (n && !b->lr_off) || !b->sr_off)
        return set_error(PR_ERR_ARG, "owned batch: lr_off and the short-read offsets are required");
    if (n && b->lr_off[0] != 0) return set_error(PR_ERR_ARG, "lr_off must start at 0");
    for (int i = 0; i < n; ++i)
        if (b->lr_off[i + 1] < b->lr_off[i]) return set_error(PR_ERR_ARG, "lr_off not monotone");
    for (int i = 0; i < b->n_sr; ++i)
        if (b->sr_off[i + 1] < b->sr_off[i]) return set_error(PR_ERR_ARG, "sr_off not monotone");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    c->cns_launched = false;
    c->iter_masked = false;
    c->n_lr = n;
    c->n_aln = 0;   // the received alignments (sized at launch: own_group)
    const int64_t tl = n ? b->lr_off[n] : 0;
    c->total_cols = tl;
    c->has_ref = true;
    c->pipe_ref_ascii = true;
    const bool from_set = (b->from_set & PR_OWN_FROM_SET) != 0, sr_res = (b->from_set & PR_OWN_RESIDENT_SR) != 0;
    c->has_qual = b->lr_qual != nullptr || from_set;
    c->has_ign = false;
    c->lr_off_host.assign(b->lr_off, b->lr_off + n + 1);
    if (!n) c->lr_off_host.assign(1, 0);
    c->out_off.assign(n + 1, 0);
    c->chim_off.assign(n + 1, 0);
    cnsp::pipe_caps(b->lr_off, n, c->out_off.data(), c->chim_off.data());
    int64_t set0 = 0;   // from_set: the owned reads' first base in the set
    if (from_set) {
        if (c->ls_n < 0) return set_error(PR_ERR_ARG, "from_set: no resident long-read set");
        if (b->lr0 < 0 || b->lr0 + n > c->ls_n) return set_error(PR_ERR_ARG, "owned long reads outside the set");
        set0 = c->ls_off[(size_t)b->lr0];
        for (int i = 0; i <= n; ++i)
            if (c->ls_off[(size_t)(b->lr0 + i)] - set0 != b->lr_off[i])
                return set_error(PR_ERR_ARG, "owned long reads differ from the set's");
    }
    c->seq_cap = c->out_off[n];
    c->chim_cap = c->chim_off[n];
    c->alg_bytes = 0;
    c->k_need = 1;
    c->pipe_sort_cap = 1;
    c->ho = handp::Plan();
    c->ho_done = false;
    DevBuf *B = c->cb;
    const size_t n1 = (size_t)n + 1;
    if ((rc = upload(B[CB_LR_OFF], c->lr_off_host.data(), n1, s))) return rc;
    if (!from_set && b->lr_qual && (rc = upload(B[CB_REF_QUAL], b->lr_qual, (size_t)tl, s))) return rc;
    // ref_seq / sr_seq NULL: the resident SW batch's long reads (the owned slice, nt4: the mapping
    // reference is the consensus reference) / short reads (every short read of the task) on the device
    SwPtrs sp{};
    if (((!b->ref_seq && !from_set) || (!b->sr_seq && !sr_res)) && (rc = sw_get_ptrs(c, &sp))) return rc;
    c->own_ref_nt4 = !b->ref_seq && !from_set;
    if (from_set) {   // the set's reads and qualities (the previous task's consensus)
        if ((rc = B[CB_REF_SEQ].ensure((size_t)tl + 1)) || (rc = B[CB_REF_QUAL].ensure((size_t)tl + 1))) return rc;
        if (tl) {
            HIPCHK(hipMemcpyAsync(B[CB_REF_SEQ].p, c->ls[LS_SEQ].as<uint8_t>() + set0, (size_t)tl, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(B[CB_REF_QUAL].p, c->ls[LS_QUAL].as<uint8_t>() + set0, (size_t)tl, hipMemcpyDeviceToDevice, s));
        }
    } else if (b->ref_seq) {
        if ((rc = upload(B[CB_REF_SEQ], b->ref_seq, (size_t)tl, s))) return rc;
    } else {
        if (b->lr0 < 0 || b->lr0 + n > sp.n_lr) return set_error(PR_ERR_ARG, "owned long reads outside the SW batch");
        int64_t base = 0, end = 0;
        HIPCHK(hipMemcpyAsync(&base, sp.lr_off + b->lr0, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&end, sp.lr_off + b->lr0 + n, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (end - base != tl) return set_error(PR_ERR_ARG, "owned long reads differ from the SW batch's");
        if ((rc = B[CB_REF_SEQ].ensure((size_t)tl + 1))) return rc;
        if (tl) HIPCHK(hipMemcpyAsync(B[CB_REF_SEQ].p, sp.lr + base, (size_t)tl, hipMemcpyDeviceToDevice, s));
    }
    if ((rc = upload(c->xb[XB_SROFF], b->sr_off, (size_t)b->n_sr + 1, s))) return rc;
    c->own_sr_resident = sr_res;
    if (sr_res) {   // the resident short reads (pr_srset_load, or the task sample) are the task's: read in place
        if (b->sr_seq) return set_error(PR_ERR_ARG, "PR_OWN_RESIDENT_SR: sr_seq must be NULL");
        const std::vector<int64_t> &ro = c->ss_samp_off.empty() ? c->ss_off : c->ss_samp_off;
        // every offset, not only the count and total: a batch with another per-read layout of the
        // same size would read the wrong bases
        if (ro.size() != (size_t)b->n_sr + 1 || !std::equal(ro.begin(), ro.end(), b->sr_off))
            return set_error(PR_ERR_ARG, "PR_OWN_RESIDENT_SR: sr_off differs from the resident short reads (pr_srset_load / "
                                         "pr_srset_sample)");
    } else if (b->sr_seq) {
        if ((rc = upload(c->xb[XB_SR], b->sr_seq, (size_t)b->sr_off[b->n_sr], s))) return rc;
    } else {
        if (sp.n_sr != b->n_sr) return set_error(PR_ERR_ARG, "sr_seq NULL: the SW batch must hold every short read");
        if ((rc = c->xb[XB_SR].ensure((size_t)b->sr_off[b->n_sr] + 1))) return rc;
        if (b->sr_off[b->n_sr])
            HIPCHK(hipMemcpyAsync(c->xb[XB_SR].p, sp.sr, (size_t)b->sr_off[b->n_sr], hipMemcpyDeviceToDevice, s));
    }
    if ((rc = c->pb[PB_CNT].ensure(n1 * 4)) || (rc = c->pb[PB_ERR].ensure(n1 * 4))) return rc;
    if ((rc = cns_ensure(c, cnsp::ALN_OFF | cnsp::READ_OUT))) return rc;
    if ((rc = upload(B[CB_OUT_OFF], c->out_off.data(), n1, s))) return rc;
    if ((rc = upload(B[CB_CHIM_OFF], c->chim_off.data(), n1, s))) return rc;
    DevBuf *X = c->xb;
    if ((rc = X[XB_GCNT].ensure(n1 * 4)) || (rc = X[XB_GCNT64].ensure(n1 * 8)) || (rc = X[XB_TASKOFF].ensure(n1 * 8)) ||
        (rc = X[XB_ERR].ensure(16)))
        return rc;
    HIPCHK(hipStreamSynchronize(s));
    c->own_lr0 = b->lr0;
    c->own = true;
    c->cns_loaded = true;
    c->pipe = true;
    return 0;
}

// owned batch: the received records regrouped by long read into the hand-off's inputs
int own_group(pr_ctx *c, SwPtrs *sp) {
    if (!c->x_ready) return set_error(PR_ERR_ARG, "no received alignments (pr_aln_exchange first)");
    hipStream_t s = c->stream;
    DevBuf *B = c->xb;
    if (c->x_pass) {   // world 1: the SW output regrouped by long read, as pr_iter_launch does
        int rc = sw_get_pipe_ptrs(c, sp, true);
        if (rc) return rc;
        c->n_aln = sp->n_task;
        return cns_ensure(c, cnsp::ALN_IN | cnsp::ALN_SCRATCH);
    }
    {   // per-alignment arrays of the hand-off and the consensus, sized by what arrived
        c->n_aln = c->x_nrecv;
        const size_t na1 = (size_t)c->x_nrecv + 1;
        int rc;
        if ((rc = cns_ensure(c, cnsp::ALN_IN | cnsp::ALN_SCRATCH)) || (rc = B[XB_RCIGAT].ensure(na1 * 8)) ||
            (rc = B[XB_GSR].ensure(na1 * 4)) || (rc = B[XB_GSTATUS].ensure(na1 * 4)) || (rc = B[XB_GPOS].ensure(na1 * 4)) ||
            (rc = B[XB_GSCORE].ensure(na1 * 4)) || (rc = B[XB_GNCIG].ensure(na1 * 4)) ||
            (rc = B[XB_GCIGAT].ensure(na1 * 8)) || (rc = B[XB_GSTRAND].ensure(na1)) || (rc = B[XB_GPASS].ensure(na1)) ||
            (rc = B[XB_KEY0].ensure(na1 * 4)) || (rc = B[XB_KEY1].ensure(na1 * 4)) || (rc = B[XB_IDX0].ensure(na1 * 4)) ||
            (rc = B[XB_IDX1].ensure(na1 * 4)) || (rc = B[XB_OPIN].ensure(na1 * 8)))
            return rc;
        const size_t tb = xchg_temp_bytes(c->x_nrecv, c->n_lr);
        if ((rc = B[XB_TEMP].ensure(tb))) return rc;
    }
    XchgRecv R;
    std::memset(&R, 0, sizeof R);
    R.n = c->x_nrecv;
    R.rec = B[XB_RREC].as<XRec>();
    R.lr0 = c->own_lr0;
    R.n_lr = c->n_lr;
    R.key0 = B[XB_KEY0].as<int32_t>();
    R.key1 = B[XB_KEY1].as<int32_t>();
    R.idx0 = B[XB_IDX0].as<int32_t>();
    R.idx1 = B[XB_IDX1].as<int32_t>();
    R.cnt = B[XB_GCNT].as<int32_t>();
    R.cnt64 = B[XB_GCNT64].as<int64_t>();
    R.task_off = B[XB_TASKOFF].as<int64_t>();
    R.op_in = B[XB_OPIN].as<int64_t>();
    R.rcig_at = B[XB_RCIGAT].as<int64_t>();
    R.err = B[XB_ERR].as<int32_t>();
    R.o_sr = B[XB_GSR].as<int32_t>();
    R.o_status = B[XB_GSTATUS].as<int32_t>();
    R.o_pos = B[XB_GPOS].as<int32_t>();
    R.o_score = B[XB_GSCORE].as<int32_t>();
    R.o_ncig = B[XB_GNCIG].as<int32_t>();
    R.o_cig_at = B[XB_GCIGAT].as<int64_t>();
    R.o_strand = B[XB_GSTRAND].as<uint8_t>();
    R.o_pass = B[XB_GPASS].as<uint8_t>();
    int e = xchg_group_launch(R, B[XB_TEMP].p, B[XB_TEMP].cap, (void *)s);
    if (e) return set_error(PR_ERR_HIP, "exchange regroup: %s", hipGetErrorString((hipError_t)e));
    std::vector<int32_t> &cnt = c->own_cnt_host;
    cnt.assign((size_t)c->n_lr + 1, 0);
    int32_t err = 0;
    if (c->n_lr) HIPCHK(hipMemcpyAsync(cnt.data(), R.cnt, (size_t)c->n_lr * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, R.err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (err) return set_error(PR_ERR_ARG, "exchange: a received alignment lies outside the owned long reads");
    int mx = 0;
    for (int i = 0; i < c->n_lr; ++i) mx = std::max(mx, cnt[(size_t)i]);
    std::memset(sp, 0, sizeof *sp);
    sp->t_sr = R.o_sr;
    sp->status = R.o_status;
    sp->pos = R.o_pos;
    sp->score = R.o_score;
    sp->ncig = R.o_ncig;
    sp->cig_at = R.o_cig_at;
    sp->strand = R.o_strand;
    sp->pass = R.o_pass;
    sp->sr_off = B[XB_SROFF].as<int64_t>();
    sp->cig = B[XB_RCIG].as<uint32_t>();
    sp->n_task = R.n;
    sp->task_off = R.task_off;
    sp->max_per_lr = mx;
    sp->cnt_host = cnt.data();
    return 0;
}

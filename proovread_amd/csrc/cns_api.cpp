// The consensus stage's host side (include/prgpu.h pr_cns_*): a resident batch, its launch and
// download.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.h"
#include "cns_dev.h"
#include "pipe_dev.h"

extern "C" void pr_cns_params_default(pr_cns_params *p) {
    p->max_coverage = 50.0;  // Seq.pm:116 default; proovread passes --coverage
    p->bin_size = 20.0;
    p->trim = 1;
    p->indel_taboo_length = 7;
    p->indel_taboo = 0.1;
    p->min_aln_length = 50;
    p->max_ins_length = 0;
    p->fallback_phred = 1;
    p->phred_offset = 33;
    p->ref_phred_offset = 33;
    p->use_ref_qual = 1;
    p->qual_weighted = 0;
    p->detect_chimera = 0;
    p->invert_scores = 0;
}

static int validate_batch(const pr_cns_batch *b) {
    if (!b || b->n_lr < 0) return set_error(PR_ERR_ARG, "null batch");
    if (b->n_lr == 0) return 0;
    if (!b->lr_off || !b->aln_off) return set_error(PR_ERR_ARG, "lr_off/aln_off required");
    if (b->lr_off[0] != 0 || b->aln_off[0] != 0) return set_error(PR_ERR_ARG, "offsets must start at 0");
    for (int i = 0; i < b->n_lr; ++i) {
        if (b->lr_off[i + 1] < b->lr_off[i] || b->aln_off[i + 1] < b->aln_off[i])
            return set_error(PR_ERR_ARG, "offsets not monotone at %d", i);
        if (b->ign_off && b->ign_off[i + 1] < b->ign_off[i]) return set_error(PR_ERR_ARG, "ign_off not monotone");
    }
    const int64_t na = b->aln_off[b->n_lr];
    if (na && (!b->aln_pos || !b->aln_score || !b->aln_flags || !b->aln_seq_off || !b->aln_lseq ||
               !b->aln_cig_off || !b->aln_ncig || !b->cig_pool))
        return set_error(PR_ERR_ARG, "alignment arrays required");
    for (int64_t a = 0; a < na; ++a) {
        if (b->aln_cig_off[a] < 0 || b->aln_ncig[a] < 0 || b->aln_cig_off[a] + b->aln_ncig[a] > b->cig_pool_len)
            return set_error(PR_ERR_ARG, "cigar out of pool at alignment %lld", (long long)a);
        if (!(b->aln_flags[a] & PR_ALN_NO_SEQ) &&
            (b->aln_seq_off[a] < 0 || b->aln_lseq[a] < 0 || b->aln_seq_off[a] + b->aln_lseq[a] > b->seq_pool_len))
            return set_error(PR_ERR_ARG, "seq out of pool at alignment %lld", (long long)a);
    }
    return 0;
}

// Output capacities per long read (shared by pr_cns_bounds_of and the upload):
// consensus bytes <= L + inserted bases of all its alignments (+1); chimera
// records: cnsp::chim_records.
static void cns_caps(const pr_cns_batch *b, std::vector<int64_t> &out_off, std::vector<int64_t> &chim_off,
                     int64_t *in_bytes, int64_t *k_need = nullptr) {
    const int n = b->n_lr;
    out_off.assign(n + 1, 0);
    chim_off.assign(n + 1, 0);
    int64_t ib = 0, kmax = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t L = b->lr_off[i + 1] - b->lr_off[i];
        int64_t ins = 0;
        for (int64_t a = b->aln_off[i]; a < b->aln_off[i + 1]; ++a) {
            ib += (b->aln_flags[a] & PR_ALN_NO_SEQ ? 0 : b->aln_lseq[a]) + 4 * (int64_t)b->aln_ncig[a] + 16;
            for (int k = 0; k < b->aln_ncig[a]; ++k) {
                const uint32_t cc = b->cig_pool[b->aln_cig_off[a] + k];
                if ((cc & 15u) == 1u) ins += cc >> 4;
            }
        }
        if (b->aln_off[i + 1] - b->aln_off[i] > kmax) kmax = b->aln_off[i + 1] - b->aln_off[i];
        out_off[i + 1] = out_off[i] + L + ins + 1;
        chim_off[i + 1] = chim_off[i] + cnsp::chim_records(L);
    }
    if (in_bytes) *in_bytes = ib;
    if (k_need) *k_need = kmax;
}

extern "C" int pr_cns_bounds_of(const pr_cns_batch *b, pr_cns_bounds *out) {
    int rc = validate_batch(b);
    if (rc) return rc;
    std::vector<int64_t> oo, co;
    cns_caps(b, oo, co, nullptr);
    out->seq_cap = oo.back();
    out->chim_cap = co.back();
    return 0;
}

// the long-read part of a resident consensus batch: lengths, reference, qualities, MCR ranges
int cns_upload_long_reads(pr_ctx *c, const pr_cns_batch *b) {
    c->cns_launched = false;
    c->iter_masked = false;
    c->own = false;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int n = b->n_lr;
    const int64_t tl = n ? b->lr_off[n] : 0;
    c->n_lr = n;
    c->total_cols = tl;
    c->pipe = false;
    if (n) c->lr_off_host.assign(b->lr_off, b->lr_off + n + 1);
    else c->lr_off_host.assign(1, 0);
    c->has_ref = b->ref_seq != nullptr;
    c->has_qual = b->ref_qual != nullptr;
    c->has_ign = b->ign_off != nullptr;
    int rc;
    DevBuf *B = c->cb;
    if ((rc = upload(B[CB_LR_OFF], c->lr_off_host.data(), n + 1, s))) return rc;
    if ((rc = upload(B[CB_REF_SEQ], b->ref_seq, b->ref_seq ? tl : 0, s))) return rc;
    if ((rc = upload(B[CB_REF_QUAL], b->ref_qual, b->ref_qual ? tl : 0, s))) return rc;
    if (b->ign_off) {
        if ((rc = upload(B[CB_IGN_OFF], b->ign_off, n + 1, s))) return rc;
        if ((rc = upload(B[CB_IGN], b->ign, 2 * b->ign_off[n], s))) return rc;
    }
    return 0;
}

extern "C" int pr_cns_upload(pr_ctx *c, const pr_cns_batch *b) {
    if (!c) return set_error(PR_ERR_ARG, "null ctx");
    int rc = validate_batch(b);
    if (rc) return rc;
    if ((rc = cns_upload_long_reads(c, b))) return rc;
    hipStream_t s = c->stream;
    const int n = b->n_lr;
    const int64_t na = n ? b->aln_off[n] : 0;
    const int64_t tl = c->total_cols;
    c->n_aln = na;
    int64_t in_bytes = 0;
    cns_caps(b, c->out_off, c->chim_off, &in_bytes, &c->k_need);
    c->seq_cap = c->out_off[n];
    c->chim_cap = c->chim_off[n];
    // SURVEY.md §8d pileup byte model: alignments in + ref seq/qual in + consensus out + state counts
    c->alg_bytes = in_bytes + tl * 2 + tl * 2 + tl * 6 * 4 * 2;

    DevBuf *B = c->cb;
    c->aln_off_host.assign(b->aln_off, b->aln_off + (n ? n + 1 : 0));
    if ((rc = upload(B[CB_ALN_OFF], b->aln_off, n + 1, s))) return rc;
    if ((rc = upload(B[CB_POS], b->aln_pos, na, s))) return rc;
    if ((rc = upload(B[CB_SCORE], b->aln_score, na, s))) return rc;
    if ((rc = upload(B[CB_AFLAGS], b->aln_flags, na, s))) return rc;
    if ((rc = upload(B[CB_SEQ_OFF], b->aln_seq_off, na, s))) return rc;
    if ((rc = upload(B[CB_LSEQ], b->aln_lseq, na, s))) return rc;
    if ((rc = upload(B[CB_CIG_OFF], b->aln_cig_off, na, s))) return rc;
    if ((rc = upload(B[CB_NCIG], b->aln_ncig, na, s))) return rc;
    if ((rc = upload(B[CB_SEQ], b->seq_pool, b->seq_pool_len, s))) return rc;
    if ((rc = upload(B[CB_CIG], b->cig_pool, b->cig_pool_len, s))) return rc;
    return cns_alloc_resident(c);
}

// the buffers of `groups` (a cnsp::Group mask) sized for the resident batch's counts
int cns_ensure(pr_ctx *c, unsigned groups) {
    const cnsp::Sizes z = {c->n_lr, c->n_aln, c->seq_cap, c->chim_cap};
    for (const cnsp::Entry &e : cnsp::TABLE) {
        int rc;
        if ((e.group & groups) && (rc = c->cb[e.id].ensure(cnsp::bytes(e, z)))) return rc;
    }
    return 0;
}

// scratch and output buffers of the resident batch (c->n_lr, n_aln, out_off, chim_off, seq_cap, chim_cap
// set), then the batch counts as loaded
int cns_alloc_resident(pr_ctx *c) {
    hipStream_t s = c->stream;
    DevBuf *B = c->cb;
    const int n = c->n_lr;
    int rc;
    if ((rc = cns_ensure(c, cnsp::ALN_SCRATCH | cnsp::READ_OUT))) return rc;
    if ((rc = upload(B[CB_OUT_OFF], c->out_off.data(), n + 1, s))) return rc;
    if ((rc = upload(B[CB_CHIM_OFF], c->chim_off.data(), n + 1, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    c->cns_loaded = true;
    return 0;
}

extern "C" int pr_cns_launch(pr_ctx *c, const pr_cns_params *p) {
    if (!c || !p) return set_error(PR_ERR_ARG, "null arg");
    if (!c->cns_loaded) return set_error(PR_ERR_ARG, "no resident consensus batch (pr_cns_upload first)");
    if (p->qual_weighted)
        return set_error(PR_ERR_UNSUPPORTED, "--qual-weighted (ccseq/utg modes) is not implemented on the GPU path");
    if (!(p->bin_size >= 1.0)) return set_error(PR_ERR_ARG, "bin_size must be >= 1");
    // a chimera candidate compares up to 6 bins of columns (4 low bins and one on either side)
    // in LDS tables of CHIM_MAXCOLS columns
    if (p->detect_chimera && 6.0 * (double)(long)p->bin_size > (double)CHIM_MAXCOLS)
        return set_error(PR_ERR_CAPACITY, "detect_chimera needs bin_size <= %d (got %g)", CHIM_MAXCOLS / 6, p->bin_size);
    HIPCHK(hipSetDevice(c->device));
    CnsParamsDev P;
    P.max_coverage = p->max_coverage;
    P.bin_size = p->bin_size;
    P.bin_max_bases = p->bin_size * p->max_coverage;   // Seq.pm:517
    P.indel_taboo = p->indel_taboo;
    P.trim = p->trim;
    P.indel_taboo_length = p->indel_taboo_length;
    P.min_aln_length = p->min_aln_length;
    P.max_ins_length = p->max_ins_length;
    P.fallback_phred = p->fallback_phred;
    P.phred_offset = p->phred_offset;
    P.ref_phred_offset = p->ref_phred_offset;
    P.use_ref_qual = p->use_ref_qual;
    P.detect_chimera = p->detect_chimera;
    P.invert_scores = p->invert_scores;
    DevBuf *B = c->cb;
    CnsDev D;
    std::memset(&D, 0, sizeof D);
    D.n_lr = c->n_lr;
    D.n_aln = c->n_aln;
    D.lr_off = B[CB_LR_OFF].as<int64_t>();
    D.ref_seq = c->has_ref ? B[CB_REF_SEQ].as<uint8_t>() : nullptr;
    D.ref_qual = c->has_qual ? B[CB_REF_QUAL].as<uint8_t>() : nullptr;
    D.ign_off = c->has_ign ? B[CB_IGN_OFF].as<int64_t>() : nullptr;
    D.ign = c->has_ign ? B[CB_IGN].as<int32_t>() : nullptr;
    D.aln_off = B[CB_ALN_OFF].as<int64_t>();
    D.pos = B[CB_POS].as<int32_t>();
    D.score = B[CB_SCORE].as<double>();
    D.aflags = B[CB_AFLAGS].as<uint8_t>();
    D.seq_off = B[CB_SEQ_OFF].as<int64_t>();
    D.lseq = B[CB_LSEQ].as<int32_t>();
    D.cig_off = B[CB_CIG_OFF].as<int64_t>();
    D.ncig = B[CB_NCIG].as<int32_t>();
    D.seq = B[CB_SEQ].as<uint8_t>();
    D.cig = B[CB_CIG].as<uint32_t>();
    D.a_st = B[CB_A_ST].as<uint32_t>();
    D.a_len = B[CB_A_LEN].as<int32_t>();
    D.a_nc = B[CB_A_NC].as<double>();
    D.a_bin = B[CB_A_BIN].as<int32_t>();
    D.a_cb = B[CB_A_CB].as<int32_t>();
    D.a_ce = B[CB_A_CE].as<int32_t>();
    D.a_sb = B[CB_A_SB].as<int32_t>();
    D.a_rpos = B[CB_A_RPOS].as<int32_t>();
    D.a_end = B[CB_A_END].as<int32_t>();
    D.sorted = B[CB_SORTED].as<int32_t>();
    D.lst_score = B[CB_LST_SCORE].as<double>();
    D.lst_aln = B[CB_LST_ALN].as<int32_t>();
    D.kept = B[CB_KEPT].as<uint8_t>();
    D.bin_off = B[CB_BIN_OFF].as<int64_t>();
    D.bin_bases = B[CB_BIN_BASES].as<int64_t>();
    D.work = B[CB_WORK].as<int32_t>();
    // per-phase clock counters (thread 0 reads the wall clock at every phase boundary): off by
    // default, PRGPU_CNS_PROF=1 turns them on (bench.py: one extra untimed step)
    {
        const char *pe = getenv("PRGPU_CNS_PROF");
        D.prof = (pe && atoi(pe) != 0) ? B[CB_PROF].as<unsigned long long>() : nullptr;
    }
    D.out_off = B[CB_OUT_OFF].as<int64_t>();
    D.chim_off = B[CB_CHIM_OFF].as<int64_t>();
    D.status = B[CB_STATUS].as<int32_t>();
    D.seq_len = B[CB_SEQ_LEN].as<int32_t>();
    D.trace_len = B[CB_TRACE_LEN].as<int32_t>();
    D.ncigar = B[CB_NCIGAR].as<int32_t>();
    D.nchim = B[CB_NCHIM].as<int32_t>();
    D.o_seq = B[CB_O_SEQ].as<uint8_t>();
    D.o_qual = B[CB_O_QUAL].as<uint8_t>();
    D.o_trace = B[CB_O_TRACE].as<uint8_t>();
    D.o_cig = B[CB_O_CIG].as<uint32_t>();
    D.o_chim = B[CB_O_CHIM].as<int32_t>();
    if (c->n_lr == 0) {
        c->cns_launched = true;
        return 0;
    }
    {
        // bins per read with this bin size (Seq.pm:1437-1444 _init_read_bins)
        const std::vector<int64_t> &lr = c->lr_off_host;
        c->bin_off.assign(c->n_lr + 1, 0);
        for (int i = 0; i < c->n_lr; ++i)
            c->bin_off[i + 1] = c->bin_off[i] + (int64_t)((double)(lr[i + 1] - lr[i]) / p->bin_size) + 1;
        int rc;
        if ((rc = upload(B[CB_BIN_OFF], c->bin_off.data(), c->n_lr + 1, c->stream))) return rc;
        if ((rc = B[CB_BIN_BASES].ensure((size_t)(c->bin_off[c->n_lr] + 1) * 8))) return rc;
        D.bin_off = B[CB_BIN_OFF].as<int64_t>();
        D.bin_bases = B[CB_BIN_BASES].as<int64_t>();
    }
    if (c->pipe && c->own) {
        // owned batch: short reads (nt4, global ids) from the task's pool, CIGARs in place in
        // the received wire pool, the ASCII consensus reference of the owned reads
        D.ref_seq = B[CB_REF_SEQ].as<uint8_t>();
        D.ref_nt4 = c->own_ref_nt4 ? 1 : 0;
        D.seq = c->own_sr_resident ? c->ls[c->ss_samp_off.empty() ? LS_SRSEQ : LS_SRSAMP].as<uint8_t>()
                                   : c->xb[XB_SR].as<uint8_t>();
        D.seq_nt4 = 1;
        D.cig = c->xb[XB_RCIG].as<uint32_t>();
        if (c->x_pass) {   // world 1: CIGARs in place in the SW output pool
            SwPtrs sp;
            int rc = sw_get_ptrs(c, &sp);
            if (rc) return rc;
            D.cig = sp.cig;
        }
    } else if (c->pipe) {
        // consensus reads the SW batch in place: long reads and short reads as
        // nt4, CIGARs in place in the SW output pool (per-task starts: pipe hand-off)
        SwPtrs sp;
        int rc = sw_get_ptrs(c, &sp);
        if (rc) return rc;
        if (c->pipe_ref_ascii) {   // bam2cns --ref differs from the mapping reference (masked HCRs)
            D.ref_seq = B[CB_REF_SEQ].as<uint8_t>();
            D.ref_nt4 = 0;
        } else {
            D.ref_seq = sp.lr;
            D.ref_nt4 = 1;
        }
        D.seq = sp.sr;
        D.seq_nt4 = 1;
        D.cig = sp.cig;
    }
    if (c->pipe && c->cns_gathered) {   // a second launch on the same hand-off: already in place
        D.seq = B[CB_SEQ].as<uint8_t>();
        D.cig = B[CB_CIG].as<uint32_t>();
    } else if (c->pipe && c->n_aln > 0 && !getenv("PRGPU_CNS_NOGATHER")) {
        // the alignments' SEQ bytes and CIGAR ops in consensus order (pipe_kernels.hip cns_gather):
        // into the standalone path's SEQ / CIGAR pools, which a pipe batch does not use
        const int64_t na = c->n_aln;
        const int64_t *tot = D.aln_off + c->n_lr;
        const size_t tb = cns_gather_temp_bytes(na);
        int rc;
        if ((rc = B[CB_GSZS].ensure((size_t)(na + 1) * 8)) || (rc = B[CB_GSZC].ensure((size_t)(na + 1) * 8)) ||
            (rc = B[CB_GSO].ensure((size_t)(na + 1) * 8)) || (rc = B[CB_GCO].ensure((size_t)(na + 1) * 8)) ||
            (rc = B[CB_GTMP].ensure(tb)))
            return rc;
        int e = cns_gather_offsets(tot, na, D.lseq, D.ncig, B[CB_GSZS].as<int64_t>(), B[CB_GSZC].as<int64_t>(),
                                   B[CB_GSO].as<int64_t>(), B[CB_GCO].as<int64_t>(), B[CB_GTMP].p, tb, (void *)c->stream);
        if (e) return set_error(PR_ERR_HIP, "consensus gather: %s", hipGetErrorString((hipError_t)e));
        int64_t tot_seq = 0, tot_cig = 0;
        HIPCHK(hipMemcpyAsync(&tot_seq, B[CB_GSO].as<int64_t>() + na, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(&tot_cig, B[CB_GCO].as<int64_t>() + na, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if ((rc = B[CB_SEQ].ensure((size_t)tot_seq + 16)) || (rc = B[CB_CIG].ensure((size_t)tot_cig * 4 + 16))) return rc;
        e = cns_gather_copy(tot, na, D.seq, D.cig, B[CB_SEQ_OFF].as<int64_t>(), D.lseq, B[CB_CIG_OFF].as<int64_t>(), D.ncig,
                            B[CB_GSO].as<int64_t>(),
                            B[CB_GCO].as<int64_t>(), B[CB_SEQ].as<uint8_t>(), B[CB_CIG].as<uint32_t>(), (void *)c->stream);
        if (e) return set_error(PR_ERR_HIP, "consensus gather: %s", hipGetErrorString((hipError_t)e));
        D.seq = B[CB_SEQ].as<uint8_t>();
        D.cig = B[CB_CIG].as<uint32_t>();
        c->cns_gathered = true;   // (the offsets now point into the gathered pools)
    }
    HIPCHK(hipMemsetAsync(D.work, 0, 64, c->stream));
    HIPCHK(hipMemsetAsync(B[CB_PROF].as<unsigned long long>(), 0, CNS_NPHASE * 8, c->stream));
    const int wgcu = cns_wg_per_cu();
    const int grid = c->n_lr < c->n_cu * wgcu ? c->n_lr : c->n_cu * wgcu;
    const int grid_retry = c->n_lr < c->n_cu ? c->n_lr : c->n_cu;
    {
        // K pool: per resident workgroup the window starts (longest read / 256 + 8 ints) and
        // 12 ints per kept alignment
        int64_t lmax = 0;
        for (int i = 0; i < c->n_lr; ++i) lmax = std::max(lmax, c->lr_off_host[i + 1] - c->lr_off_host[i]);
        const int64_t kc = ((lmax / 256 + 12) + 12 * (c->k_need < 64 ? 64 : c->k_need) + 3) & ~(int64_t)3;   // 16-byte entries
        int rc;
        if ((rc = B[CB_K].ensure((size_t)grid * kc * 4))) return rc;
        D.k_pool = B[CB_K].as<int32_t>();
        D.k_cap = kc;
        D.retry = B[CB_RETRY].as<int32_t>();
        D.retry_n = B[CB_RETRY].as<int32_t>() + c->n_lr + 8;
        HIPCHK(hipMemsetAsync(D.retry_n, 0, 4, c->stream));
        D.debug = getenv("PRGPU_CNS_DEBUG") ? atoi(getenv("PRGPU_CNS_DEBUG")) : 0;
        const char *fl = getenv("PRGPU_CNS_LARGE");   // diagnostics: all reads through the large geometry
        if (fl && atoi(fl)) {
            D.force_large = 1;
            std::vector<int32_t> all((size_t)c->n_lr + 1);
            for (int i = 0; i < c->n_lr; ++i) all[(size_t)i] = i;
            all[(size_t)c->n_lr] = c->n_lr;
            HIPCHK(hipMemcpyAsync(D.retry, all.data(), (size_t)c->n_lr * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(D.retry_n, &all[(size_t)c->n_lr], 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    HIPCHK(hipEventRecord(c->ev[4], c->stream));
    int e = cns_launch(D, P, grid, grid_retry, (void *)c->stream);
    if (e != 0) return set_error(PR_ERR_HIP, "cns kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    HIPCHK(hipEventRecord(c->ev[5], c->stream));
    c->cns_launched = true;
    return 0;
}

extern "C" int pr_cns_download(pr_ctx *c, pr_cns_out *o) {
    if (!c || !o) return set_error(PR_ERR_ARG, "null arg");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    float ms = 0.f;
    if (c->n_lr && hipEventElapsedTime(&ms, c->ev[4], c->ev[5]) == hipSuccess) c->last_ms = ms;
    if (c->pipe && c->n_lr && hipEventElapsedTime(&ms, c->ev[0], c->ev[4]) == hipSuccess) c->ms_pipe = ms;
    const int n = c->n_lr;
    DevBuf *B = c->cb;
    int rc;
    if (o->out_off) std::memcpy(o->out_off, c->out_off.data(), (n + 1) * sizeof(int64_t));
    if (o->chim_off) std::memcpy(o->chim_off, c->chim_off.data(), (n + 1) * sizeof(int64_t));
    if ((rc = download(o->status, B[CB_STATUS], n, s)) || (rc = download(o->seq_len, B[CB_SEQ_LEN], n, s)) ||
        (rc = download(o->trace_len, B[CB_TRACE_LEN], n, s)) || (rc = download(o->ncigar, B[CB_NCIGAR], n, s)) ||
        (rc = download(o->nchim, B[CB_NCHIM], n, s)) || (rc = download(o->seq, B[CB_O_SEQ], c->seq_cap, s)) ||
        (rc = download(o->qual, B[CB_O_QUAL], c->seq_cap, s)) ||
        (rc = download(o->trace, B[CB_O_TRACE], c->seq_cap, s)) ||
        (rc = download(o->cigar, B[CB_O_CIG], c->seq_cap, s)) ||
        (rc = download(o->chim, B[CB_O_CHIM], c->chim_cap * 4, s)) ||
        (rc = download(o->kept, B[CB_KEPT], c->n_aln, s)))
        return rc;
    if (o->bin_bases && c->bin_off.size() == (size_t)n + 1)
        if ((rc = download(o->bin_bases, B[CB_BIN_BASES], c->bin_off[n], s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int pr_cns_run(pr_ctx *c, const pr_cns_params *p, const pr_cns_batch *b, pr_cns_out *o) {
    int rc = pr_cns_upload(c, b);
    if (rc) return rc;
    if ((rc = pr_cns_launch(c, p))) return rc;
    return pr_cns_download(c, o);
}

extern "C" int pr_cns_last_timing(pr_ctx *c, double *ms_prep, double *ms_pileup) {
    if (!c) return set_error(PR_ERR_ARG, "null ctx");
    if (ms_prep) *ms_prep = 0.0;
    if (ms_pileup) *ms_pileup = c->last_ms;
    return 0;
}

extern "C" int pr_cns_phase_ticks(pr_ctx *c, uint64_t *ticks, int n) {
    if (!c || !ticks || n < 8) return set_error(PR_ERR_ARG, "need ctx and >= 8 ticks");
    if (!c->cns_loaded || !c->cb[CB_PROF].p) return set_error(PR_ERR_ARG, "no consensus launch yet");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(ticks, c->cb[CB_PROF].p, (size_t)(n < CNS_NPHASE ? n : CNS_NPHASE) * 8, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pr_cns_resident_stats(pr_ctx *c, int64_t *columns, int64_t *alg_bytes) {
    if (!c) return set_error(PR_ERR_ARG, "null ctx");
    if (columns) *columns = c->total_cols;
    if (alg_bytes) *alg_bytes = c->alg_bytes;
    return 0;
}


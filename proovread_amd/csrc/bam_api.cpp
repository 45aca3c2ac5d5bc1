// The device BAM decoder's entries of the C-ABI (include/prgpu.h): pr_bam_decode_alns_gpu (the
// decoder alone, downloaded, to compare with pr_bam_decode_alns), pr_cns_upload_bam (a record
// stream decoded and grouped per long read into the resident consensus batch) and what a driver
// needs of that batch (pr_cns_resident_bounds, pr_cns_resident_aln_count, pr_bam_decode_last_ms).
// The two _opts entries take PR_BAM_RESTORE_SEQ: the donor table, the lookup and the restoring
// unpack run as well, and the host formats a refusal's message from the record index it gets back.
//
// The host's share: one pre-pass over the records' sizes (the offsets the kernels index by, and
// the three size errors of bam_codec.cpp:491-500), the scans over reference ids and long reads
// (a few thousand entries) between the passes, and Perl's numification of AS:Z scores.
//
// And the encoder's (bam_enc_kernels.hip): pr_iter_export_bam, pr_iter_export_bam_bytes and
// pr_bam_export_last_ms -- the refusals, the upload of the names and qualities, the passes over
// the resident hand-off, the download of the record stream.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "bam_core.h"
#include "bam_dev.h"
#include "bam_enc_core.h"
#include "bam_enc_dev.h"

using namespace prgpu::bam;

namespace {

enum { T_RECS, T_OFF, T_FSCORE, T_FFLAGS, T_FKEEP, T_CNT, T_ERR, T_TEXT, T_KIDX, T_REF2LR, T_REFSTART, T_DELTA,
       T_SCAN, T_SRC, T_INS, T_TAB, T_RST, T_SEQSRC, T_HL, T_RC, T_COUNT };

struct Temps {
    DevBuf b[T_COUNT];
    hipEvent_t ev[6] = {};
    Temps() {
        for (int i = 0; i < T_COUNT; ++i) b[i].grp = "bam", b[i].id = i;
    }
    ~Temps() {
        for (auto &x : b) x.release();
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// where the decoded columns go (the resident consensus buffers, or buffers of a plain decode)
struct Columns {
    DevBuf *rid, *pos, *score, *flags, *seq_off, *lseq, *cig_off, *ncig, *seq, *qual, *cig;
};

struct Decoded {
    int64_t n = 0, n_kept = 0, seq_len = 0, cig_len = 0;
    std::vector<int64_t> lr_count, lr_ins;   // per long read: alignments, inserted bases of their CIGARs
};

int scan_records(const uint8_t *recs, int64_t len, std::vector<int64_t> &off) {
    for (int64_t o = 0; o < len;) {
        int64_t next = 0;
        const int e = bam_check_record(recs, len, o, &next);
        if (e) return pr_set_error(PR_ERR_ARG, bam_error_text(e));
        off.push_back(o);
        o = next;
    }
    if (off.size() >= ((size_t)1 << 31)) return pr_set_error(PR_ERR_CAPACITY, "more than 2^31 - 1 BAM records in one stream");
    return 0;
}

// the QNAME of record i for a message (at most 64 bytes of it)
std::string qname_of(const uint8_t *recs, const std::vector<int64_t> &off, unsigned long long i) {
    const uint8_t *rec = recs + off[(size_t)i];
    const size_t l = rec[12] ? (size_t)rec[12] - 1 : 0;
    std::string s((const char *)bam_name_at(rec), l < 64 ? l : 64);
    if (l > 64) s += "...";
    return s;
}

// The passes of bam_kernels.hip over a record stream.  ref_to_lr NULL: every record is kept, in
// file order; otherwise the kept records come out grouped by long read (n_lr of them).
// flags & PR_BAM_RESTORE_SEQ: a kept record without SEQ takes it from its donor (bam_core.h);
// *n_restored counts them.
int decode(pr_ctx *c, const uint8_t *recs, int64_t len, const int32_t *ref_to_lr, int32_t n_ref, int32_t n_lr,
           const Columns &O, Decoded &R, uint32_t flags = 0, int64_t *n_restored = nullptr) {
    std::vector<int64_t> off;
    int rc = scan_records(recs, len, off);
    if (rc) return rc;
    const int64_t n = (int64_t)off.size();
    R.n = n;
    const bool restore = (flags & PR_BAM_RESTORE_SEQ) != 0;
    if (n_restored) *n_restored = 0;
    std::vector<int32_t> lr_to_ref;
    if (ref_to_lr) {
        lr_to_ref.assign((size_t)n_lr, -1);
        for (int32_t r = 0; r < n_ref; ++r) {
            const int32_t l = ref_to_lr[r];
            if (l < -1 || l >= n_lr) return set_error(PR_ERR_ARG, "ref_to_lr[%d] = %d is outside [-1, %d)", r, l, n_lr);
            if (l >= 0 && lr_to_ref[(size_t)l] >= 0)
                return set_error(PR_ERR_ARG, "ref_to_lr maps references %d and %d to long read %d", lr_to_ref[(size_t)l], r, l);
            if (l >= 0) lr_to_ref[(size_t)l] = r;
        }
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Temps T;
    for (auto &e : T.ev) HIPCHK(hipEventCreate(&e));
    DevBuf *B = T.b;
    const size_t tb = bam_scan_temp_bytes(n);
    if ((rc = upload(B[T_RECS], recs, (size_t)len, s)) || (rc = upload(B[T_OFF], off.data(), (size_t)n, s)) ||
        (rc = B[T_FSCORE].ensure((size_t)n * 8)) || (rc = B[T_FFLAGS].ensure((size_t)n)) ||
        (rc = B[T_FKEEP].ensure((size_t)(n + 1) * 4)) || (rc = B[T_CNT].ensure((size_t)(n_ref + 1) * 8)) ||
        (rc = B[T_ERR].ensure(8)) || (rc = B[T_TEXT].ensure((size_t)n * 4)) || (rc = B[T_KIDX].ensure((size_t)(n + 1) * 8)) ||
        (rc = B[T_SCAN].ensure(tb)))
        return rc;
    if (ref_to_lr && (rc = upload(B[T_REF2LR], ref_to_lr, (size_t)n_ref, s))) return rc;
    HIPCHK(hipMemsetAsync(B[T_FKEEP].p, 0, (size_t)(n + 1) * 4, s));
    HIPCHK(hipMemsetAsync(B[T_CNT].p, 0, (size_t)(n_ref + 1) * 8, s));
    HIPCHK(hipMemsetAsync(B[T_ERR].p, 0, 8, s));
    BamDev D;
    std::memset(&D, 0, sizeof D);
    D.recs = B[T_RECS].as<uint8_t>();
    D.off = B[T_OFF].as<int64_t>();
    D.n = n;
    D.ref_to_lr = ref_to_lr ? B[T_REF2LR].as<int32_t>() : nullptr;
    D.n_ref = ref_to_lr ? n_ref : 0;
    D.f_score = B[T_FSCORE].as<double>();
    D.f_flags = B[T_FFLAGS].as<uint8_t>();
    D.f_keep = B[T_FKEEP].as<int32_t>();
    D.cnt_ref = B[T_CNT].as<unsigned long long>();
    D.err = B[T_ERR].as<int32_t>();
    D.text_list = B[T_TEXT].as<int32_t>();
    D.kidx = B[T_KIDX].as<int64_t>();
    float ms_donor = 0.f;
    if (restore) {
        // the donor table: a power of two of slots, at least twice the records that may lend a SEQ
        // (counted here from the fixed fields; the kernel also leaves out those with an H op)
        int64_t eligible = 0;
        for (int64_t i = 0; i < n; ++i) {
            const uint8_t *rec = recs + off[(size_t)i];
            eligible += bam_fixed(rec).l_seq > 0 && !(bam_flag(rec) & BAM_DONOR_EXCLUDED);
        }
        const int64_t slots = bam_table_slots(eligible);
        if ((rc = B[T_TAB].ensure((size_t)slots * 8)) || (rc = B[T_RST].ensure(24))) return rc;
        HIPCHK(hipMemsetAsync(B[T_TAB].p, 0xFF, (size_t)slots * 8, s));
        HIPCHK(hipMemsetAsync(B[T_RST].p, 0xFF, 16, s));
        HIPCHK(hipMemsetAsync((uint8_t *)B[T_RST].p + 16, 0, 8, s));
        D.tab = B[T_TAB].as<unsigned long long>();
        D.tab_mask = slots - 1;
        D.rst = B[T_RST].as<unsigned long long>();
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HIPCHK(hipEventCreate(&e0));
        hipError_t he = hipEventCreate(&e1);
        if (he == hipSuccess) he = hipEventRecord(e0, s);
        if (he == hipSuccess) he = (hipError_t)bam_donor_pass(D, s);
        if (he == hipSuccess) he = hipEventRecord(e1, s);
        if (he == hipSuccess) he = hipEventSynchronize(e1);
        if (he == hipSuccess) (void)hipEventElapsedTime(&ms_donor, e0, e1);
        (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        HIPCHK(he);
    }

    // field pass + the kept records' indices
    HIPCHK(hipEventRecord(T.ev[0], s));
    HIPCHK((hipError_t)bam_field_pass(D, B[T_KIDX].as<int64_t>(), B[T_SCAN].p, tb, s));
    HIPCHK(hipEventRecord(T.ev[1], s));
    int32_t err[2] = {0, 0};
    int64_t n_kept = 0;
    std::vector<int64_t> cnt((size_t)n_ref + 1, 0);
    HIPCHK(hipMemcpyAsync(err, B[T_ERR].p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&n_kept, B[T_KIDX].as<int64_t>() + n, 8, hipMemcpyDeviceToHost, s));
    if (ref_to_lr && n_ref) HIPCHK(hipMemcpyAsync(cnt.data(), B[T_CNT].p, (size_t)n_ref * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (err[0] & BAM_E_AUX) return pr_set_error(PR_ERR_SAM, bam_error_text(BAM_BAD_AUX));
    if (err[0] & BAM_E_RID) return set_error(PR_ERR_ARG, "BAM record with reference id outside [-1, %d)", n_ref);
    R.n_kept = n_kept;

    // the kept records of a reference move from the histogram's block to their long read's columns
    std::vector<int64_t> ref_start((size_t)n_ref + 1, 0), delta((size_t)n_ref + 1, 0);   // (alive until the last sync)
    if (ref_to_lr) {
        for (int32_t r = 0; r < n_ref; ++r) ref_start[(size_t)r + 1] = ref_start[(size_t)r] + cnt[(size_t)r];
        R.lr_count.assign((size_t)n_lr, 0);
        int64_t at = 0;
        for (int32_t l = 0; l < n_lr; ++l) {
            const int32_t r = lr_to_ref[(size_t)l];
            if (r < 0) continue;
            R.lr_count[(size_t)l] = cnt[(size_t)r];
            delta[(size_t)r] = at - ref_start[(size_t)r];
            at += cnt[(size_t)r];
        }
        if ((rc = upload(B[T_REFSTART], ref_start.data(), ref_start.size(), s)) ||
            (rc = upload(B[T_DELTA], delta.data(), delta.size(), s)) || (rc = B[T_INS].ensure((size_t)(n_lr + 1) * 8)))
            return rc;
        HIPCHK(hipMemsetAsync(B[T_INS].p, 0, (size_t)(n_lr + 1) * 8, s));
        D.ref_start = B[T_REFSTART].as<int64_t>();
        D.delta = B[T_DELTA].as<int64_t>();
        D.ins = B[T_INS].as<unsigned long long>();
    }
    const size_t k1 = (size_t)n_kept + 1;
    if ((O.rid && (rc = O.rid->ensure(k1 * 4))) || (rc = O.pos->ensure(k1 * 4)) || (rc = O.score->ensure(k1 * 8)) ||
        (rc = O.flags->ensure(k1)) || (rc = O.seq_off->ensure(k1 * 8)) || (rc = O.lseq->ensure(k1 * 4)) ||
        (rc = O.cig_off->ensure(k1 * 8)) || (rc = O.ncig->ensure(k1 * 4)) || (rc = B[T_SRC].ensure(k1 * 8)))
        return rc;
    if (restore) {
        if ((rc = B[T_SEQSRC].ensure(k1 * 8)) || (rc = B[T_HL].ensure(k1 * 4)) || (rc = B[T_RC].ensure(k1))) return rc;
        D.a_seq_src = B[T_SEQSRC].as<int64_t>();
        D.a_hl = B[T_HL].as<int32_t>();
        D.a_rc = B[T_RC].as<uint8_t>();
    }
    HIPCHK(hipMemsetAsync(O.lseq->p, 0, k1 * 4, s));
    HIPCHK(hipMemsetAsync(O.ncig->p, 0, k1 * 4, s));
    HIPCHK(hipMemsetAsync(B[T_SRC].p, 0, k1 * 8, s));
    D.n_kept = n_kept;
    D.a_rid = O.rid ? O.rid->as<int32_t>() : nullptr;
    D.a_pos = O.pos->as<int32_t>();
    D.a_score = O.score->as<double>();
    D.a_flags = O.flags->as<uint8_t>();
    D.a_lseq = O.lseq->as<int32_t>();
    D.a_ncig = O.ncig->as<int32_t>();
    D.a_src = B[T_SRC].as<int64_t>();
    D.seq_off = O.seq_off->as<int64_t>();
    D.cig_off = O.cig_off->as<int64_t>();
    HIPCHK(hipEventRecord(T.ev[2], s));
    if (restore)
        HIPCHK((hipError_t)bam_place_restore_pass(D, O.seq_off->as<int64_t>(), O.cig_off->as<int64_t>(), B[T_SCAN].p, tb, s));
    else
        HIPCHK((hipError_t)bam_place_pass(D, O.seq_off->as<int64_t>(), O.cig_off->as<int64_t>(), B[T_SCAN].p, tb, s));
    HIPCHK(hipEventRecord(T.ev[3], s));
    HIPCHK(hipMemcpyAsync(err, B[T_ERR].p, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&R.seq_len, O.seq_off->as<int64_t>() + n_kept, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&R.cig_len, O.cig_off->as<int64_t>() + n_kept, 8, hipMemcpyDeviceToHost, s));
    unsigned long long rst[3] = {0, 0, 0};
    if (restore) HIPCHK(hipMemcpyAsync(rst, B[T_RST].p, 24, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (err[0] & BAM_E_ORDER) return pr_set_error(PR_ERR_ARG, "BAM records are not coordinate-sorted");
    if (restore) {
        // (the placement's BAM_E_NOSEQ is what the lookup answers; the lower record index speaks first)
        const bool nd = (err[0] & BAM_E_NODONOR) != 0, dl = (err[0] & BAM_E_DONORLEN) != 0;
        if (nd && (!dl || rst[0] < rst[1]))
            return set_error(PR_ERR_NOSEQ, "Cannot restore SEQ of BAM record %llu (%s): no primary record with SEQ and "
                             "without hard clips under its name", rst[0], qname_of(recs, off, rst[0]).c_str());
        if (dl)
            return set_error(PR_ERR_SAM, "Cannot restore SEQ of BAM record %llu (%s): its CIGAR does not span its "
                             "primary record's SEQ", rst[1], qname_of(recs, off, rst[1]).c_str());
        if (n_restored) *n_restored = (int64_t)rst[2];
    } else if (err[0] & BAM_E_NOSEQ) {
        return pr_set_error(PR_ERR_NOSEQ, "Cannot handle BAM secondary alignments without seq/qual");
    }

    // SEQ, QUAL and CIGAR ops into the pools
    if ((rc = O.seq->ensure((size_t)R.seq_len + 16)) || (O.qual && (rc = O.qual->ensure((size_t)R.seq_len + 16))) ||
        (rc = O.cig->ensure((size_t)R.cig_len * 4 + 16)))
        return rc;
    D.seq = O.seq->as<uint8_t>();
    D.qual = O.qual ? O.qual->as<uint8_t>() : nullptr;
    D.cig = O.cig->as<uint32_t>();
    HIPCHK(hipEventRecord(T.ev[4], s));
    HIPCHK((hipError_t)(restore ? bam_unpack_restore_pass(D, s) : bam_unpack_pass(D, s)));
    HIPCHK(hipEventRecord(T.ev[5], s));

    // AS:Z / AS:H scores: Perl's number of the text, into the score column
    if (err[1] > 0) {
        std::vector<int32_t> list((size_t)err[1]);
        HIPCHK(hipMemcpyAsync(list.data(), B[T_TEXT].p, list.size() * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int32_t i : list) {
            const uint8_t *rec = recs + off[(size_t)i];
            const Fixed f = bam_fixed(rec);
            double sc = 0.0;
            uint32_t fl = 0;
            int32_t text = 0;
            (void)bam_aux_walk(bam_aux_at(rec, f), bam_end_of(rec, f), &sc, &fl, &text);
            const char *t0 = (const char *)bam_aux_at(rec, f) + text;
            sc = bam_perl_number(t0, t0 + std::strlen(t0));
            int64_t d = i;
            if (ref_to_lr) {
                if (f.rid < 0 || ref_to_lr[f.rid] < 0) continue;   // a dropped record
                HIPCHK(hipMemcpyAsync(&d, B[T_KIDX].as<int64_t>() + i, 8, hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                d += delta[(size_t)f.rid];
            }
            HIPCHK(hipMemcpyAsync(O.score->as<double>() + d, &sc, 8, hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    }
    if (ref_to_lr) {
        R.lr_ins.assign((size_t)n_lr + 1, 0);
        HIPCHK(hipMemcpyAsync(R.lr_ins.data(), B[T_INS].p, (size_t)n_lr * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    c->ms_bam = ms_donor;
    for (int k = 0; k < 6; k += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, T.ev[k], T.ev[k + 1]) == hipSuccess) c->ms_bam += ms;
    }
    return 0;
}

}   // namespace

extern "C" int pr_bam_decode_alns_gpu(pr_ctx *c, const uint8_t *recs, int64_t len, pr_bam_alns *out) {
    return pr_bam_decode_alns_gpu_opts(c, recs, len, 0, out, nullptr);
}

extern "C" int pr_bam_decode_alns_gpu_opts(pr_ctx *c, const uint8_t *recs, int64_t len, uint32_t flags, pr_bam_alns *out,
                                           int64_t *n_restored) {
    if (!c || !out || len < 0 || (len && !recs)) return pr_set_error(PR_ERR_ARG, "null arg");
    if (flags & ~(uint32_t)PR_BAM_RESTORE_SEQ) return set_error(PR_ERR_ARG, "unknown BAM decode flags 0x%x", flags);
    std::memset(out, 0, sizeof *out);
    struct Bufs {
        DevBuf b[11];
        ~Bufs() {
            for (auto &x : b) x.release();
        }
    } U;
    for (int i = 0; i < 11; ++i) U.b[i].grp = "bam", U.b[i].id = 32 + i;
    DevBuf *b = U.b;
    const Columns O = {&b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &b[6], &b[7], &b[8], &b[9], &b[10]};
    Decoded R;
    int rc = decode(c, recs, len, nullptr, 0, 0, O, R, flags, n_restored);
    if (rc) return rc;
    const size_t n = (size_t)R.n_kept;
    auto alloc = [](size_t bytes) { return std::malloc(bytes ? bytes : 1); };
    out->n = R.n_kept;
    out->rid = (int32_t *)alloc(4 * n);
    out->pos1 = (int32_t *)alloc(4 * n);
    out->score = (double *)alloc(8 * n);
    out->flags = (uint8_t *)alloc(n);
    out->seq_off = (int64_t *)alloc(8 * n);
    out->lseq = (int32_t *)alloc(4 * n);
    out->cig_off = (int64_t *)alloc(8 * n);
    out->ncig = (int32_t *)alloc(4 * n);
    out->seq = (uint8_t *)alloc((size_t)R.seq_len);
    out->qual = (uint8_t *)alloc((size_t)R.seq_len);
    out->cig = (uint32_t *)alloc(4 * (size_t)R.cig_len);
    out->seq_len = R.seq_len;
    out->cig_len = R.cig_len;
    if (!out->rid || !out->pos1 || !out->score || !out->flags || !out->seq_off || !out->lseq || !out->cig_off ||
        !out->ncig || !out->seq || !out->qual || !out->cig) {
        pr_bam_alns_free(out);
        return pr_set_error(PR_ERR_ARG, "out of host memory");
    }
    hipStream_t s = c->stream;
    if ((rc = download(out->rid, b[0], n, s)) || (rc = download(out->pos1, b[1], n, s)) ||
        (rc = download(out->score, b[2], n, s)) || (rc = download(out->flags, b[3], n, s)) ||
        (rc = download(out->seq_off, b[4], n, s)) || (rc = download(out->lseq, b[5], n, s)) ||
        (rc = download(out->cig_off, b[6], n, s)) || (rc = download(out->ncig, b[7], n, s)) ||
        (rc = download(out->seq, b[8], (size_t)R.seq_len, s)) || (rc = download(out->qual, b[9], (size_t)R.seq_len, s)) ||
        (rc = download(out->cig, b[10], (size_t)R.cig_len, s)) ||
        (hipStreamSynchronize(s) != hipSuccess && (rc = pr_set_error(PR_ERR_HIP, "download of the decoded columns failed")))) {
        pr_bam_alns_free(out);
        return rc;
    }
    return 0;
}

extern "C" int pr_cns_upload_bam(pr_ctx *c, const pr_cns_batch *reads, const uint8_t *recs, int64_t len,
                                 const int32_t *ref_to_lr, int32_t n_ref, int64_t *n_kept) {
    return pr_cns_upload_bam_opts(c, reads, recs, len, ref_to_lr, n_ref, 0, n_kept, nullptr);
}

extern "C" int pr_cns_upload_bam_opts(pr_ctx *c, const pr_cns_batch *reads, const uint8_t *recs, int64_t len,
                                      const int32_t *ref_to_lr, int32_t n_ref, uint32_t flags, int64_t *n_kept,
                                      int64_t *n_restored) {
    if (!c || !reads || len < 0 || (len && !recs) || n_ref < 0 || (n_ref && !ref_to_lr))
        return pr_set_error(PR_ERR_ARG, "null arg");
    if (flags & ~(uint32_t)PR_BAM_RESTORE_SEQ) return set_error(PR_ERR_ARG, "unknown BAM decode flags 0x%x", flags);
    const int32_t n = reads->n_lr;
    if (n < 0 || (n && !reads->lr_off)) return pr_set_error(PR_ERR_ARG, "lr_off required");
    if (n && reads->lr_off[0] != 0) return pr_set_error(PR_ERR_ARG, "offsets must start at 0");
    for (int32_t i = 0; i < n; ++i)
        if (reads->lr_off[i + 1] < reads->lr_off[i] || (reads->ign_off && reads->ign_off[i + 1] < reads->ign_off[i]))
            return set_error(PR_ERR_ARG, "offsets not monotone at %d", i);
    c->cns_loaded = false;
    int rc = cns_upload_long_reads(c, reads);
    if (rc) return rc;
    DevBuf *B = c->cb;
    static const int32_t none = -1;
    const Columns O = {nullptr, &B[CB_POS], &B[CB_SCORE], &B[CB_AFLAGS], &B[CB_SEQ_OFF], &B[CB_LSEQ], &B[CB_CIG_OFF],
                       &B[CB_NCIG], &B[CB_SEQ], nullptr, &B[CB_CIG]};
    Decoded R;
    if ((rc = decode(c, recs, len, n_ref ? ref_to_lr : &none, n_ref ? n_ref : 1, n, O, R, flags, n_restored))) return rc;
    // offsets, output bounds and the byte model as pr_cns_upload derives them from a host batch
    c->n_aln = R.n_kept;
    c->aln_off_host.assign((size_t)n + 1, 0);
    c->out_off.assign((size_t)n + 1, 0);
    c->chim_off.assign((size_t)n + 1, 0);
    c->k_need = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t L = reads->lr_off[i + 1] - reads->lr_off[i];
        c->aln_off_host[(size_t)i + 1] = c->aln_off_host[(size_t)i] + R.lr_count[(size_t)i];
        c->out_off[(size_t)i + 1] = c->out_off[(size_t)i] + L + R.lr_ins[(size_t)i] + 1;
        c->chim_off[(size_t)i + 1] = c->chim_off[(size_t)i] + ((int64_t)((double)L / 20.0) + 1) / 2 + 2;
        if (R.lr_count[(size_t)i] > c->k_need) c->k_need = R.lr_count[(size_t)i];
    }
    c->seq_cap = c->out_off[(size_t)n];
    c->chim_cap = c->chim_off[(size_t)n];
    const int64_t tl = c->total_cols;
    c->alg_bytes = R.seq_len + 4 * R.cig_len + 16 * R.n_kept + tl * 2 + tl * 2 + tl * 6 * 4 * 2;
    if ((rc = upload(B[CB_ALN_OFF], c->aln_off_host.data(), (size_t)n + 1, c->stream))) return rc;
    if ((rc = cns_alloc_resident(c))) return rc;
    if (n_kept) *n_kept = R.n_kept;
    return 0;
}

extern "C" int pr_cns_resident_bounds(pr_ctx *c, pr_cns_bounds *out) {
    if (!c || !out) return pr_set_error(PR_ERR_ARG, "null arg");
    if (!c->cns_loaded || c->pipe) return pr_set_error(PR_ERR_ARG, "no resident consensus batch (pr_cns_upload / pr_cns_upload_bam first)");
    out->seq_cap = c->seq_cap;
    out->chim_cap = c->chim_cap;
    return 0;
}

extern "C" int pr_cns_resident_aln_count(pr_ctx *c, int64_t *n_aln, int64_t *aln_off) {
    if (!c) return pr_set_error(PR_ERR_ARG, "null ctx");
    if (!c->cns_loaded || c->pipe) return pr_set_error(PR_ERR_ARG, "no resident consensus batch (pr_cns_upload / pr_cns_upload_bam first)");
    if (n_aln) *n_aln = c->n_aln;
    if (aln_off) std::memcpy(aln_off, c->aln_off_host.data(), c->aln_off_host.size() * sizeof(int64_t));
    return 0;
}

extern "C" int pr_bam_decode_last_ms(pr_ctx *c, double *ms) {
    if (!c || !ms) return pr_set_error(PR_ERR_ARG, "null arg");
    *ms = c->ms_bam;
    return 0;
}

// ---------------------------------------------------------------------------
// the encoder: the resident hand-off as BAM records
namespace {

struct EncEvents {
    hipEvent_t ev[4] = {};
    ~EncEvents() {
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// the record stream's device buffer is not held past the call that made it (up to a GiB per range)
struct ReleaseOnExit {
    DevBuf &b;
    ~ReleaseOnExit() { b.release(); }
};

// The refusals, the uploads (once per launch), the FLAG scatter and the size pass of the range:
// D is ready for the write pass, *total the bytes of the range's records.
int export_prepare(pr_ctx *c, const pr_bam_export_in *in, BamEncDev &D, int64_t *total, EncEvents &E) {
    if (!c || !in) return pr_set_error(PR_ERR_ARG, "null arg");
    if (c->pipe && c->own)
        return pr_set_error(PR_ERR_UNSUPPORTED, "BAM export: an owned batch carries only the strand bit of FLAG");
    if (!c->pipe || !c->ho_done)
        return pr_set_error(PR_ERR_ARG, "BAM export: no resident bwa-mode iteration (pr_iter_launch first)");
    SwResident &r = c->sw;
    if (!r.loaded || c->ho_sw_gen != r.gen)   // a pr_sw_upload / pr_sw_launch of its own since: other pools under the old hand-off
        return pr_set_error(PR_ERR_ARG, "BAM export: the SW batch was uploaded or launched again after the hand-off "
                                        "(pr_iter_launch first)");
    if (!r.bwa)
        return pr_set_error(PR_ERR_ARG, "BAM export: an explicit-task batch has no FLAG column (bwa mode only)");
    if (!in->sr_off || !in->sr_names || !in->sr_name_off) return pr_set_error(PR_ERR_ARG, "BAM export: null pools");
    if (in->lr_first < 0 || in->lr_count < 0 || (int64_t)in->lr_first + in->lr_count > c->n_lr)
        return set_error(PR_ERR_ARG, "BAM export: reads [%d, %d + %d) outside the batch's %d", in->lr_first, in->lr_first,
                         in->lr_count, c->n_lr);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t n_sr = (size_t)r.n_sr;
    DevBuf *B = c->eb;
    int rc;
    if (c->eb_sr_gen != r.gen) {   // the batch's offsets, downloaded once per SW batch
        c->eb_sr_gen = -1;
        c->eb_sr_off.assign(n_sr + 1, 0);
        HIPCHK(hipMemcpyAsync(c->eb_sr_off.data(), r.buf[SWB_SR_OFF].p, (n_sr + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        c->eb_sr_gen = r.gen;
    }
    const std::vector<int64_t> &batch_off = c->eb_sr_off;
    if (std::memcmp(batch_off.data(), in->sr_off, (n_sr + 1) * 8) != 0)
        return pr_set_error(PR_ERR_ARG, "BAM export: sr_off differs from the resident batch's short reads");
    const bool fill = c->eb_gen != c->iter_gen || c->eb_names_key != (const void *)in->sr_names ||
                      c->eb_qual_key != (const void *)in->sr_qual;
    if (fill) {
        if (in->sr_name_off[0] < 0) return pr_set_error(PR_ERR_ARG, "BAM export: sr_name_off must start at or after 0");
        for (size_t i = 0; i < n_sr; ++i) {
            const int64_t l = in->sr_name_off[i + 1] - in->sr_name_off[i];
            if (l < 1 || l > 254)
                return set_error(PR_ERR_ARG, "BAM export: the name of short read %zu (%.*s%s) has %lld bytes: 1 to 254 fit l_read_name",
                                 i, (int)(l > 32 ? 32 : (l > 0 ? l : 0)), in->sr_names + in->sr_name_off[i], l > 32 ? "..." : "",
                                 (long long)l);
        }
    }
    std::memset(&D, 0, sizeof D);
    D.lr_first = in->lr_first;
    D.lr_count = in->lr_count;
    D.aln_off = c->cb[CB_ALN_OFF].as<int64_t>();
    // the range's alignments, and the hand-off's error flags of its reads: a read whose hand-off
    // failed has no order to export (pr_iter_download reports the same flags)
    int64_t a[2] = {0, 0};
    std::vector<int32_t> err((size_t)in->lr_count + 1, 0);
    HIPCHK(hipMemcpyAsync(&a[0], D.aln_off + in->lr_first, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&a[1], D.aln_off + in->lr_first + in->lr_count, 8, hipMemcpyDeviceToHost, s));
    if (in->lr_count)
        HIPCHK(hipMemcpyAsync(err.data(), c->pb[PB_ERR].as<int32_t>() + in->lr_first, (size_t)in->lr_count * 4,
                              hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int32_t i = 0; i < in->lr_count; ++i)
        if (err[(size_t)i])
            return set_error(PR_ERR_CAPACITY, "BAM export: the hand-off of long read %d failed (code %d)", in->lr_first + i,
                             err[(size_t)i]);
    if (a[0] < 0 || a[1] < a[0] || a[1] > r.n_aln) return pr_set_error(PR_ERR_ARG, "BAM export: the hand-off's offsets are not those of this batch");
    for (auto &e : E.ev) HIPCHK(hipEventCreate(&e));
    D.g0 = a[0];
    D.n = a[1] - a[0];
    SwPtrs sp;
    if ((rc = sw_get_pipe_ptrs(c, &sp, false))) return rc;
    D.a_pos = c->cb[CB_POS].as<int32_t>();
    D.a_score = c->cb[CB_SCORE].as<double>();
    D.a_lseq = c->cb[CB_LSEQ].as<int32_t>();
    D.a_ncig = c->cb[CB_NCIG].as<int32_t>();
    D.a_task = c->pb[PB_ORDER].as<int32_t>();
    D.task_off = sp.task_off;
    D.t_sr = sp.t_sr;
    D.strand = sp.strand;
    D.cig_at = sp.cig_at;
    D.glist = r.buf[SWB_GLIST].as<int32_t>();
    D.cig = sp.cig;
    D.sr = sp.sr;
    D.sr_off = sp.sr_off;
    D.alist = r.buf[SWB_ALIST].as<int32_t>();
    D.aflag = r.buf[SWB_AFLAG].as<int32_t>();
    D.n_sam = r.n_aln;
    const size_t n1 = (size_t)D.n + 1, tb = bam_enc_temp_bytes(D.n);
    if (fill) {
        c->eb_gen = -1;
        const size_t nb = (size_t)in->sr_name_off[n_sr] - (size_t)in->sr_name_off[0];
        // (name offsets as given: the pool is uploaded from its first used byte, the offsets rebased)
        std::vector<int64_t> noff(n_sr + 1);
        for (size_t i = 0; i <= n_sr; ++i) noff[i] = in->sr_name_off[i] - in->sr_name_off[0];
        if ((rc = upload(B[EB_NAMES], (const uint8_t *)in->sr_names + in->sr_name_off[0], nb, s)) ||
            (rc = upload(B[EB_NAME_OFF], noff.data(), n_sr + 1, s)) ||
            (in->sr_qual && (rc = upload(B[EB_QUAL], in->sr_qual, (size_t)batch_off[n_sr], s))) ||
            (rc = B[EB_FLAG].ensure(((size_t)r.n_task + 1) * 2)))
            return rc;
        HIPCHK(hipStreamSynchronize(s));   // (noff leaves scope)
    }
    if ((rc = B[EB_LR].ensure(n1 * 4)) || (rc = B[EB_J].ensure(n1 * 4)) || (rc = B[EB_SIZE].ensure(n1 * 8)) ||
        (rc = B[EB_OFF].ensure(n1 * 8)) || (rc = B[EB_TEMP].ensure(tb)))
        return rc;
    D.flag_by_task = B[EB_FLAG].as<uint16_t>();
    D.names = B[EB_NAMES].as<uint8_t>();
    D.name_off = B[EB_NAME_OFF].as<int64_t>();
    D.qual = in->sr_qual ? B[EB_QUAL].as<uint8_t>() : nullptr;
    D.e_lr = B[EB_LR].as<int32_t>();
    D.e_j = B[EB_J].as<int32_t>();
    D.e_size = B[EB_SIZE].as<int64_t>();
    D.e_off = B[EB_OFF].as<int64_t>();
    HIPCHK(hipEventRecord(E.ev[0], s));
    if (fill) HIPCHK((hipError_t)bam_enc_flag_pass(D, (void *)s));
    HIPCHK((hipError_t)bam_enc_size_pass(D, B[EB_OFF].as<int64_t>(), B[EB_TEMP].p, tb, (void *)s));
    HIPCHK(hipEventRecord(E.ev[1], s));
    HIPCHK(hipMemcpyAsync(total, D.e_off + D.n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (fill) {
        c->eb_gen = c->iter_gen;
        c->eb_names_key = in->sr_names;
        c->eb_qual_key = in->sr_qual;
    }
    float ms = 0.f;
    c->ms_bam_enc = hipEventElapsedTime(&ms, E.ev[0], E.ev[1]) == hipSuccess ? ms : 0.f;
    return 0;
}

}   // namespace

extern "C" int pr_iter_export_bam_bytes(pr_ctx *c, const pr_bam_export_in *in, int64_t *len) {
    if (!len) return pr_set_error(PR_ERR_ARG, "null arg");
    BamEncDev D;
    EncEvents E;
    return export_prepare(c, in, D, len, E);
}

extern "C" int pr_iter_export_bam_read_bytes(pr_ctx *c, const pr_bam_export_in *in, int64_t *per_read) {
    if (!per_read) return pr_set_error(PR_ERR_ARG, "null arg");
    BamEncDev D;
    EncEvents E;
    int64_t total = 0;
    int rc = export_prepare(c, in, D, &total, E);
    if (rc || in->lr_count == 0) return rc;
    DevBuf &rb = c->eb[EB_READ_BYTES];
    if ((rc = rb.ensure((size_t)in->lr_count * 8))) return rc;
    HIPCHK((hipError_t)bam_enc_read_bytes(D, rb.as<int64_t>(), (void *)c->stream));
    HIPCHK(hipMemcpyAsync(per_read, rb.p, (size_t)in->lr_count * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int pr_iter_export_bam(pr_ctx *c, const pr_bam_export_in *in, uint8_t **recs, int64_t *len, int64_t *n_records) {
    if (!recs || !len) return pr_set_error(PR_ERR_ARG, "null arg");
    *recs = nullptr;
    *len = 0;
    BamEncDev D;
    EncEvents E;
    int64_t total = 0;
    int rc = export_prepare(c, in, D, &total, E);
    if (rc) return rc;
    hipStream_t s = c->stream;
    DevBuf &out = c->eb[EB_OUT];
    ReleaseOnExit out_guard{out};
    if ((rc = out.ensure((size_t)total + 16))) return rc;
    D.out = out.as<uint8_t>();
    HIPCHK(hipEventRecord(E.ev[2], s));
    HIPCHK((hipError_t)bam_enc_write_pass(D, (void *)s));
    HIPCHK(hipEventRecord(E.ev[3], s));
    uint8_t *h = (uint8_t *)std::malloc(total ? (size_t)total : 1);
    if (!h) {
        (void)hipStreamSynchronize(s);   // (the write pass, before its buffer goes)
        return set_error(PR_ERR_CAPACITY, "BAM export: no host memory for %lld bytes of records: export fewer reads per call",
                         (long long)total);
    }
    hipError_t e = total ? hipMemcpyAsync(h, out.p, (size_t)total, hipMemcpyDeviceToHost, s) : hipSuccess;
    const hipError_t e2 = hipStreamSynchronize(s);   // (also after a failed copy: the write pass still runs)
    if (e == hipSuccess) e = e2;
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        std::free(h);
        return set_error(PR_ERR_HIP, "BAM export: %s", hipGetErrorString(e));
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, E.ev[2], E.ev[3]) == hipSuccess) c->ms_bam_enc += ms;
    *recs = h;
    *len = total;
    if (n_records) *n_records = D.n;
    return 0;
}

extern "C" int pr_bam_export_last_ms(pr_ctx *c, double *ms) {
    if (!c || !ms) return pr_set_error(PR_ERR_ARG, "null arg");
    *ms = c->ms_bam_enc;
    return 0;
}

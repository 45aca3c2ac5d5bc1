// The unitig consensus entries of the C-ABI (include/prgpu.h): `bam2cns --utg-mode`, the
// generate_consensus of bam2cns:375-455 for a batch of long reads, on the host (threads over
// reads) or on the device (utg_kernels.hip).  Both paths run utg_core.h.
#include <atomic>
#include <thread>

#include "ctx.h"
#include "utg_dev.h"

using namespace prgpu::utg;

namespace {

int check_params(const pr_utg_params *p) {
    if (!p) return pr_set_error(PR_ERR_ARG, "utg: no parameters");
    if (p->min_aln_length < 0 || p->phred_offset < 0 || p->ref_phred_offset < 0 || p->indel_taboo_length < 0 || p->max_ins_length < 0 ||
        !(p->indel_taboo >= 0.0) || p->indel_taboo > 1.0 || p->fallback_phred < 0 || p->fallback_phred + p->phred_offset > 255)
        return pr_set_error(PR_ERR_ARG, "utg: bad consensus settings");
    if (p->has_min_ncscore && p->min_ncscore != p->min_ncscore) return pr_set_error(PR_ERR_ARG, "utg: min_ncscore is not a number");
    return 0;
}

int check_batch(const pr_utg_batch *b, const pr_utg_out *o) {
    if (!b || b->n_reads < 0 || b->n_alns < 0) return pr_set_error(PR_ERR_ARG, "utg: bad batch");
    if (!b->n_reads) return 0;
    if (!b->read_off || !b->ref_seq || !b->aln_off || !b->ign_off || !b->out_off || !b->win_off)
        return pr_set_error(PR_ERR_ARG, "utg: batch without arrays");
    if (b->n_alns && (!b->pos || !b->score || !b->has_score || !b->has_qual || !b->seq_off || !b->seq || !b->qual || !b->cig_off || !b->cigar))
        return pr_set_error(PR_ERR_ARG, "utg: batch without alignment arrays");
    if (!o || !o->status || !o->seq_len || !o->trace_len || !o->n_win || !o->seq || !o->qual || !o->trace || !o->win || (b->n_alns && !o->kept))
        return pr_set_error(PR_ERR_ARG, "utg: no output arrays");
    if (b->aln_off[0] != 0 || b->aln_off[b->n_reads] != b->n_alns || b->read_off[0] < 0 || b->ign_off[0] < 0)
        return pr_set_error(PR_ERR_ARG, "utg: offsets do not span the batch");
    for (int64_t a = 0; a < b->n_alns; ++a)
        if (b->seq_off[a + 1] < b->seq_off[a] || b->cig_off[a + 1] < b->cig_off[a] || b->seq_off[a + 1] - b->seq_off[a] > INT32_MAX / 4 ||
            b->cig_off[a + 1] - b->cig_off[a] > INT32_MAX / 4)
            return pr_set_error(PR_ERR_ARG, "utg: offsets not monotone");
    for (int r = 0; r < b->n_reads; ++r) {
        const int64_t len = b->read_off[r + 1] - b->read_off[r], na = b->aln_off[r + 1] - b->aln_off[r];
        if (len < 0 || na < 0 || b->ign_off[r + 1] < b->ign_off[r] || b->out_off[r + 1] < b->out_off[r] || b->win_off[r + 1] < b->win_off[r])
            return pr_set_error(PR_ERR_ARG, "utg: offsets not monotone");
        if (len > PR_UTG_MAX_LEN || na > PR_UTG_MAX_ALNS) continue;   // flagged, no output
        int64_t need = len;
        for (int64_t a = b->aln_off[r]; a < b->aln_off[r + 1]; ++a) need += b->seq_off[a + 1] - b->seq_off[a];
        if (b->out_off[r + 1] - b->out_off[r] < need) return set_error(PR_ERR_ARG, "utg: output slot of read %d too small", r);
        if (b->win_off[r + 1] - b->win_off[r] < std::max<int64_t>(na, 1)) return set_error(PR_ERR_ARG, "utg: window slot of read %d too small", r);
    }
    return 0;
}

int read_status(const pr_utg_batch *b, int r) {
    return (b->read_off[r + 1] - b->read_off[r] > PR_UTG_MAX_LEN ? PR_UTG_TOO_LONG : 0) |
           (b->aln_off[r + 1] - b->aln_off[r] > PR_UTG_MAX_ALNS ? PR_UTG_TOO_MANY : 0);
}

// Seq.pm:281-284: a missing QUAL is --fallback-phred over the whole SEQ
std::vector<uint8_t> filled_quals(const pr_utg_params &p, const pr_utg_batch *b) {
    const int64_t n = b->n_alns ? b->seq_off[b->n_alns] : 0;
    std::vector<uint8_t> q((size_t)n + 1, 0);
    for (int64_t a = 0; a < b->n_alns; ++a) {
        const int64_t s = b->seq_off[a], e = b->seq_off[a + 1];
        if (b->has_qual[a]) std::copy(b->qual + s, b->qual + e, q.begin() + s);
        else std::fill(q.begin() + s, q.begin() + e, (uint8_t)(p.fallback_phred + p.phred_offset));
    }
    return q;
}

void clear_out(const pr_utg_batch *b, pr_utg_out *o) {
    for (int r = 0; r < b->n_reads; ++r) o->status[r] = read_status(b, r), o->seq_len[r] = o->trace_len[r] = o->n_win[r] = 0;
    for (int64_t a = 0; a < b->n_alns; ++a) o->kept[a] = 0;
}

int run_host(const pr_utg_params &p, const pr_utg_batch *b, int n_threads, pr_utg_out *o) {
    const std::vector<uint8_t> qual = filled_quals(p, b);
    const size_t na = (size_t)b->n_alns + 1, nc = (size_t)(b->n_alns ? b->cig_off[b->n_alns] : 0) + 1, nr = (size_t)b->n_reads;
    std::vector<Prep> prep(na);
    std::vector<int32_t> alen(na), span_e(na), op_r(nc), op_q(nc), cov((size_t)b->read_off[nr] + nr + 1), ulist(na), rlist(na), n_u(nr), n_r(nr);
    std::vector<double> sc(na);
    std::vector<uint8_t> flag(na);
    View V = {};
    V.p = p, V.sp = sm_params(p), V.b = *b, V.o = *o;
    V.b.qual = qual.data();
    V.prep = prep.data(), V.alen = alen.data(), V.span_e = span_e.data(), V.sc = sc.data(), V.flag = flag.data();
    V.op_r = op_r.data(), V.op_q = op_q.data(), V.cov = cov.data(), V.ulist = ulist.data(), V.rlist = rlist.data();
    V.n_u = n_u.data(), V.n_r = n_r.data();
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int r; (r = next.fetch_add(1)) < b->n_reads;)
            if (!o->status[r]) run_read_host(V, r);
    };
    int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(std::min(nt, 64), b->n_reads));
    if (nt == 1) {
        work();
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work);
        for (auto &x : th) x.join();
    }
    return 0;
}

int run_gpu(pr_ctx *c, const pr_utg_params &p, const pr_utg_batch *b, pr_utg_out *o) {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->ms_utg = 0.f;
    int kernel = 0;
    for (float &x : c->ms_utg_k) x = 0.f;
    const int nr = b->n_reads;
    const int64_t na = b->n_alns;
    enum { B_ROFF, B_RSEQ, B_RQUAL, B_AOFF, B_POS, B_SCORE, B_HASSC, B_SOFF, B_SEQ, B_QUAL, B_COFF, B_CIG, B_IOFF, B_IGN, B_OOFF, B_WOFF,
           B_AREAD, B_PREP, B_ALEN, B_SPANE, B_SC, B_FLAG, B_OPR, B_OPQ, B_COV, B_ULIST, B_RLIST, B_NU, B_NR, B_FPOS, B_FLEN, B_FID, B_FSC,
           B_OST, B_OSL, B_OTL, B_ONW, B_OSEQ, B_OQUAL, B_OTRACE, B_OKEPT, B_OWIN, B_PSAT, B_PTAT, B_PSEQ, B_PQUAL, B_PTRACE, B_COUNT };
    DevBuf buf[B_COUNT];
    for (int k = 0; k < B_COUNT; ++k) buf[k].grp = "utg", buf[k].id = k;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    auto timed = [&](auto &&launch) -> int {
        HIPCHK(hipEventRecord(ev0, s));
        HIPCHK((hipError_t)launch());
        HIPCHK(hipEventRecord(ev1, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) c->ms_utg += ms, c->ms_utg_k[kernel] = ms;
        ++kernel;
        return 0;
    };
    const std::vector<uint8_t> qual = filled_quals(p, b);
    std::vector<int32_t> aread((size_t)na + 1, 0);
    for (int r = 0; r < nr; ++r)
        for (int64_t a = b->aln_off[r]; a < b->aln_off[r + 1]; ++a) aread[a] = r;
    auto body = [&]() -> int {
        int e;
        HIPCHK(hipEventCreate(&ev0));
        HIPCHK(hipEventCreate(&ev1));
        const int64_t nbases = b->read_off[nr], nseq = na ? b->seq_off[na] : 0, ncig = na ? b->cig_off[na] : 0;
        const int64_t nign = b->ign_off[nr], nout = b->out_off[nr], nwin = b->win_off[nr];
        const int64_t zero64[2] = {0, 0};
        if ((e = upload(buf[B_ROFF], b->read_off, (size_t)nr + 1, s))) return e;
        if ((e = upload(buf[B_RSEQ], b->ref_seq, (size_t)nbases, s))) return e;
        if (b->ref_qual && (e = upload(buf[B_RQUAL], b->ref_qual, (size_t)nbases, s))) return e;
        if ((e = upload(buf[B_AOFF], b->aln_off, (size_t)nr + 1, s))) return e;
        if ((e = upload(buf[B_POS], b->pos, (size_t)na, s))) return e;
        if ((e = upload(buf[B_SCORE], b->score, (size_t)na, s))) return e;
        if ((e = upload(buf[B_HASSC], b->has_score, (size_t)na, s))) return e;
        if ((e = upload(buf[B_SOFF], na ? b->seq_off : zero64, (size_t)na + 1, s))) return e;
        if ((e = upload(buf[B_SEQ], b->seq, (size_t)nseq, s))) return e;
        if ((e = upload(buf[B_QUAL], qual.data(), (size_t)nseq, s))) return e;
        if ((e = upload(buf[B_COFF], na ? b->cig_off : zero64, (size_t)na + 1, s))) return e;
        if ((e = upload(buf[B_CIG], b->cigar, (size_t)ncig, s))) return e;
        if ((e = upload(buf[B_IOFF], b->ign_off, (size_t)nr + 1, s))) return e;
        if ((e = upload(buf[B_IGN], b->ign, (size_t)(2 * nign), s))) return e;
        if ((e = upload(buf[B_OOFF], b->out_off, (size_t)nr + 1, s))) return e;
        if ((e = upload(buf[B_WOFF], b->win_off, (size_t)nr + 1, s))) return e;
        if ((e = upload(buf[B_AREAD], aread.data(), (size_t)na, s))) return e;
        if ((e = upload(buf[B_OST], o->status, (size_t)nr, s))) return e;
        if ((e = buf[B_PREP].ensure((size_t)na * sizeof(Prep)))) return e;
        for (int k : {B_ALEN, B_SPANE, B_ULIST, B_RLIST, B_FPOS, B_FLEN, B_FID})
            if ((e = buf[k].ensure((size_t)na * sizeof(int32_t)))) return e;
        for (int k : {B_SC, B_FSC})
            if ((e = buf[k].ensure((size_t)na * sizeof(double)))) return e;
        if ((e = buf[B_FLAG].ensure((size_t)na))) return e;
        if ((e = buf[B_OPR].ensure((size_t)ncig * sizeof(int32_t)))) return e;
        if ((e = buf[B_OPQ].ensure((size_t)ncig * sizeof(int32_t)))) return e;
        if ((e = buf[B_COV].ensure((size_t)(nbases + nr) * sizeof(int32_t)))) return e;
        for (int k : {B_NU, B_NR, B_OSL, B_OTL, B_ONW}) {
            if ((e = buf[k].ensure((size_t)nr * sizeof(int32_t)))) return e;
            HIPCHK(hipMemsetAsync(buf[k].p, 0, (size_t)nr * sizeof(int32_t), s));
        }
        for (int k : {B_OSEQ, B_OQUAL, B_OTRACE})
            if ((e = buf[k].ensure((size_t)nout))) return e;
        if ((e = buf[B_OKEPT].ensure((size_t)na))) return e;
        HIPCHK(hipMemsetAsync(buf[B_OKEPT].p, 0, (size_t)na + 1, s));
        if ((e = buf[B_OWIN].ensure((size_t)(2 * nwin) * sizeof(int32_t)))) return e;
        View V = {};
        V.p = p, V.sp = sm_params(p);
        V.b = *b;
        V.b.read_off = buf[B_ROFF].as<int64_t>(), V.b.ref_seq = buf[B_RSEQ].as<uint8_t>();
        V.b.ref_qual = b->ref_qual ? buf[B_RQUAL].as<uint8_t>() : nullptr;
        V.b.aln_off = buf[B_AOFF].as<int64_t>(), V.b.pos = buf[B_POS].as<int32_t>(), V.b.score = buf[B_SCORE].as<double>();
        V.b.has_score = buf[B_HASSC].as<uint8_t>(), V.b.has_qual = nullptr;
        V.b.seq_off = buf[B_SOFF].as<int64_t>(), V.b.seq = buf[B_SEQ].as<uint8_t>(), V.b.qual = buf[B_QUAL].as<uint8_t>();
        V.b.cig_off = buf[B_COFF].as<int64_t>(), V.b.cigar = buf[B_CIG].as<uint32_t>();
        V.b.ign_off = buf[B_IOFF].as<int64_t>(), V.b.ign = buf[B_IGN].as<int32_t>();
        V.b.out_off = buf[B_OOFF].as<int64_t>(), V.b.win_off = buf[B_WOFF].as<int64_t>();
        V.o.status = buf[B_OST].as<int32_t>(), V.o.seq_len = buf[B_OSL].as<int32_t>(), V.o.trace_len = buf[B_OTL].as<int32_t>();
        V.o.n_win = buf[B_ONW].as<int32_t>(), V.o.seq = buf[B_OSEQ].as<uint8_t>(), V.o.qual = buf[B_OQUAL].as<uint8_t>();
        V.o.trace = buf[B_OTRACE].as<uint8_t>(), V.o.kept = buf[B_OKEPT].as<uint8_t>(), V.o.win = buf[B_OWIN].as<int32_t>();
        V.aln_read = buf[B_AREAD].as<int32_t>(), V.prep = buf[B_PREP].as<Prep>(), V.alen = buf[B_ALEN].as<int32_t>();
        V.span_e = buf[B_SPANE].as<int32_t>(), V.sc = buf[B_SC].as<double>(), V.flag = buf[B_FLAG].as<uint8_t>();
        V.op_r = buf[B_OPR].as<int32_t>(), V.op_q = buf[B_OPQ].as<int32_t>(), V.cov = buf[B_COV].as<int32_t>();
        V.ulist = buf[B_ULIST].as<int32_t>(), V.rlist = buf[B_RLIST].as<int32_t>(), V.n_u = buf[B_NU].as<int32_t>(), V.n_r = buf[B_NR].as<int32_t>();
        V.f_pos = buf[B_FPOS].as<int32_t>(), V.f_len = buf[B_FLEN].as<int32_t>(), V.f_id = buf[B_FID].as<int32_t>(), V.f_sc = buf[B_FSC].as<double>();
        if ((e = timed([&]() { return utg_prep_launch(V, s); }))) return e;
        if ((e = timed([&]() { return utg_cov_launch(V, s); }))) return e;
        if ((e = timed([&]() { return utg_contained_launch(V, s); }))) return e;
        if ((e = timed([&]() { return utg_cns_launch(V, s); }))) return e;
        if ((e = download(o->status, buf[B_OST], (size_t)nr, s))) return e;
        if ((e = download(o->seq_len, buf[B_OSL], (size_t)nr, s))) return e;
        if ((e = download(o->trace_len, buf[B_OTL], (size_t)nr, s))) return e;
        if ((e = download(o->n_win, buf[B_ONW], (size_t)nr, s))) return e;
        if ((e = download(o->kept, buf[B_OKEPT], (size_t)na, s))) return e;
        if ((e = download(o->win, buf[B_OWIN], (size_t)(2 * nwin), s))) return e;
        HIPCHK(hipStreamSynchronize(s));
        // the outputs behind each other, one download, then into the caller's slots
        std::vector<int64_t> sat((size_t)nr + 1, 0), tat((size_t)nr + 1, 0);
        for (int r = 0; r < nr; ++r) sat[r + 1] = sat[r] + o->seq_len[r], tat[r + 1] = tat[r] + o->trace_len[r];
        if ((e = upload(buf[B_PSAT], sat.data(), (size_t)nr, s))) return e;
        if ((e = upload(buf[B_PTAT], tat.data(), (size_t)nr, s))) return e;
        if ((e = buf[B_PSEQ].ensure((size_t)sat[nr]))) return e;
        if ((e = buf[B_PQUAL].ensure((size_t)sat[nr]))) return e;
        if ((e = buf[B_PTRACE].ensure((size_t)tat[nr]))) return e;
        UtgPackDev P = {buf[B_PSAT].as<int64_t>(), buf[B_PTAT].as<int64_t>(), buf[B_PSEQ].as<uint8_t>(), buf[B_PQUAL].as<uint8_t>(),
                        buf[B_PTRACE].as<uint8_t>()};
        if ((e = timed([&]() { return utg_pack_launch(V, P, s); }))) return e;
        std::vector<uint8_t> hs((size_t)sat[nr] + 1), hq((size_t)sat[nr] + 1), ht((size_t)tat[nr] + 1);
        if ((e = download(hs.data(), buf[B_PSEQ], (size_t)sat[nr], s))) return e;
        if ((e = download(hq.data(), buf[B_PQUAL], (size_t)sat[nr], s))) return e;
        if ((e = download(ht.data(), buf[B_PTRACE], (size_t)tat[nr], s))) return e;
        HIPCHK(hipStreamSynchronize(s));
        for (int r = 0; r < nr; ++r) {
            std::copy(hs.begin() + sat[r], hs.begin() + sat[r + 1], o->seq + b->out_off[r]);
            std::copy(hq.begin() + sat[r], hq.begin() + sat[r + 1], o->qual + b->out_off[r]);
            std::copy(ht.begin() + tat[r], ht.begin() + tat[r + 1], o->trace + b->out_off[r]);
        }
        return 0;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(s);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (int k = 0; k < B_COUNT; ++k) buf[k].release();
    return rc;
}

}   // namespace

/* bam2cns:375-455 with --utg-mode: Seq.pm:919-927, 949-999, 1001-1047, bam2cns:398-422,
 * Seq.pm:714-734 */
extern "C" int pr_utg_run(pr_ctx *ctx, const pr_utg_params *p, const pr_utg_batch *b, int n_threads, pr_utg_out *out) {
    int rc = check_params(p);
    if (!rc) rc = check_batch(b, out);
    if (rc) return rc;
    if (!b->n_reads) return 0;
    clear_out(b, out);
    return ctx ? run_gpu(ctx, *p, b, out) : run_host(*p, b, n_threads, out);
}

extern "C" int pr_utg_last_ms(pr_ctx *ctx, double *ms) {
    if (!ctx || !ms) return pr_set_error(PR_ERR_ARG, "utg: no context");
    *ms = ctx->ms_utg;
    return 0;
}

extern "C" int pr_utg_last_split(pr_ctx *ctx, double *ms) {
    if (!ctx || !ms) return pr_set_error(PR_ERR_ARG, "utg: no context");
    for (int k = 0; k < 5; ++k) ms[k] = ctx->ms_utg_k[k];
    return 0;
}

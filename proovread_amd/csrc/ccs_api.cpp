// The ccs-1 entries of the C-ABI (include/prgpu.h): bin/ccseq's grouping (:237-299), its
// bwa-proovread calls replaced by rules (ccs_core.h) and the Sam::Seq consensus of each group,
// on the host (threads over groups) or on the device (ccs_kernels.hip).
#include <atomic>
#include <thread>

#include "ccs_dev.h"
#include "ctx.h"

using namespace prgpu::ccs;

namespace {

int check_params(const pr_ccs_params *p) {
    if (!p) return pr_set_error(PR_ERR_ARG, "ccs: no parameters");
    if (p->k < 1 || p->w < 1 || p->w > PR_CCS_MAX_BAND) return set_error(PR_ERR_ARG, "ccs: needs k >= 1 and 1 <= w <= %d", PR_CCS_MAX_BAND);
    if (p->a <= 0 || p->b < 0 || p->o_del < 0 || p->o_ins < 0 || p->e_del <= 0 || p->e_ins <= 0 || p->a > 127 || p->b > 127 ||
        p->o_del > 1000 || p->o_ins > 1000 || p->e_del > 1000 || p->e_ins > 1000)
        return pr_set_error(PR_ERR_ARG, "ccs: needs 0 < a, 0 <= b (both <= 127), 0 <= o, 0 < e (<= 1000)");
    if (p->min_aln_length < 0 || p->phred_offset < 0 || !(p->indel_taboo >= 0.0) || p->indel_taboo > 1.0)
        return pr_set_error(PR_ERR_ARG, "ccs: bad consensus settings");
    return 0;
}

int64_t len_of(const pr_ccs_batch *b, int s) { return b->off[s + 1] - b->off[s]; }

// shapes, slots and alphabet; with_out: the output slots too
int check_batch(const pr_ccs_batch *b, bool with_out) {
    if (!b || b->n_groups < 0 || b->n_sub < 0) return pr_set_error(PR_ERR_ARG, "ccs: bad batch");
    if (!b->n_groups) return 0;
    if (!b->grp_off || !b->grp_ref || !b->off || !b->seq || !b->qual || !b->cig_off || (with_out && !b->out_off))
        return pr_set_error(PR_ERR_ARG, "ccs: batch without arrays");
    for (int s = 0; s < b->n_sub; ++s)
        if (b->off[s + 1] < b->off[s] || b->cig_off[s + 1] < b->cig_off[s] || len_of(b, s) > INT32_MAX / 4)
            return pr_set_error(PR_ERR_ARG, "ccs: offsets not monotone");
    if (b->grp_off[0] < 0 || b->grp_off[b->n_groups] > b->n_sub) return pr_set_error(PR_ERR_ARG, "ccs: groups leave the batch");
    for (int g = 0; g < b->n_groups; ++g) {
        const int s0 = b->grp_off[g], s1 = b->grp_off[g + 1], r = b->grp_ref[g];
        if (s1 - s0 < 2 || r < s0 || r >= s1) return set_error(PR_ERR_ARG, "ccs: group %d needs two subreads and a reference among them", g);
        int64_t total = 0;
        for (int s = s0; s < s1; ++s) {
            total += len_of(b, s);
            if (s != r && b->cig_off[s + 1] - b->cig_off[s] < len_of(b, s) + len_of(b, r) + 2)
                return set_error(PR_ERR_ARG, "ccs: CIGAR slot of subread %d too small", s);
        }
        if (with_out && (b->out_off[g + 1] < b->out_off[g] || b->out_off[g + 1] - b->out_off[g] < total))
            return set_error(PR_ERR_ARG, "ccs: output slot of group %d too small", g);
    }
    const int64_t nb = b->off[b->n_sub];
    for (int64_t x = b->off[0]; x < nb; ++x) {
        const uint8_t c = b->seq[x];
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'N')
            return set_error(PR_ERR_ARG, "ccs: sequences must be A C G T N (byte %lld)", (long long)x);
    }
    return 0;
}

int group_status(const pr_ccs_batch *b, int g) {
    int st = b->grp_off[g + 1] - b->grp_off[g] > PR_CCS_MAX_SUBREADS ? PR_CCS_TOO_MANY : 0;
    for (int s = b->grp_off[g]; s < b->grp_off[g + 1]; ++s)
        if (len_of(b, s) > PR_CCS_MAX_LEN) st |= PR_CCS_TOO_LONG;
    return st;
}

int n_workers(int n_threads, int64_t n) {
    int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(nt, 64));
    return (int)std::min<int64_t>(nt, std::max<int64_t>(n, 1));
}

template <class F>
void over_groups(int n_groups, int n_threads, F f) {
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int g; (g = next.fetch_add(1)) < n_groups;) f(g);
    };
    const int nt = n_workers(n_threads, n_groups);
    if (nt == 1) {
        work();
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work);
        for (auto &x : th) x.join();
    }
}

Read read_of(const pr_ccs_batch *b, int s, int rev) { return Read{b->seq + b->off[s], b->qual + b->off[s], (int32_t)len_of(b, s), rev}; }

void clear_alns(const pr_ccs_batch *b, pr_ccs_alns *A) {
    for (int s = 0; s < b->n_sub; ++s) A->mapped[s] = A->strand[s] = A->pos[s] = A->score[s] = A->n_cigar[s] = 0;
}

void map_group_host(const pr_ccs_params &p, const pr_ccs_batch *b, int g, pr_ccs_alns *A, std::vector<uint8_t> &dir) {
    const int r = b->grp_ref[g];
    const Read R = read_of(b, r, 0);
    for (int s = b->grp_off[g]; s < b->grp_off[g + 1]; ++s) {
        if (s == r) continue;   // -e: the reference is not aligned to itself
        const Centre c = centre_host(p, R, read_of(b, s, 0));
        if (!c.found) continue;
        const Aln a = align_host(p, R, read_of(b, s, c.rev), c.d0, dir, A->cigar + b->cig_off[s]);
        A->mapped[s] = a.mapped, A->strand[s] = a.mapped ? a.strand : 0, A->pos[s] = a.pos, A->score[s] = a.score, A->n_cigar[s] = a.n_cigar;
    }
}

int run_host(const pr_ccs_params &p, const pr_ccs_batch *b, int n_threads, pr_ccs_alns *A, bool do_map, pr_ccs_out *O) {
    over_groups(b->n_groups, n_threads, [&](int g) {
        const int st = group_status(b, g);
        if (O) O->status[g] = st, O->seq_len[g] = 0, O->trace_len[g] = 0;
        if (st) return;
        std::vector<uint8_t> dir;
        std::vector<ColEnt> slab;
        if (do_map) map_group_host(p, b, g, A, dir);
        if (O) cns_group_host(p, b, g, A, O, slab);
    });
    return 0;
}

// the device path: uploads, the mapping in chunks of pairs that bound the direction slab, the
// consensus in chunks of groups that bound the column maps
int run_gpu(pr_ctx *c, const pr_ccs_params &p, const pr_ccs_batch *b, pr_ccs_alns *A, bool do_map, pr_ccs_out *O) {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->ms_ccs = 0.f;
    const int ng = b->n_groups, nsub = b->n_sub;
    std::vector<int32_t> status((size_t)ng), glist, psub, pref;
    for (int g = 0; g < ng; ++g) {
        status[g] = group_status(b, g);
        if (O) O->status[g] = status[g], O->seq_len[g] = 0, O->trace_len[g] = 0;
        if (status[g]) continue;
        glist.push_back(g);
        for (int q = b->grp_off[g]; q < b->grp_off[g + 1]; ++q)
            if (q != b->grp_ref[g]) psub.push_back(q), pref.push_back(b->grp_ref[g]);
    }
    if (glist.empty()) return 0;
    enum { B_SEQ, B_QUAL, B_OFF, B_GOFF, B_GREF, B_CIGOFF, B_MAPPED, B_STRAND, B_POS, B_SCORE, B_NCIG, B_CIG, B_PSUB, B_PREF,
           B_BSUM, B_BKEY, B_BOFF, B_CENTRE, B_DIR, B_DIROFF, B_GLIST, B_SLAB, B_SLABOFF, B_OPR, B_OPQ, B_OUTOFF, B_OSEQ,
           B_OQUAL, B_OTRACE, B_OST, B_OSL, B_OTL, B_COUNT };
    DevBuf buf[B_COUNT];
    for (int k = 0; k < B_COUNT; ++k) buf[k].grp = "ccs", buf[k].id = k;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    auto timed = [&](auto &&launch) -> int {
        HIPCHK(hipEventRecord(ev0, s));
        HIPCHK((hipError_t)launch());
        HIPCHK(hipEventRecord(ev1, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) c->ms_ccs += ms;
        return 0;
    };
    auto body = [&]() -> int {
        int e;
        HIPCHK(hipEventCreate(&ev0));
        HIPCHK(hipEventCreate(&ev1));
        const int64_t nbases = b->off[nsub], ncig = b->cig_off[nsub];
        if ((e = upload(buf[B_SEQ], b->seq, (size_t)nbases, s))) return e;
        if ((e = upload(buf[B_QUAL], b->qual, (size_t)nbases, s))) return e;
        if ((e = upload(buf[B_OFF], b->off, (size_t)nsub + 1, s))) return e;
        if ((e = upload(buf[B_GOFF], b->grp_off, (size_t)ng + 1, s))) return e;
        if ((e = upload(buf[B_GREF], b->grp_ref, (size_t)ng, s))) return e;
        if ((e = upload(buf[B_CIGOFF], b->cig_off, (size_t)nsub + 1, s))) return e;
        for (int k : {B_MAPPED, B_STRAND, B_POS, B_SCORE, B_NCIG})
            if ((e = buf[k].ensure((size_t)nsub * sizeof(int32_t)))) return e;
        if ((e = buf[B_CIG].ensure((size_t)ncig * sizeof(uint32_t)))) return e;
        CcsDev D;
        D.p = p;
        D.seq = buf[B_SEQ].as<uint8_t>(), D.qual = buf[B_QUAL].as<uint8_t>(), D.off = buf[B_OFF].as<int64_t>();
        D.grp_off = buf[B_GOFF].as<int32_t>(), D.grp_ref = buf[B_GREF].as<int32_t>(), D.cig_off = buf[B_CIGOFF].as<int64_t>();
        D.mapped = buf[B_MAPPED].as<int32_t>(), D.strand = buf[B_STRAND].as<int32_t>(), D.pos = buf[B_POS].as<int32_t>();
        D.score = buf[B_SCORE].as<int32_t>(), D.n_cigar = buf[B_NCIG].as<int32_t>(), D.cigar = buf[B_CIG].as<uint32_t>();
        if (do_map) {
            const int np = (int)psub.size(), W = 2 * p.w + 1;
            HIPCHK(hipMemsetAsync(buf[B_MAPPED].p, 0, (size_t)nsub * sizeof(int32_t), s));
            HIPCHK(hipMemsetAsync(buf[B_STRAND].p, 0, (size_t)nsub * sizeof(int32_t), s));
            HIPCHK(hipMemsetAsync(buf[B_POS].p, 0, (size_t)nsub * sizeof(int32_t), s));
            HIPCHK(hipMemsetAsync(buf[B_SCORE].p, 0, (size_t)nsub * sizeof(int32_t), s));
            HIPCHK(hipMemsetAsync(buf[B_NCIG].p, 0, (size_t)nsub * sizeof(int32_t), s));
            std::vector<int64_t> boff((size_t)np + 1, 0), doff((size_t)np, 0);
            for (int k = 0; k < np; ++k)
                boff[k + 1] = boff[k] + 2 * ((int64_t)n_buckets((int)len_of(b, pref[k]), (int)len_of(b, psub[k]), p.w) + 1);
            if ((e = upload(buf[B_PSUB], psub.data(), (size_t)np, s))) return e;
            if ((e = upload(buf[B_PREF], pref.data(), (size_t)np, s))) return e;
            if ((e = upload(buf[B_BOFF], boff.data(), (size_t)np, s))) return e;
            if ((e = buf[B_BSUM].ensure((size_t)boff[np] * sizeof(uint32_t)))) return e;
            if ((e = buf[B_BKEY].ensure((size_t)boff[np] * sizeof(uint64_t)))) return e;
            if ((e = buf[B_CENTRE].ensure((size_t)np * sizeof(Centre)))) return e;
            HIPCHK(hipMemsetAsync(buf[B_BSUM].p, 0, (size_t)boff[np] * sizeof(uint32_t), s));
            HIPCHK(hipMemsetAsync(buf[B_BKEY].p, 0, (size_t)boff[np] * sizeof(uint64_t), s));
            CcsMapDev M;
            M.n_pairs = np;
            M.pair_sub = buf[B_PSUB].as<int32_t>(), M.pair_ref = buf[B_PREF].as<int32_t>();
            M.bsum = buf[B_BSUM].as<uint32_t>(), M.bkey = buf[B_BKEY].as<uint64_t>(), M.b_off = buf[B_BOFF].as<int64_t>();
            M.centre = buf[B_CENTRE].as<Centre>();
            M.dir = nullptr, M.dir_off = nullptr, M.first = 0, M.count = 0;
            if ((e = timed([&]() { return ccs_seeds_launch(D, M, s); }))) return e;
            // the alignments, in chunks whose direction slabs fit the budget
            const int64_t budget = 1ll << 30;
            for (int k0 = 0; k0 < np;) {
                int k1 = k0;
                int64_t bytes = 0;
                while (k1 < np && (k1 == k0 || bytes + len_of(b, pref[k1]) * W <= budget) && k1 - k0 < 65535) {
                    doff[k1] = bytes;
                    bytes += ((len_of(b, pref[k1]) * W + 15) / 16) * 16;
                    ++k1;
                }
                if ((e = buf[B_DIR].ensure((size_t)bytes))) return e;
                if ((e = upload(buf[B_DIROFF], doff.data(), (size_t)np, s))) return e;
                M.dir = buf[B_DIR].as<uint8_t>(), M.dir_off = buf[B_DIROFF].as<int64_t>(), M.first = k0, M.count = k1 - k0;
                if ((e = timed([&]() { return ccs_align_launch(D, M, s); }))) return e;
                k0 = k1;
            }
            if ((e = download(A->mapped, buf[B_MAPPED], (size_t)nsub, s))) return e;
            if ((e = download(A->strand, buf[B_STRAND], (size_t)nsub, s))) return e;
            if ((e = download(A->pos, buf[B_POS], (size_t)nsub, s))) return e;
            if ((e = download(A->score, buf[B_SCORE], (size_t)nsub, s))) return e;
            if ((e = download(A->n_cigar, buf[B_NCIG], (size_t)nsub, s))) return e;
            HIPCHK(hipStreamSynchronize(s));
            for (int q : psub)
                if (A->mapped[q] && (e = download(A->cigar + b->cig_off[q], buf[B_CIG], (size_t)A->n_cigar[q], s, (size_t)b->cig_off[q])))
                    return e;
            HIPCHK(hipStreamSynchronize(s));
        } else {
            // pr_ccs_cns: the alignments are the caller's; a count beyond its slot is malformed
            std::vector<int32_t> ncg(A->n_cigar, A->n_cigar + nsub);
            for (int q = 0; q < nsub; ++q)
                if (ncg[q] < 0 || ncg[q] > b->cig_off[q + 1] - b->cig_off[q]) ncg[q] = 0;
            if ((e = upload(buf[B_MAPPED], A->mapped, (size_t)nsub, s))) return e;
            if ((e = upload(buf[B_STRAND], A->strand, (size_t)nsub, s))) return e;
            if ((e = upload(buf[B_POS], A->pos, (size_t)nsub, s))) return e;
            if ((e = upload(buf[B_NCIG], ncg.data(), (size_t)nsub, s))) return e;
            if ((e = upload(buf[B_CIG], A->cigar, (size_t)ncig, s))) return e;
            HIPCHK(hipStreamSynchronize(s));   // ncg is the stack's
        }
        if (!O) return 0;
        const int64_t nout = b->out_off[ng];
        if ((e = upload(buf[B_OUTOFF], b->out_off, (size_t)ng + 1, s))) return e;
        for (int k : {B_OSEQ, B_OQUAL, B_OTRACE})
            if ((e = buf[k].ensure((size_t)nout))) return e;
        for (int k : {B_OST, B_OSL, B_OTL}) {
            if ((e = buf[k].ensure((size_t)ng * sizeof(int32_t)))) return e;
            HIPCHK(hipMemsetAsync(buf[k].p, 0, (size_t)ng * sizeof(int32_t), s));
        }
        if ((e = buf[B_OPR].ensure((size_t)ncig * sizeof(int32_t)))) return e;
        if ((e = buf[B_OPQ].ensure((size_t)ncig * sizeof(int32_t)))) return e;
        CcsCnsDev C;
        C.op_r = buf[B_OPR].as<int32_t>(), C.op_q = buf[B_OPQ].as<int32_t>();
        C.out_off = buf[B_OUTOFF].as<int64_t>();
        C.seq = buf[B_OSEQ].as<uint8_t>(), C.qual = buf[B_OQUAL].as<uint8_t>(), C.trace = buf[B_OTRACE].as<uint8_t>();
        C.status = buf[B_OST].as<int32_t>(), C.seq_len = buf[B_OSL].as<int32_t>(), C.trace_len = buf[B_OTL].as<int32_t>();
        const int64_t budget = (1ll << 30) / (int64_t)sizeof(ColEnt);
        std::vector<int64_t> soff;
        for (size_t k0 = 0; k0 < glist.size();) {
            size_t k1 = k0;
            int64_t ents = 0;
            soff.clear();
            while (k1 < glist.size() && k1 - k0 < 65535) {
                const int g = glist[k1];
                const int64_t need = (int64_t)(b->grp_off[g + 1] - b->grp_off[g] - 1) * len_of(b, b->grp_ref[g]);
                if (k1 > k0 && ents + need > budget) break;
                soff.push_back(ents);
                ents += need;
                ++k1;
            }
            if ((e = buf[B_SLAB].ensure((size_t)ents * sizeof(ColEnt)))) return e;
            if ((e = upload(buf[B_SLABOFF], soff.data(), soff.size(), s))) return e;
            if ((e = upload(buf[B_GLIST], glist.data() + k0, k1 - k0, s))) return e;
            C.n = (int32_t)(k1 - k0), C.glist = buf[B_GLIST].as<int32_t>();
            C.slab = buf[B_SLAB].as<ColEnt>(), C.slab_off = buf[B_SLABOFF].as<int64_t>();
            if ((e = timed([&]() { return ccs_cns_launch(D, C, s); }))) return e;
            k0 = k1;
        }
        std::vector<int32_t> st((size_t)ng), sl((size_t)ng), tl((size_t)ng);
        if ((e = download(st.data(), buf[B_OST], (size_t)ng, s))) return e;
        if ((e = download(sl.data(), buf[B_OSL], (size_t)ng, s))) return e;
        if ((e = download(tl.data(), buf[B_OTL], (size_t)ng, s))) return e;
        HIPCHK(hipStreamSynchronize(s));
        for (int g : glist) {
            O->status[g] = st[g], O->seq_len[g] = sl[g], O->trace_len[g] = tl[g];
            const size_t at = (size_t)b->out_off[g];
            if ((e = download(O->seq + at, buf[B_OSEQ], (size_t)sl[g], s, at))) return e;
            if ((e = download(O->qual + at, buf[B_OQUAL], (size_t)sl[g], s, at))) return e;
            if ((e = download(O->trace + at, buf[B_OTRACE], (size_t)tl[g], s, at))) return e;
        }
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(s);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (int k = 0; k < B_COUNT; ++k) buf[k].release();
    return rc;
}

int entry(pr_ctx *ctx, const pr_ccs_params *p, const pr_ccs_batch *b, int n_threads, pr_ccs_alns *A, bool do_map, pr_ccs_out *O,
          bool want_out) {
    int rc = check_params(p);
    if (!rc) rc = check_batch(b, want_out);
    if (rc) return rc;
    if (!b->n_groups) return 0;
    if (!A || !A->mapped || !A->strand || !A->pos || !A->score || !A->n_cigar || !A->cigar)
        return pr_set_error(PR_ERR_ARG, "ccs: no alignment arrays");
    if (want_out && (!O || !O->status || !O->seq_len || !O->trace_len || !O->seq || !O->qual || !O->trace))
        return pr_set_error(PR_ERR_ARG, "ccs: no output arrays");
    if (do_map) clear_alns(b, A);
    return ctx ? run_gpu(ctx, *p, b, A, do_map, want_out ? O : nullptr) : run_host(*p, b, n_threads, A, do_map, want_out ? O : nullptr);
}

}   // namespace

extern "C" void pr_ccs_params_default(pr_ccs_params *p) {
    if (!p) return;
    // ccseq:97 bwa_opt: -k 9 -w 300 -A 5 -B 11 -O 2,1 -E 4,3; ccseq:214-215 and Seq.pm's class defaults
    *p = pr_ccs_params{9, 300, 5, 11, 2, 1, 4, 3, 1, 50, 33, 0, 0.001};
}

extern "C" int pr_ccs_group(int32_t n, const char *ids, const int64_t *id_off, const int32_t *len, int32_t *role,
                            int32_t *group, int32_t *n_groups, int32_t *bad_kind, int32_t *bad_index) {
    if (n < 0 || !n_groups || !bad_kind || !bad_index || (n && (!ids || !id_off || !len || !role || !group)))
        return pr_set_error(PR_ERR_ARG, "ccs: bad id list");
    for (int32_t r = 0; r < n; ++r)
        if (id_off[r + 1] < id_off[r]) return pr_set_error(PR_ERR_ARG, "ccs: id offsets not monotone");
    const int ng = group_ids(n, ids, id_off, len, role, group, bad_kind, bad_index);
    *n_groups = ng < 0 ? 0 : ng;
    return 0;
}

extern "C" int pr_ccs_last_ms(pr_ctx *ctx, double *ms) {
    if (!ctx || !ms) return pr_set_error(PR_ERR_ARG, "ccs: no context");
    *ms = ctx->ms_ccs;
    return 0;
}

extern "C" int pr_ccs_run(pr_ctx *ctx, const pr_ccs_params *p, const pr_ccs_batch *b, int n_threads, pr_ccs_alns *alns,
                          pr_ccs_out *out) {
    return entry(ctx, p, b, n_threads, alns, true, out, true);
}

extern "C" int pr_ccs_map(pr_ctx *ctx, const pr_ccs_params *p, const pr_ccs_batch *b, int n_threads, pr_ccs_alns *alns) {
    return entry(ctx, p, b, n_threads, alns, true, nullptr, false);
}

extern "C" int pr_ccs_cns(pr_ctx *ctx, const pr_ccs_params *p, const pr_ccs_batch *b, int n_threads, const pr_ccs_alns *alns,
                          pr_ccs_out *out) {
    return entry(ctx, p, b, n_threads, const_cast<pr_ccs_alns *>(alns), false, out, true);
}

// The siamaera entries of the C-ABI (include/prgpu.h): bin/siamaera's blastn calls (:490-579)
// and its per-read decision (:250-474), on the host (threads over reads) or with the self-
// alignments on the device (siam_kernels.hip).  Identity threshold, culling and the decision
// are the same host code (siam_core.h) on both paths.
#include <atomic>
#include <thread>

#include "ctx.h"
#include "siam_dev.h"

using namespace prgpu::siam;

namespace {

thread_local std::vector<pr_siam_hsp> g_hsps;   // the records pr_siam_hsps_* return

int check_aligner(const pr_siam_aligner *al) {
    if (!al) return pr_set_error(PR_ERR_ARG, "siamaera: no aligner options");
    if (al->a <= 0 || al->b < 0 || al->o < 0 || al->e <= 0 || al->word < 1)
        return pr_set_error(PR_ERR_ARG, "siamaera: aligner needs a > 0, b >= 0, o >= 0, e > 0, word >= 1");
    if (al->w < 0 || al->w > 31) return pr_set_error(PR_ERR_ARG, "siamaera: band w must be 0 .. 31");
    return 0;
}

int check_batch(const uint8_t *seq, const int64_t *off, int32_t n) {
    if (n < 0 || (n && (!seq || !off))) return pr_set_error(PR_ERR_ARG, "siamaera: bad batch");
    for (int32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return pr_set_error(PR_ERR_ARG, "siamaera: offsets not monotone");
    return 0;
}

int n_workers(int n_threads, int64_t n) {
    int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(nt, 64));
    return (int)std::min<int64_t>(nt, std::max<int64_t>(n, 1));
}

using Lists = std::vector<std::vector<pr_siam_hsp>>;

// the alignments produced for reads idx[k] of the batch, on the host
void produce_batch_host(const pr_siam_aligner &al, const uint8_t *seq, const int64_t *off, const std::vector<int32_t> &idx,
                        int n_threads, Lists &prod, int32_t *status) {
    prod.assign(idx.size(), {});
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t k; (k = next.fetch_add(1)) < idx.size();) {
            const int32_t r = idx[k];
            status[r] |= produce_host(al, seq + off[r], off[r + 1] - off[r], r, prod[k]);
        }
    };
    const int nt = n_workers(n_threads, (int64_t)idx.size());
    if (nt == 1) {
        work();
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work);
        for (auto &x : th) x.join();
    }
}

// the same on the device, in chunks of reads that bound the seed scratch
int produce_batch_gpu(pr_ctx *c, const pr_siam_aligner &al, const uint8_t *seq, const int64_t *off,
                      const std::vector<int32_t> &idx, Lists &prod, int32_t *status) {
    prod.assign(idx.size(), {});
    if (idx.empty()) return 0;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t max_reads = 4096;
    const int64_t max_bases = 1ll << 28;
    DevBuf b_seq, b_off, b_seeds, b_ns, b_hsps, b_nh, b_st, b_pl, b_po;
    for (DevBuf *b : {&b_seq, &b_off, &b_seeds, &b_ns, &b_hsps, &b_nh, &b_st, &b_pl, &b_po}) b->grp = "siam";
    auto release = [&]() {
        for (DevBuf *b : {&b_seq, &b_off, &b_seeds, &b_ns, &b_hsps, &b_nh, &b_st, &b_pl, &b_po}) b->release();
    };
    hipEvent_t ev0, ev1;
    HIPCHK(hipEventCreate(&ev0));
    HIPCHK(hipEventCreate(&ev1));
    std::vector<uint8_t> pool;
    std::vector<int64_t> coff, poff;
    std::vector<pr_siam_hsp> hs;
    std::vector<int32_t> nh, st;
    int rc = 0;
    for (size_t k0 = 0; k0 < idx.size() && !rc;) {
        size_t k1 = k0;
        pool.clear();
        coff.assign(1, 0);
        while (k1 < idx.size() && k1 - k0 < max_reads && (k1 == k0 || (int64_t)pool.size() < max_bases)) {
            const int32_t r = idx[k1++];
            pool.insert(pool.end(), seq + off[r], seq + off[r + 1]);
            coff.push_back((int64_t)pool.size());
        }
        const size_t m = k1 - k0;
        auto chunk = [&]() -> int {
            int e;
            if ((e = upload(b_seq, pool.data(), pool.size(), s))) return e;
            if ((e = upload(b_off, coff.data(), coff.size(), s))) return e;
            poff.assign(m + 1, 0);
            for (size_t k = 0; k < m; ++k) {
                const int64_t len = coff[k + 1] - coff[k];
                poff[k + 1] = poff[k] + (len <= PR_SIAM_MAX_LEN ? 8 * (int64_t)plane_words((int)len) : 0);
            }
            if ((e = upload(b_po, poff.data(), poff.size(), s))) return e;
            if ((e = b_pl.ensure((size_t)poff[m] * sizeof(uint64_t)))) return e;
            if ((e = b_seeds.ensure(m * PR_SIAM_MAX_SEEDS * sizeof(Seed)))) return e;
            if ((e = b_ns.ensure(m * sizeof(int32_t)))) return e;
            if ((e = b_hsps.ensure(m * PR_SIAM_MAX_HSPS * sizeof(pr_siam_hsp)))) return e;
            if ((e = b_nh.ensure(m * sizeof(int32_t)))) return e;
            if ((e = b_st.ensure(m * sizeof(int32_t)))) return e;
            SiamDev D;
            D.n = (int32_t)m;
            D.off = b_off.as<int64_t>();
            D.seq = b_seq.as<uint8_t>();
            D.planes = b_pl.as<uint64_t>();
            D.plane_off = b_po.as<int64_t>();
            D.seeds = b_seeds.as<Seed>();
            D.n_seeds = b_ns.as<int32_t>();
            D.hsps = b_hsps.as<pr_siam_hsp>();
            D.n_hsps = b_nh.as<int32_t>();
            D.status = b_st.as<int32_t>();
            D.al = al;
            HIPCHK(hipEventRecord(ev0, s));
            HIPCHK((hipError_t)siam_launch(D, s));
            HIPCHK(hipEventRecord(ev1, s));
            hs.resize(m * PR_SIAM_MAX_HSPS);
            nh.resize(m);
            st.resize(m);
            if ((e = download(nh.data(), b_nh, m, s))) return e;
            if ((e = download(st.data(), b_st, m, s))) return e;
            if ((e = download(hs.data(), b_hsps, hs.size(), s))) return e;
            HIPCHK(hipStreamSynchronize(s));
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) c->ms_siam += ms;
            return 0;
        };
        rc = chunk();
        if (!rc) {
            for (size_t k = 0; k < m; ++k) {
                const int32_t r = idx[k0 + k];
                status[r] |= st[k];
                const pr_siam_hsp *h = hs.data() + k * PR_SIAM_MAX_HSPS;
                prod[k0 + k].assign(h, h + nh[k]);
                for (pr_siam_hsp &x : prod[k0 + k]) x.read = r;
            }
        }
        k0 = k1;
    }
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    release();
    return rc;
}

int produce_batch(pr_ctx *c, const pr_siam_aligner &al, const uint8_t *seq, const int64_t *off,
                  const std::vector<int32_t> &idx, int n_threads, Lists &prod, int32_t *status) {
    if (c) return produce_batch_gpu(c, al, seq, off, idx, prod, status);
    produce_batch_host(al, seq, off, idx, n_threads, prod, status);
    return 0;
}

int hsps_entry(pr_ctx *c, const pr_siam_aligner *al, double min_idy, const uint8_t *seq, const int64_t *off, int32_t n,
               int n_threads, const pr_siam_hsp **hsps, int64_t *n_hsps, int32_t *status) {
    int rc = check_aligner(al);
    if (rc) return rc;
    if ((rc = check_batch(seq, off, n))) return rc;
    if (!hsps || !n_hsps || (n && !status)) return pr_set_error(PR_ERR_ARG, "siamaera: no output");
    std::vector<int32_t> idx((size_t)n);
    for (int32_t i = 0; i < n; ++i) idx[i] = i, status[i] = 0;
    Lists prod;
    if (c) c->ms_siam = 0.f;
    if ((rc = produce_batch(c, *al, seq, off, idx, n_threads, prod, status))) return rc;
    g_hsps.clear();
    for (int32_t i = 0; i < n; ++i)
        if (!status[i]) select_hsps(prod[i].data(), (int)prod[i].size(), min_idy, g_hsps);
    *hsps = g_hsps.data();
    *n_hsps = (int64_t)g_hsps.size();
    return 0;
}

}   // namespace

extern "C" void pr_siam_params_default(pr_siam_params *p) {
    if (!p) return;
    p->seq_min_len = 150;
    p->term_ignore_len = 10;
    p->trim = 5;
    p->filter_inconclusive = 1;
    p->aln_min_idy = 97.5;
    // blast(): -penalty -4 -gapopen 3 -gapextend 2 -xdrop_gap_final 25, megablast word 28
    p->pass1 = pr_siam_aligner{1, 4, 3, 2, 31, 25, 28};
    // reblast(): megablast's defaults (-penalty -2, linear gaps restated as o 0, e 3), -xdrop_gap_final 100
    p->pass2 = pr_siam_aligner{1, 2, 0, 3, 31, 100, 28};
}

extern "C" int pr_siam_hsps_host(const pr_siam_aligner *al, double min_idy, const uint8_t *seq, const int64_t *off,
                                 int32_t n, int n_threads, const pr_siam_hsp **hsps, int64_t *n_hsps, int32_t *status) {
    return hsps_entry(nullptr, al, min_idy, seq, off, n, n_threads, hsps, n_hsps, status);
}

extern "C" int pr_siam_hsps_gpu(pr_ctx *ctx, const pr_siam_aligner *al, double min_idy, const uint8_t *seq,
                                const int64_t *off, int32_t n, const pr_siam_hsp **hsps, int64_t *n_hsps,
                                int32_t *status) {
    if (!ctx) return pr_set_error(PR_ERR_ARG, "siamaera: no context");
    return hsps_entry(ctx, al, min_idy, seq, off, n, 0, hsps, n_hsps, status);
}

extern "C" int pr_siam_decide(const pr_siam_params *p, int32_t len, const pr_siam_hsp *h1, int32_t n1,
                              const pr_siam_hsp *h2, int32_t n2, pr_siam_decision *out, int32_t *inconclusive) {
    if (!p || !out || !inconclusive || n1 < 0 || n2 < 0 || (n1 && !h1) || (n2 && !h2))
        return pr_set_error(PR_ERR_ARG, "siamaera: bad decision input");
    std::vector<pr_siam_hsp> b(h1, h1 + n1), b2(h2, h2 + n2);
    *out = pr_siam_decision{PR_SIAM_KEEP, 0, len};
    *inconclusive = 0;
    if (len < p->seq_min_len || b.empty()) return 0;
    after_pass1(*p, len, b);
    *out = decide(*p, len, b, b2, inconclusive);
    return 0;
}

extern "C" int pr_siam_run(pr_ctx *ctx, const pr_siam_params *p, const uint8_t *seq, const int64_t *off, int32_t n,
                           int n_threads, pr_siam_decision *out, int32_t *status, int64_t *summary) {
    if (!p) return pr_set_error(PR_ERR_ARG, "siamaera: no parameters");
    int rc = check_aligner(&p->pass1);
    if (!rc) rc = check_aligner(&p->pass2);
    if (!rc) rc = check_batch(seq, off, n);
    if (rc) return rc;
    if (n && (!out || !status)) return pr_set_error(PR_ERR_ARG, "siamaera: no output");
    if (ctx) ctx->ms_siam = 0.f;
    std::vector<int32_t> idx;
    for (int32_t i = 0; i < n; ++i) {
        status[i] = 0;
        out[i] = pr_siam_decision{PR_SIAM_KEEP, 0, (int32_t)std::min<int64_t>(off[i + 1] - off[i], INT32_MAX)};
        if (off[i + 1] - off[i] >= p->seq_min_len) idx.push_back(i);   // siamaera:258
    }
    Lists prod;
    if ((rc = produce_batch(ctx, p->pass1, seq, off, idx, n_threads, prod, status))) return rc;
    // pass 1's lists after the identity threshold, culling and the first filter (:266-312)
    Lists b(idx.size());
    std::vector<int32_t> again, again_k;
    for (size_t k = 0; k < idx.size(); ++k) {
        const int32_t r = idx[k];
        if (status[r]) continue;
        select_hsps(prod[k].data(), (int)prod[k].size(), p->aln_min_idy, b[k]);
        if (b[k].empty()) continue;
        if (after_pass1(*p, (int)(off[r + 1] - off[r]), b[k])) again.push_back(r), again_k.push_back((int32_t)k);
    }
    Lists prod2, b2(idx.size());
    if ((rc = produce_batch(ctx, p->pass2, seq, off, again, n_threads, prod2, status))) return rc;
    for (size_t q = 0; q < again.size(); ++q)
        if (!status[again[q]])
            select_hsps(prod2[q].data(), (int)prod2[q].size(), p->aln_min_idy - 2, b2[again_k[q]]);
    int64_t sum[4] = {n, 0, 0, 0};
    for (size_t k = 0; k < idx.size(); ++k) {
        const int32_t r = idx[k];
        if (status[r]) {
            ++sum[3];
            continue;
        }
        if (b[k].empty()) continue;
        int inc = 0;
        out[r] = decide(*p, (int)(off[r + 1] - off[r]), b[k], b2[k], &inc);
        sum[1] += out[r].action == PR_SIAM_TRIM;
        sum[2] += inc;
    }
    if (summary)
        for (int q = 0; q < 4; ++q) summary[q] = sum[q];
    return 0;
}

extern "C" int pr_siam_last_ms(pr_ctx *ctx, double *ms) {
    if (!ctx || !ms) return pr_set_error(PR_ERR_ARG, "siamaera: no context");
    *ms = ctx->ms_siam;
    return 0;
}

extern "C" int pr_siam_seeds_host(const uint8_t *seq, int32_t len, int32_t word, int32_t *out, int32_t cap, int32_t *n) {
    if (len < 0 || (len && !seq) || word < 1 || !n || cap < 0 || (cap && !out))
        return pr_set_error(PR_ERR_ARG, "siamaera: bad seed query");
    std::vector<Seed> v;
    seeds_host(seq, len, word, v);
    sort_seeds(v);
    *n = (int32_t)v.size();
    for (int32_t k = 0; k < cap && k < *n; ++k) out[3 * k] = v[k].i, out[3 * k + 1] = v[k].p, out[3 * k + 2] = v[k].len;
    return 0;
}

extern "C" int pr_siam_extend_host(const pr_siam_aligner *al, const uint8_t *q, int32_t qlen, const uint8_t *t,
                                   int32_t tlen, int32_t h0, int32_t *out) {
    int rc = check_aligner(al);
    if (rc) return rc;
    if (qlen < 0 || tlen < 0 || (qlen && !q) || (tlen && !t) || !out)
        return pr_set_error(PR_ERR_ARG, "siamaera: bad extension");
    const Ext e = extend_host(*al, qlen, [&](int j) { return (int)q[j]; }, tlen, [&](int i) { return (int)t[i]; }, h0);
    out[0] = e.score, out[1] = e.qle, out[2] = e.tle, out[3] = e.m, out[4] = e.c;
    return 0;
}

extern "C" int pr_siam_extend_gpu(pr_ctx *c, const pr_siam_aligner *al, const uint8_t *q, const int64_t *q_off,
                                  const uint8_t *t, const int64_t *t_off, const int32_t *h0, int32_t n, int32_t *out) {
    int rc = check_aligner(al);
    if (rc) return rc;
    if (!c || n < 0 || (n && (!q_off || !t_off || !h0 || !out))) return pr_set_error(PR_ERR_ARG, "siamaera: bad extension batch");
    if (!n) return 0;
    for (int32_t k = 0; k < n; ++k)
        if (q_off[k + 1] < q_off[k] || t_off[k + 1] < t_off[k] || q_off[k + 1] - q_off[k] > PR_SIAM_MAX_LEN ||
            t_off[k + 1] - t_off[k] > PR_SIAM_MAX_LEN)
            return pr_set_error(PR_ERR_ARG, "siamaera: bad extension offsets");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevBuf bq, bt, bqo, bto, bh, bo;
    DevBuf *all[] = {&bq, &bt, &bqo, &bto, &bh, &bo};
    for (DevBuf *b : all) b->grp = "siam";
    auto run = [&]() -> int {
        int e;
        if ((e = upload(bq, q, (size_t)q_off[n], s))) return e;
        if ((e = upload(bt, t, (size_t)t_off[n], s))) return e;
        if ((e = upload(bqo, q_off, (size_t)n + 1, s))) return e;
        if ((e = upload(bto, t_off, (size_t)n + 1, s))) return e;
        if ((e = upload(bh, h0, (size_t)n, s))) return e;
        if ((e = bo.ensure(sizeof(int32_t) * 5 * (size_t)n))) return e;
        SiamPairs D;
        D.n = n;
        D.q = bq.as<uint8_t>();
        D.t = bt.as<uint8_t>();
        D.q_off = bqo.as<int64_t>();
        D.t_off = bto.as<int64_t>();
        D.h0 = bh.as<int32_t>();
        D.out = bo.as<int32_t>();
        D.al = *al;
        HIPCHK((hipError_t)siam_pairs_launch(D, s));
        if ((e = download(out, bo, 5 * (size_t)n, s))) return e;
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    };
    rc = run();
    for (DevBuf *b : all) b->release();
    return rc;
}

// proovread_amd/csrc/bam_core.h compiled for the host (tests/test_bam_core_host.py): the record
// decoder the device kernels run, driven record by record and "lane" by "lane".
//
// As a shared library: bam_core_decode fills a pr_bam_alns from a record stream; every record
// is decoded from a heap copy of exactly its size and the pools are allocated at exactly their
// sizes, so a read or write past either end is an error a sanitizer sees.
// As a program (main): records of many shapes, built here, against a plain byte-by-byte
// decoder, and every truncation of an aux area; exit status 0 when all agree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../proovread_amd/csrc/bam_core.h"

using namespace prgpu::bam;

static std::string g_error;

extern "C" {

const char *bam_core_last_error() { return g_error.c_str(); }

void bam_core_free(pr_bam_alns *a, int64_t *text_at) {
    void *p[] = {a->rid, a->pos1, a->score, a->flags, a->seq_off, a->lseq, a->cig_off, a->ncig, a->seq, a->qual, a->cig, text_at};
    for (void *x : p) free(x);
    memset(a, 0, sizeof *a);
}

// text_at[i]: offset in recs of record i's AS:Z / AS:H text (its score is left 0), or -1.
// nlanes: the unpack functions are called for lane 0 .. nlanes - 1 in turn, as a lane group would.
int bam_core_decode(const uint8_t *recs, int64_t len, int nlanes, pr_bam_alns *out, int64_t **text_at_out) {
    memset(out, 0, sizeof *out);
    *text_at_out = nullptr;
    std::vector<int64_t> off, so(1, 0), co(1, 0);
    for (int64_t o = 0; o < len;) {
        int64_t next = 0;
        const int e = bam_check_record(recs, len, o, &next);
        if (e) {
            g_error = bam_error_text(e);
            return PR_ERR_ARG;
        }
        const Fixed f = bam_fixed(recs + o);
        off.push_back(o);
        so.push_back(so.back() + f.l_seq);
        co.push_back(co.back() + f.n_cigar);
        o = next;
    }
    const size_t n = off.size();
    auto alloc = [](size_t b) { return malloc(b ? b : 1); };
    out->n = (int64_t)n;
    out->rid = (int32_t *)alloc(4 * n);
    out->pos1 = (int32_t *)alloc(4 * n);
    out->score = (double *)alloc(8 * n);
    out->flags = (uint8_t *)alloc(n);
    out->seq_off = (int64_t *)alloc(8 * n);
    out->lseq = (int32_t *)alloc(4 * n);
    out->cig_off = (int64_t *)alloc(8 * n);
    out->ncig = (int32_t *)alloc(4 * n);
    out->seq = (uint8_t *)alloc((size_t)so.back());
    out->qual = (uint8_t *)alloc((size_t)so.back());
    out->cig = (uint32_t *)alloc(4 * (size_t)co.back());
    out->seq_len = so.back();
    out->cig_len = co.back();
    int64_t *text_at = (int64_t *)alloc(8 * n);
    *text_at_out = text_at;
    int rc = 0;
    for (size_t i = 0; i < n && !rc; ++i) {
        const int64_t size = (i + 1 < n ? off[i + 1] : len) - off[i];
        uint8_t *rec = (uint8_t *)malloc((size_t)size);   // exactly the record
        memcpy(rec, recs + off[i], (size_t)size);
        const Fixed f = bam_fixed(rec);
        double score = 0.0;
        uint32_t fl = 0;
        int32_t text = 0;
        if (bam_aux_walk(bam_aux_at(rec, f), bam_end_of(rec, f), &score, &fl, &text) != BAM_OK) {
            g_error = bam_error_text(BAM_BAD_AUX);
            rc = PR_ERR_SAM;
        } else {
            text_at[i] = (fl & BAM_AS_TEXT) ? off[i] + (bam_aux_at(rec, f) - rec) + text : -1;
            fl = (fl & ~(uint32_t)BAM_AS_TEXT) | bam_seq_flags(rec, f);
            out->rid[i] = f.rid;
            out->pos1[i] = f.pos + 1;
            out->score[i] = score;
            out->flags[i] = (uint8_t)fl;
            out->seq_off[i] = so[i];
            out->lseq[i] = f.l_seq;
            out->cig_off[i] = co[i];
            out->ncig[i] = f.n_cigar;
            for (int lane = 0; lane < nlanes; ++lane) {
                bam_unpack_seq(bam_seq_at(rec, f), f.l_seq, out->seq + so[i], lane, nlanes);
                bam_unpack_qual(bam_qual_at(rec, f), f.l_seq, (fl & PR_ALN_NO_QUAL) != 0, out->qual + so[i], lane, nlanes);
                (void)bam_copy_cigar(bam_cigar_at(rec, f), f.n_cigar, out->cig + co[i], lane, nlanes);
            }
        }
        free(rec);
    }
    if (rc) {
        bam_core_free(out, text_at);
        *text_at_out = nullptr;
    }
    return rc;
}
}

// ---------------------------------------------------------------------------- the program
namespace {

void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k)));
}
void put16(std::vector<uint8_t> &v, uint32_t x) {
    v.push_back((uint8_t)x);
    v.push_back((uint8_t)(x >> 8));
}

uint32_t g_rng = 12345;
uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

std::vector<uint8_t> record(int32_t rid, int32_t pos, int name_len, int n_cig, int l_seq, bool qual,
                            const std::vector<uint8_t> &aux) {
    std::vector<uint8_t> b;
    put32(b, (uint32_t)rid);
    put32(b, (uint32_t)pos);
    b.push_back((uint8_t)name_len);
    b.push_back(60);
    put16(b, 4680);
    put16(b, (uint32_t)n_cig);
    put16(b, 0);
    put32(b, (uint32_t)l_seq);
    put32(b, 0xffffffffu);
    put32(b, 0xffffffffu);
    put32(b, 0);
    for (int k = 0; k + 1 < name_len; ++k) b.push_back((uint8_t)('a' + k));
    b.push_back(0);
    for (int k = 0; k < n_cig; ++k) put32(b, ((rnd() % 300 + 1) << 4) | (rnd() % 9));
    for (int k = 0; k < (l_seq + 1) / 2; ++k) b.push_back((uint8_t)rnd());
    for (int k = 0; k < l_seq; ++k) b.push_back(qual ? (uint8_t)(rnd() % 94) : (uint8_t)0xFF);
    b.insert(b.end(), aux.begin(), aux.end());
    std::vector<uint8_t> r;
    put32(r, (uint32_t)b.size());
    r.insert(r.end(), b.begin(), b.end());
    return r;
}

void tag(std::vector<uint8_t> &a, const char *name, char type) {
    a.push_back((uint8_t)name[0]);
    a.push_back((uint8_t)name[1]);
    a.push_back((uint8_t)type);
}

// every skip type, then an AS of the given type
std::vector<uint8_t> aux_fields(char as_type, bool skips, bool twice) {
    std::vector<uint8_t> a;
    if (skips) {
        tag(a, "XA", 'A'); a.push_back('x');
        tag(a, "Xc", 'c'); a.push_back(0x80);
        tag(a, "XC", 'C'); a.push_back(200);
        tag(a, "Xs", 's'); put16(a, 0x8001);
        tag(a, "XS", 'S'); put16(a, 60000);
        tag(a, "Xi", 'i'); put32(a, 0x80000001u);
        tag(a, "XI", 'I'); put32(a, 4000000000u);
        tag(a, "Xf", 'f'); put32(a, 0x40490fdbu);
        tag(a, "XZ", 'Z'); a.push_back('h'); a.push_back('i'); a.push_back(0);
        tag(a, "XE", 'Z'); a.push_back(0);
        tag(a, "XH", 'H'); a.push_back('1'); a.push_back('F'); a.push_back(0);
        const char sub[] = "cCsSiIf";
        const int es[] = {1, 1, 2, 2, 4, 4, 4};
        for (int k = 0; k < 7; ++k) {
            tag(a, "XB", 'B');
            a.push_back((uint8_t)sub[k]);
            put32(a, 3);
            for (int j = 0; j < 3 * es[k]; ++j) a.push_back((uint8_t)rnd());
        }
        tag(a, "X0", 'B'); a.push_back('i'); put32(a, 0);
    }
    for (int rep = 0; rep < (twice ? 2 : 1); ++rep) {
        const char t = rep ? 'c' : as_type;
        if (!t) break;
        tag(a, "AS", t);
        switch (t) {
            case 'c': a.push_back((uint8_t)-7); break;
            case 'C': a.push_back(250); break;
            case 's': put16(a, (uint32_t)(uint16_t)-300); break;
            case 'S': put16(a, 65000); break;
            case 'i': put32(a, (uint32_t)-100000); break;
            case 'I': put32(a, 3000000000u); break;
            case 'f': put32(a, 0x42f6e979u); break;   // 123.456
            default: a.push_back('4'); a.push_back('2'); a.push_back(0); break;   // Z
        }
    }
    return a;
}

// the plain decoder: one record, byte by byte
struct Plain {
    int32_t rid, pos1, lseq, ncig;
    double score;
    uint32_t flags;
    bool text;
    std::string seq, qual;
    std::vector<uint32_t> cig;
};
Plain plain(const uint8_t *r) {
    Plain p;
    memcpy(&p.rid, r + 4, 4);
    int32_t pos, bs;
    memcpy(&bs, r, 4);
    memcpy(&pos, r + 8, 4);
    p.pos1 = pos + 1;
    uint16_t nc;
    memcpy(&nc, r + 16, 2);
    p.ncig = nc;
    memcpy(&p.lseq, r + 20, 4);
    const uint8_t *c = r + 36 + r[12];
    for (int k = 0; k < p.ncig; ++k) {
        uint32_t x;
        memcpy(&x, c + 4 * k, 4);
        p.cig.push_back(x);
    }
    const uint8_t *sb = c + 4 * p.ncig, *qb = sb + (p.lseq + 1) / 2;
    p.flags = p.lseq == 0 ? PR_ALN_NO_SEQ : 0;
    const bool nq = p.lseq && qb[0] == 0xFF;
    if (nq) p.flags |= PR_ALN_NO_QUAL;
    for (int k = 0; k < p.lseq; ++k) {
        p.seq.push_back("=ACMGRSVTWYHKDBN"[(sb[k >> 1] >> (4 * (1 - (k & 1)))) & 15]);
        p.qual.push_back(nq ? '!' : (char)(uint8_t)(qb[k] + 33));
    }
    p.score = 0.0;
    p.text = false;
    const uint8_t *a = qb + p.lseq, *end = r + 4 + bs;
    while (a < end) {   // well-formed records only
        const bool as = a[0] == 'A' && a[1] == 'S';
        const char t = (char)a[2];
        a += 3;
        double v = 0.0;
        int w = 0;
        bool text = false;
        if (t == 'A') w = 1;
        else if (t == 'c') v = (int8_t)a[0], w = 1;
        else if (t == 'C') v = a[0], w = 1;
        else if (t == 's') { int16_t x; memcpy(&x, a, 2); v = x; w = 2; }
        else if (t == 'S') { uint16_t x; memcpy(&x, a, 2); v = x; w = 2; }
        else if (t == 'i') { int32_t x; memcpy(&x, a, 4); v = x; w = 4; }
        else if (t == 'I') { uint32_t x; memcpy(&x, a, 4); v = x; w = 4; }
        else if (t == 'f') { float x; memcpy(&x, a, 4); v = x; w = 4; }
        else if (t == 'Z' || t == 'H') { w = (int)strlen((const char *)a) + 1; text = true; }
        else {
            int32_t cnt;
            memcpy(&cnt, a + 1, 4);
            const char st = (char)a[0];
            w = 5 + cnt * ((st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4);
        }
        if (as && t != 'A' && t != 'B') {
            p.score = v;
            p.text = text;
            p.flags |= PR_ALN_HAS_SCORE;
        }
        a += w;
    }
    return p;
}

int fails = 0;
#define EXPECT(c)                                              \
    do {                                                       \
        if (!(c)) {                                            \
            ++fails;                                           \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                      \
    } while (0)

void check_stream(const std::vector<std::vector<uint8_t>> &recs) {
    std::vector<uint8_t> all;
    for (auto &r : recs) all.insert(all.end(), r.begin(), r.end());
    uint8_t *stream = (uint8_t *)malloc(all.size() ? all.size() : 1);   // exactly the stream
    if (!all.empty()) memcpy(stream, all.data(), all.size());
    for (int nlanes : {1, 16}) {
        pr_bam_alns A;
        int64_t *text_at = nullptr;
        const int rc = bam_core_decode(stream, (int64_t)all.size(), nlanes, &A, &text_at);
        EXPECT(rc == 0);
        if (rc) continue;
        EXPECT(A.n == (int64_t)recs.size());
        int64_t so = 0, co = 0;
        for (size_t i = 0; i < recs.size(); ++i) {
            const Plain p = plain(recs[i].data());
            EXPECT(A.rid[i] == p.rid && A.pos1[i] == p.pos1 && A.lseq[i] == p.lseq && A.ncig[i] == p.ncig);
            EXPECT(A.flags[i] == p.flags);
            EXPECT((text_at[i] >= 0) == p.text);
            EXPECT(A.score[i] == p.score);
            EXPECT(A.seq_off[i] == so && A.cig_off[i] == co);
            EXPECT(memcmp(A.seq + so, p.seq.data(), p.seq.size()) == 0);
            EXPECT(memcmp(A.qual + so, p.qual.data(), p.qual.size()) == 0);
            EXPECT(p.cig.empty() || memcmp(A.cig + co, p.cig.data(), 4 * p.cig.size()) == 0);
            so += p.lseq;
            co += p.ncig;
        }
        EXPECT(A.seq_len == so && A.cig_len == co);
        bam_core_free(&A, text_at);
    }
    free(stream);
}

}   // namespace

int main() {
    const int lseqs[] = {0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257};
    const int ncigs[] = {0, 1, 3, 40};
    const char as_types[] = {0, 'c', 'C', 's', 'S', 'i', 'I', 'f', 'Z'};
    std::vector<std::vector<uint8_t>> recs;
    int k = 0;
    for (int l : lseqs)
        for (int name = 1; name <= 8; ++name)
            for (int nc : ncigs) {
                const char t = as_types[k % 9];
                recs.push_back(record(k % 5 == 4 ? -1 : k % 3, k % 5 == 4 ? -1 : 10 * k, name, nc, l, k % 3 != 1,
                                      aux_fields(t, k % 2 == 0, k % 7 == 3)));
                ++k;
            }
    check_stream(recs);
    check_stream({});
    // every odd start of the pools: records of growing length, one at a time and together
    for (int l = 0; l < 40; ++l) check_stream({record(0, l, 3, 2, l, true, {}), record(0, l, 3, 2, 33, false, {})});

    // every truncation of an aux area is refused, and never read past
    const std::vector<uint8_t> aux = aux_fields('i', true, true);
    int refused = 0, taken = 0;
    for (size_t cut = 0; cut <= aux.size(); ++cut) {
        const std::vector<uint8_t> r = record(0, 5, 4, 2, 9, true, std::vector<uint8_t>(aux.begin(), aux.begin() + cut));
        uint8_t *rec = (uint8_t *)malloc(r.size());
        memcpy(rec, r.data(), r.size());
        pr_bam_alns A;
        int64_t *text_at = nullptr;
        const int rc = bam_core_decode(rec, (int64_t)r.size(), 16, &A, &text_at);
        EXPECT(rc == 0 || rc == PR_ERR_SAM);
        if (rc == 0) ++taken, bam_core_free(&A, text_at);
        else ++refused;
        free(rec);
    }
    EXPECT(taken == 22 && refused == (int)aux.size() + 1 - 22);   // taken: the empty area and the 21 field ends
    // bad type letters and array subtypes, a negative array count, an unterminated string
    const char *bad[] = {"XXq\1", "XXBq\1\0\0\0\1", "XXBc\377\377\377\377", "XXZabc"};
    const size_t bad_len[] = {4, 9, 8, 6};
    for (int b = 0; b < 4; ++b) {
        const std::vector<uint8_t> r = record(0, 5, 2, 1, 4, true, std::vector<uint8_t>(bad[b], bad[b] + bad_len[b]));
        pr_bam_alns A;
        int64_t *text_at = nullptr;
        EXPECT(bam_core_decode(r.data(), (int64_t)r.size(), 16, &A, &text_at) == PR_ERR_SAM);
    }
    // the three size errors
    {
        const std::vector<uint8_t> r = record(0, 5, 2, 1, 4, true, {});
        pr_bam_alns A;
        int64_t *text_at = nullptr;
        EXPECT(bam_core_decode(r.data(), 3, 1, &A, &text_at) == PR_ERR_ARG && g_error == "truncated BAM record");
        EXPECT(bam_core_decode(r.data(), (int64_t)r.size() - 1, 1, &A, &text_at) == PR_ERR_ARG && g_error == "bad BAM record size");
        std::vector<uint8_t> s = r;
        s[20] = 200;   // l_seq beyond the record
        EXPECT(bam_core_decode(s.data(), (int64_t)s.size(), 1, &A, &text_at) == PR_ERR_ARG &&
               g_error == "BAM record fields exceed its size");
    }
    if (fails) {
        fprintf(stderr, "bam_core_host: %d checks failed\n", fails);
        return 1;
    }
    printf("bam_core_host: %d records, %d truncations refused, all equal\n", k, refused);
    return 0;
}

// The SEQ-restoring part of proovread_amd/csrc/bam_core.h compiled for the host
// (tests/test_bam_restore_host.py): the key hash and compare, the donor table, the CIGAR walk and
// bam_unpack_seq_from / bam_unpack_qual_from, driven record by record and "lane" by "lane" the way
// the device kernels drive them.
//
// As a shared library: bam_restore_decode fills a pr_bam_alns from a record stream with
// PR_BAM_RESTORE_SEQ's rule applied to every record.  The stream and every donor record are
// read from heap copies of exactly their sizes, and the pools lie between guard bytes that are
// checked afterwards, so a read or write past an end is an error here and under a sanitizer.
// As a program (main): donors of many lengths, every leading / trailing hard-clip split of three
// CIGAR shapes, both orientations, QUAL present and absent, IUPAC and `=` codes, against a plain
// letter-by-letter statement of the rule; exit status 0 when all agree.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../proovread_amd/csrc/bam_core.h"

using namespace prgpu::bam;

namespace {
const int GUARD = 48;
const uint8_t GUARD_BYTE = 0xA5;
std::string g_error;

uint8_t *heap_copy(const uint8_t *p, size_t n) {
    uint8_t *h = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(h, p, n);
    return h;
}

struct Guarded {
    uint8_t *base = nullptr;
    size_t n = 0;
    explicit Guarded(size_t bytes) : n(bytes) {
        base = (uint8_t *)malloc(n + 2 * GUARD);
        memset(base, GUARD_BYTE, n + 2 * GUARD);
    }
    ~Guarded() { free(base); }
    uint8_t *data() { return base + GUARD; }
    bool intact() const {
        for (int k = 0; k < GUARD; ++k)
            if (base[k] != GUARD_BYTE || base[GUARD + n + k] != GUARD_BYTE) return false;
        return true;
    }
};
}   // namespace

extern "C" {

const char *bam_restore_last_error() { return g_error.c_str(); }

void bam_restore_free(pr_bam_alns *a, int64_t *donor_of) {
    void *p[] = {a->rid, a->pos1, a->score, a->flags, a->seq_off, a->lseq, a->cig_off, a->ncig, a->seq, a->qual, a->cig, donor_of};
    for (void *x : p) free(x);
    memset(a, 0, sizeof *a);
}

// 0, PR_ERR_NOSEQ or PR_ERR_SAM (*bad: the lowest offending record), PR_ERR_ARG for a stream the
// size checks refuse.  donor_of_out[i]: the record whose SEQ record i took, or -1.
int bam_restore_decode(const uint8_t *recs_in, int64_t len, int nlanes, pr_bam_alns *out, int64_t *n_restored, int64_t *bad,
                       int64_t **donor_of_out) {
    memset(out, 0, sizeof *out);
    *n_restored = 0;
    *bad = -1;
    *donor_of_out = nullptr;
    uint8_t *recs = heap_copy(recs_in, (size_t)len);   // exactly the stream
    std::vector<int64_t> off;
    for (int64_t o = 0; o < len;) {
        int64_t next = 0;
        const int e = bam_check_record(recs, len, o, &next);
        if (e) {
            g_error = bam_error_text(e);
            free(recs);
            return PR_ERR_ARG;
        }
        off.push_back(o);
        o = next;
    }
    const size_t n = off.size();
    // the donor table
    int64_t eligible = 0;
    for (size_t i = 0; i < n; ++i) eligible += bam_is_donor(recs + off[i], bam_fixed(recs + off[i]));
    const int64_t slots = bam_table_slots(eligible);
    std::vector<unsigned long long> tab((size_t)slots, BAM_SLOT_EMPTY);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t *r = recs + off[i];
        const Fixed f = bam_fixed(r);
        if (bam_is_donor(r, f)) bam_table_insert(tab.data(), slots - 1, recs, off.data(), (int64_t)i, r, f);
    }
    // the lookup
    std::vector<int64_t> src(n), so(n + 1, 0), co(n + 1, 0);
    std::vector<int32_t> hl(n, 0), lseq(n, 0);
    std::vector<uint8_t> rc(n, 0), flags(n, 0);
    std::vector<double> score(n, 0.0);
    int64_t bad_noseq = -1, bad_len = -1;
    int err = 0;
    for (size_t i = 0; i < n && !err; ++i) {
        const uint8_t *r = recs + off[i];
        const Fixed f = bam_fixed(r);
        uint32_t fl = 0;
        int32_t text = 0;
        if (bam_aux_walk(bam_aux_at(r, f), bam_end_of(r, f), &score[i], &fl, &text) != BAM_OK || (fl & BAM_AS_TEXT)) {
            g_error = "aux fields this driver does not take";
            err = PR_ERR_ARG;
            break;
        }
        fl |= bam_seq_flags(r, f);
        src[i] = (int64_t)i;
        lseq[i] = f.l_seq;
        if (fl & PR_ALN_NO_SEQ) {
            const int64_t dn = bam_table_find(tab.data(), slots - 1, recs, off.data(), r, f);
            if (dn < 0) {
                if (bad_noseq < 0) bad_noseq = (int64_t)i;
            } else {
                const uint8_t *d = recs + off[(size_t)dn];
                const Fixed df = bam_fixed(d);
                const CigarSpan sp = bam_cigar_span(r, f);
                if (sp.hl + sp.q + sp.ht != (int64_t)df.l_seq) {
                    if (bad_len < 0) bad_len = (int64_t)i;
                } else {
                    src[i] = dn;
                    hl[i] = (int32_t)sp.hl;
                    rc[i] = ((bam_flag(r) ^ bam_flag(d)) & BAM_REVERSE) ? 1 : 0;
                    lseq[i] = (int32_t)sp.q;
                    fl = (fl & ~(uint32_t)PR_ALN_NO_SEQ) | bam_seq_flags(d, df);
                    ++*n_restored;
                }
            }
        }
        flags[i] = (uint8_t)fl;
        so[i + 1] = so[i] + lseq[i];
        co[i + 1] = co[i] + f.n_cigar;
    }
    if (!err && bad_noseq >= 0 && (bad_len < 0 || bad_noseq < bad_len)) {
        err = PR_ERR_NOSEQ;
        *bad = bad_noseq;
    } else if (!err && bad_len >= 0) {
        err = PR_ERR_SAM;
        *bad = bad_len;
    }
    if (err) {
        free(recs);
        return err;
    }
    // the unpack, every source record from a heap copy of exactly its size
    Guarded seq((size_t)so[n]), qual((size_t)so[n]);
    std::vector<uint32_t> cig((size_t)co[n] + 1);
    int64_t *donor_of = (int64_t *)malloc(8 * (n ? n : 1));
    for (size_t i = 0; i < n; ++i) {
        const size_t j = (size_t)src[i];
        donor_of[i] = j == i ? -1 : (int64_t)j;
        const int64_t size = (j + 1 < n ? off[j + 1] : len) - off[j];
        uint8_t *s = heap_copy(recs + off[j], (size_t)size);
        const Fixed sf = bam_fixed(s);
        const uint8_t *r = recs + off[i];
        const Fixed f = bam_fixed(r);
        for (int lane = 0; lane < nlanes; ++lane) {
            if (j == i) {
                bam_unpack_seq(bam_seq_at(s, sf), sf.l_seq, seq.data() + so[i], lane, nlanes);
                bam_unpack_qual(bam_qual_at(s, sf), sf.l_seq, (flags[i] & PR_ALN_NO_QUAL) != 0, qual.data() + so[i], lane, nlanes);
            } else {
                bam_unpack_seq_from(bam_seq_at(s, sf), sf.l_seq, hl[i], lseq[i], rc[i] != 0, seq.data() + so[i], lane, nlanes);
                bam_unpack_qual_from(bam_qual_at(s, sf), sf.l_seq, hl[i], lseq[i], rc[i] != 0, bam_qual_at(s, sf)[0] == 0xFF,
                                     qual.data() + so[i], lane, nlanes);
            }
            (void)bam_copy_cigar(bam_cigar_at(r, f), f.n_cigar, cig.data() + co[i], lane, nlanes);
        }
        free(s);
    }
    if (!seq.intact() || !qual.intact()) {
        g_error = "a pool's guard bytes were written";
        free(donor_of);
        free(recs);
        return PR_ERR_ARG;
    }
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
    out->seq = (uint8_t *)alloc((size_t)so[n]);
    out->qual = (uint8_t *)alloc((size_t)so[n]);
    out->cig = (uint32_t *)alloc(4 * (size_t)co[n]);
    out->seq_len = so[n];
    out->cig_len = co[n];
    for (size_t i = 0; i < n; ++i) {
        const Fixed f = bam_fixed(recs + off[i]);
        out->rid[i] = f.rid;
        out->pos1[i] = f.pos + 1;
        out->score[i] = score[i];
        out->flags[i] = flags[i];
        out->seq_off[i] = so[i];
        out->lseq[i] = lseq[i];
        out->cig_off[i] = co[i];
        out->ncig[i] = f.n_cigar;
    }
    if (so[n]) memcpy(out->seq, seq.data(), (size_t)so[n]), memcpy(out->qual, qual.data(), (size_t)so[n]);
    if (co[n]) memcpy(out->cig, cig.data(), 4 * (size_t)co[n]);
    *donor_of_out = donor_of;
    free(recs);
    return 0;
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

uint32_t g_rng = 2024;
uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

const char NT16[] = "=ACMGRSVTWYHKDBN";

// a record; seq: letters of NT16 ("" = no SEQ), qual: raw phred bytes ("" with a SEQ: absent, 0xFF)
std::vector<uint8_t> record(const std::string &name, uint32_t flag, int32_t rid, int32_t pos,
                            const std::vector<uint32_t> &cigar, const std::string &seq, const std::string &qual) {
    std::vector<uint8_t> b;
    put32(b, (uint32_t)rid);
    put32(b, (uint32_t)pos);
    b.push_back((uint8_t)(name.size() + 1));
    b.push_back(60);
    put16(b, 4680);
    put16(b, (uint32_t)cigar.size());
    put16(b, flag);
    put32(b, (uint32_t)seq.size());
    put32(b, 0xffffffffu);
    put32(b, 0xffffffffu);
    put32(b, 0);
    b.insert(b.end(), name.begin(), name.end());
    b.push_back(0);
    for (uint32_t op : cigar) put32(b, op);
    for (size_t k = 0; k < seq.size(); k += 2) {
        const uint32_t hi = (uint32_t)(strchr(NT16, seq[k]) - NT16);
        const uint32_t lo = k + 1 < seq.size() ? (uint32_t)(strchr(NT16, seq[k + 1]) - NT16) : 0u;
        b.push_back((uint8_t)(hi << 4 | lo));
    }
    for (size_t k = 0; k < seq.size(); ++k) b.push_back(qual.empty() ? (uint8_t)0xFF : (uint8_t)qual[k]);
    std::vector<uint8_t> r;
    put32(r, (uint32_t)b.size());
    r.insert(r.end(), b.begin(), b.end());
    return r;
}

uint32_t op(uint32_t len, char c) { return len << 4 | (uint32_t)(strchr("MIDNSHP=X", c) - "MIDNSHP=X"); }

// the rule, letter by letter
std::string plain_seq(const std::string &donor, int hl, int q, bool rev) {
    std::string o = donor;
    if (rev) {
        std::reverse(o.begin(), o.end());
        for (char &c : o) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c;
    }
    return o.substr((size_t)hl, (size_t)q);
}
std::string plain_qual(const std::string &donor_qual, size_t dl, int hl, int q, bool rev) {
    if (donor_qual.empty()) return std::string((size_t)q, '!');
    std::string o = donor_qual;
    (void)dl;
    if (rev) std::reverse(o.begin(), o.end());
    o = o.substr((size_t)hl, (size_t)q);
    for (char &c : o) c = (char)(uint8_t)((uint8_t)c + 33);
    return o;
}

int fails = 0;
long checked = 0;
#define EXPECT(c)                                              \
    do {                                                       \
        if (!(c)) {                                            \
            ++fails;                                           \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                      \
    } while (0)

// the body of a record of q bases between hl and ht hard-clipped ones, in one of three shapes
std::vector<uint32_t> shape(int kind, int hl, int q, int ht) {
    std::vector<uint32_t> c;
    if (hl) c.push_back(op((uint32_t)hl, 'H'));
    if (kind == 0 || q < 4) {
        c.push_back(op((uint32_t)q, 'M'));
    } else if (kind == 1) {                        // soft clip, match, insertion, deletion, match
        c.push_back(op(1, 'S'));
        c.push_back(op((uint32_t)q - 3, 'M'));
        c.push_back(op(1, 'I'));
        c.push_back(op(2, 'D'));
        c.push_back(op(1, 'M'));
    } else {                                       // =, X, a skip, padding
        c.push_back(op((uint32_t)q - 2, '='));
        c.push_back(op(3, 'N'));
        c.push_back(op(1, 'X'));
        c.push_back(op(1, 'P'));
        c.push_back(op(1, 'M'));
    }
    if (ht) c.push_back(op((uint32_t)ht, 'H'));
    return c;
}

// one donor and one record that takes its SEQ: decoded through the driver above, by 1 and 16 lanes
void check_pair(int dl, int hl, int ht, int kind, bool rev, bool has_qual, int pad) {
    std::string seq((size_t)dl, 'A'), qual;
    for (char &c : seq) c = NT16[rnd() % 16];
    if (has_qual) {
        qual.assign((size_t)dl, 0);
        for (char &c : qual) c = (char)(rnd() % 94);
        if ((uint8_t)qual[0] == 0xFF) qual[0] = 0;
    }
    const int q = dl - hl - ht;
    std::vector<std::vector<uint8_t>> recs;
    // a first record of `pad` bases moves the pools' offsets over a 16-byte line
    if (pad) recs.push_back(record("pad", 0, 0, 1, {op((uint32_t)pad, 'M')}, std::string((size_t)pad, 'C'), std::string((size_t)pad, 5)));
    recs.push_back(record("read", 0x100 | (rev ? 0x10 : 0), 0, 5, shape(kind, hl, q, ht), "", ""));
    recs.push_back(record("read", 0, 1, 9, {op((uint32_t)dl, 'M')}, seq, qual));
    std::vector<uint8_t> all;
    for (auto &r : recs) all.insert(all.end(), r.begin(), r.end());
    const size_t at = pad ? 1 : 0;
    for (int nlanes : {1, 16}) {
        pr_bam_alns A;
        int64_t nr = 0, bad = 0, *donor_of = nullptr;
        const int rc = bam_restore_decode(all.data(), (int64_t)all.size(), nlanes, &A, &nr, &bad, &donor_of);
        EXPECT(rc == 0);
        if (rc) continue;
        EXPECT(nr == 1 && donor_of[at] == (int64_t)at + 1 && donor_of[at + 1] == -1);
        EXPECT(A.lseq[at] == q && A.seq_off[at] == pad);
        EXPECT(A.flags[at] == (has_qual ? 0 : PR_ALN_NO_QUAL));
        const std::string es = plain_seq(seq, hl, q, rev), eq = plain_qual(qual, (size_t)dl, hl, q, rev);
        EXPECT(memcmp(A.seq + A.seq_off[at], es.data(), (size_t)q) == 0);
        EXPECT(memcmp(A.qual + A.seq_off[at], eq.data(), (size_t)q) == 0);
        EXPECT(memcmp(A.seq + A.seq_off[at + 1], seq.data(), (size_t)dl) == 0);   // the donor itself
        ++checked;
        bam_restore_free(&A, donor_of);
    }
}

int refusal(const std::vector<std::vector<uint8_t>> &recs, int64_t *bad) {
    std::vector<uint8_t> all;
    for (auto &r : recs) all.insert(all.end(), r.begin(), r.end());
    pr_bam_alns A;
    int64_t nr = 0, *donor_of = nullptr;
    const int rc = bam_restore_decode(all.data(), (int64_t)all.size(), 16, &A, &nr, bad, &donor_of);
    if (rc == 0) bam_restore_free(&A, donor_of);
    return rc;
}

}   // namespace

int main() {
    // every split of the donor's bases into leading clip, slice and trailing clip
    int k = 0;
    for (int dl = 1; dl <= 70; ++dl)
        for (int hl = 0; hl < dl; ++hl)
            for (int ht = 0; hl + ht < dl; ++ht, ++k)
                check_pair(dl, hl, ht, k % 3, (k / 3) % 2 != 0, (k / 6) % 2 != 0, k % 16);
    // long donors: clips around the 16-byte lines and the nibble phase, every combination
    for (int dl : {255, 256, 1000})
        for (int hl : {0, 1, 2, 15, 16, 17, 100, 101})
            for (int ht : {0, 1, 8, 33})
                for (int kind = 0; kind < 3; ++kind)
                    for (int rev = 0; rev < 2; ++rev)
                        for (int hq = 0; hq < 2; ++hq) check_pair(dl, hl, ht, kind, rev != 0, hq != 0, (hl + ht + kind) % 16);

    // keys: the mate bits and the whole name tell donors apart; the lower index wins
    {
        const std::vector<uint32_t> m4 = {op(4, 'M')};
        std::vector<std::vector<uint8_t>> recs = {
            record("pair", 0x141, 0, 1, m4, "", ""), record("pair", 0x181, 0, 2, m4, "", ""),
            record("pair", 0x81, 0, 3, m4, "GGGG", "abcd"), record("pair", 0x41, 0, 4, m4, "ACGT", "abcd"),
            record("pair", 0x41, 0, 5, m4, "TTTT", "abcd"), record("pairs", 0, 0, 6, m4, "CCCC", "abcd"),
            record("pai", 0x100, 0, 7, m4, "", ""), record("pai", 0, 1, 8, m4, "AAAA", ""),
        };
        std::vector<uint8_t> all;
        for (auto &r : recs) all.insert(all.end(), r.begin(), r.end());
        pr_bam_alns A;
        int64_t nr = 0, bad = 0, *donor_of = nullptr;
        EXPECT(bam_restore_decode(all.data(), (int64_t)all.size(), 16, &A, &nr, &bad, &donor_of) == 0);
        EXPECT(nr == 3 && donor_of[0] == 3 && donor_of[1] == 2 && donor_of[6] == 7);
        EXPECT(memcmp(A.seq, "ACGTGGGG", 8) == 0 && A.flags[6] == PR_ALN_NO_QUAL);
        bam_restore_free(&A, donor_of);
    }
    // refusals: no donor at all, only a secondary / supplementary / unmapped / hard-clipped one, another
    // mate; a length mismatch; the lower record index speaks
    {
        const std::vector<uint32_t> m4 = {op(4, 'M')}, m5 = {op(5, 'M')}, h = {op(1, 'H'), op(4, 'M')};
        int64_t bad = -1;
        EXPECT(refusal({record("a", 0x100, 0, 1, m4, "", "")}, &bad) == PR_ERR_NOSEQ && bad == 0);
        for (uint32_t fl : {0x100u, 0x800u, 0x4u})
            EXPECT(refusal({record("a", fl, 0, 1, m4, "ACGT", ""), record("a", 0x100, 0, 2, m4, "", "")}, &bad) == PR_ERR_NOSEQ && bad == 1);
        EXPECT(refusal({record("a", 0, 0, 1, h, "ACGT", ""), record("a", 0x100, 0, 2, m4, "", "")}, &bad) == PR_ERR_NOSEQ && bad == 1);
        EXPECT(refusal({record("a", 0x41, 0, 1, m4, "ACGT", ""), record("a", 0x181, 0, 2, m4, "", "")}, &bad) == PR_ERR_NOSEQ && bad == 1);
        EXPECT(refusal({record("a", 0, 0, 1, m4, "ACGT", ""), record("a", 0x100, 0, 2, m5, "", "")}, &bad) == PR_ERR_SAM && bad == 1);
        EXPECT(refusal({record("a", 0, 0, 1, m4, "ACGT", ""), record("a", 0x100, 0, 2, h, "", "")}, &bad) == PR_ERR_SAM && bad == 1);
        EXPECT(refusal({record("a", 0, 0, 1, m4, "ACGT", ""), record("a", 0x100, 0, 2, m5, "", ""), record("b", 0x100, 0, 3, m4, "", "")},
                       &bad) == PR_ERR_SAM && bad == 1);
        EXPECT(refusal({record("a", 0, 0, 1, m4, "ACGT", ""), record("b", 0x100, 0, 2, m4, "", ""), record("a", 0x100, 0, 3, m5, "", "")},
                       &bad) == PR_ERR_NOSEQ && bad == 1);
    }
    // a table under load: names one letter apart, each donor found behind its collisions
    {
        std::vector<std::vector<uint8_t>> recs;
        const int n = 500;
        for (int i = 0; i < n; ++i) {
            char name[16];
            snprintf(name, sizeof name, "q%04d", i);
            std::string s(6, 'A');
            for (int j = 0; j < 6; ++j) s[(size_t)j] = "ACGT"[(i >> (2 * j)) & 3];
            recs.push_back(record(name, 0x100, 0, i, {op(6, 'M')}, "", ""));
            recs.push_back(record(name, 0, 1, i, {op(6, 'M')}, s, ""));
        }
        std::vector<uint8_t> all;
        for (auto &r : recs) all.insert(all.end(), r.begin(), r.end());
        pr_bam_alns A;
        int64_t nr = 0, bad = 0, *donor_of = nullptr;
        EXPECT(bam_restore_decode(all.data(), (int64_t)all.size(), 16, &A, &nr, &bad, &donor_of) == 0);
        EXPECT(nr == n);
        for (int i = 0; i < n; ++i) EXPECT(donor_of[2 * i] == 2 * i + 1);
        bam_restore_free(&A, donor_of);
    }
    if (fails) {
        fprintf(stderr, "bam_restore_host: %d checks failed\n", fails);
        return 1;
    }
    printf("bam_restore_host: %ld slices, all equal\n", checked);
    return 0;
}

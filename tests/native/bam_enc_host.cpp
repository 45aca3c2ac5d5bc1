// proovread_amd/csrc/bam_enc_core.h compiled for the host (tests/test_bam_enc_host.py): the record
// encoder the device kernels run, driven record by record and "lane" by "lane", against
// pr_sam_encode (proovread_amd/csrc/bam_codec.cpp, compiled in) of the equivalent SAM line.
//
// As a shared library: bam_enc_record encodes one record (the Python test compares it with the
// library's own pr_sam_encode), bam_enc_grid runs the whole grid of cases below.
// As a program (main): the same grid for 1 and 16 lanes; exit status 0 when every byte agrees.
//
// Every record is written into a scratch buffer with guard bytes on both sides, at the offset in
// a 16-byte line it has in the stream; its inputs (name, CIGAR, bases, qualities) are heap copies
// of exactly their sizes, so a read or write past either end is an error a sanitizer sees.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../proovread_amd/csrc/bam_enc_core.h"

using namespace prgpu::bam;

// the library's error text (prgpu_api.cpp), for bam_codec.cpp
static std::string g_error;
int set_error(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}
int pr_set_error(int code, const char *msg) { return set_error(code, "%s", msg); }

namespace {

enum { GUARD = 64, GUARD_BYTE = 0xA5 };

template <class T>
T *exact_copy(const T *src, size_t n) {
    T *p = (T *)malloc(n ? n * sizeof(T) : 1);
    if (n) memcpy(p, src, n * sizeof(T));
    return p;
}

// one record by nl emulated lanes at line offset `align`; -1: a guard byte was touched
int64_t encode_one(int32_t rid, int32_t pos, int32_t flag, int32_t score, const char *name, int32_t l_name,
                   const uint32_t *cig, int32_t n_cigar, const uint8_t *seq, const uint8_t *qual, int32_t l_seq, int rev,
                   int nl, int align, std::vector<uint8_t> &out) {
    EncRec R;
    R.rid = rid; R.pos = pos; R.flag = flag; R.score = score; R.l_name = l_name; R.n_cigar = n_cigar; R.l_seq = l_seq;
    R.rev = rev;
    uint8_t *nm = exact_copy((const uint8_t *)name, (size_t)l_name);
    uint32_t *cg = exact_copy(cig, (size_t)n_cigar);
    uint8_t *sq = exact_copy(seq, (size_t)l_seq);
    uint8_t *ql = qual ? exact_copy(qual, (size_t)l_seq) : nullptr;
    R.name = nm; R.cig = cg; R.seq = sq; R.qual = ql;
    const int64_t size = enc_size(l_name, n_cigar, l_seq, score);
    const size_t total = (size_t)(2 * GUARD + 16 + size);
    uint8_t *buf = (uint8_t *)aligned_alloc(16, (total + 15) & ~(size_t)15);
    memset(buf, GUARD_BYTE, total);
    uint8_t *dst = buf + GUARD + (align & 15);
    int64_t span = 0;
    for (int lane = 0; lane < nl; ++lane) span += enc_span_part(R.cig, n_cigar, lane, nl);
    for (int lane = nl - 1; lane >= 0; --lane) enc_write(R, span, dst, lane, nl);   // (any lane order)
    bool touched = false;
    for (uint8_t *p = buf; p < dst; ++p) touched |= *p != GUARD_BYTE;
    for (uint8_t *p = dst + size; p < buf + total; ++p) touched |= *p != GUARD_BYTE;
    out.insert(out.end(), dst, dst + size);
    free(buf); free(nm); free(cg); free(sq); free(ql);
    return touched ? -1 : size;
}

// ------------------------------------------------------------------------------- the grid
const int LSEQS[] = {1, 2, 15, 16, 17, 25, 26, 150, 151, 1000};
const int NAMES[] = {1, 2, 3, 4, 5, 254};
const int SCORES[] = {-129, -128, 0, 127, 128, 255, 256, 32767, 32768, 65535, 65536};
// CIGAR shapes: n_cigar 1, 2 (soft clip), 2 (reference span 0), 7 (clips at both ends, every op
// that counts for the span and both that do not)
enum { CIG_1, CIG_2_CLIP, CIG_2_SPAN0, CIG_7, CIG_KINDS };
// POS: windows ending at 16383, 16384, 16385, and windows straddling 1 << 17, 20, 23, 26 (one
// case per reg2bin level, the last returning bin 0)
enum { POS_E16383, POS_E16384, POS_E16385, POS_S17, POS_S20, POS_S23, POS_S26, POS_KINDS };

uint32_t g_rng;
uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }

std::vector<uint32_t> cigar_of(int kind, int l) {
    auto op = [](uint32_t len, int o) { return (len << 4) | (uint32_t)o; };
    switch (kind) {
        case CIG_1: return {op((uint32_t)l, 0)};
        case CIG_2_CLIP: return l > 1 ? std::vector<uint32_t>{op((uint32_t)(l / 3 + 1 > l - 1 ? l - 1 : l / 3 + 1), 4),
                                                               op((uint32_t)(l - (l / 3 + 1 > l - 1 ? l - 1 : l / 3 + 1)), 0)}
                                      : std::vector<uint32_t>{op(1, 0), op(3, 2)};
        case CIG_2_SPAN0: return {op(1, 4), op((uint32_t)l, 1)};
        default: return {op(2, 4), op(3, 0), op(1, 1), op(4, 7), op(2, 2), op(5, 3), op((uint32_t)l, 8)};
    }
}

int64_t span_of(const std::vector<uint32_t> &c) {
    int64_t s = 0;
    for (uint32_t x : c) {
        const uint32_t o = x & 15u;
        if (o == 0 || o == 2 || o == 3 || o == 7 || o == 8) s += x >> 4;
    }
    return s;
}

int32_t pos_of(int kind, int64_t span) {
    const int64_t w = span ? span : 1;
    switch (kind) {
        case POS_E16383: return (int32_t)(16383 - w);
        case POS_E16384: return (int32_t)(16384 - w);
        case POS_E16385: return (int32_t)(16385 - w);
        case POS_S17: return (int32_t)((1 << 17) - (w + 1) / 2);
        case POS_S20: return (int32_t)((1 << 20) - (w + 1) / 2);
        case POS_S23: return (int32_t)((1 << 23) - (w + 1) / 2);
        default: return (int32_t)((1 << 26) - (w + 1) / 2);
    }
}

struct GridResult {
    int64_t cases = 0, mismatches = 0, guards = 0;
    std::string first;
};

GridResult run_grid(int nl) {
    static const char OPS[] = "MIDNSHP=X";
    GridResult G;
    g_rng = 20240607u;
    std::string sam;
    std::vector<uint8_t> got;
    std::vector<std::string> what;
    char num[64];
    int64_t k = 0;
    for (int l : LSEQS) {
        std::vector<uint8_t> seq((size_t)l), qual((size_t)l);
        for (int i = 0; i < l; ++i) seq[(size_t)i] = (uint8_t)(rnd() >> 8) % 5, qual[(size_t)i] = (uint8_t)(33 + (rnd() >> 8) % 42);
        std::string fw, rc, qf, qr;
        for (int i = 0; i < l; ++i) fw.push_back("ACGTN"[seq[(size_t)i]]), qf.push_back((char)qual[(size_t)i]);
        for (int i = l - 1; i >= 0; --i) rc.push_back("TGCAN"[seq[(size_t)i]]), qr.push_back((char)qual[(size_t)i]);
        for (int ln : NAMES) {
            std::string name;
            for (int i = 0; i < ln; ++i) name.push_back((char)('a' + (rnd() >> 8) % 26));
            for (int ck = 0; ck < CIG_KINDS; ++ck) {
                const std::vector<uint32_t> cig = cigar_of(ck, l);
                std::string cs;
                for (uint32_t x : cig) snprintf(num, sizeof num, "%u%c", x >> 4, OPS[x & 15u]), cs += num;
                const int64_t span = span_of(cig);
                for (int rev = 0; rev < 2; ++rev)
                    for (int hq = 0; hq < 2; ++hq)
                        for (int sc : SCORES)
                            for (int pk = 0; pk < POS_KINDS; ++pk, ++k) {
                                const int32_t pos = pos_of(pk, span), rid = (int32_t)(k % 3);
                                const int32_t flag = (rev ? 16 : 0) | (k % 5 == 0 ? 0x100 : 0);
                                const int64_t at = (int64_t)got.size();
                                const int64_t sz = encode_one(rid, pos, flag, sc, name.data(), ln, cig.data(), (int32_t)cig.size(),
                                                              seq.data(), hq ? qual.data() : nullptr, l, rev, nl, (int)(at & 15), got);
                                if (sz < 0) ++G.guards;
                                snprintf(num, sizeof num, "\t%d\tlr%d\t%d\t%d\t", flag, rid, pos + 1, (flag & 0x100) ? 0 : 60);
                                sam += name;
                                sam += num;
                                sam += cs;
                                sam += "\t*\t0\t0\t";
                                sam += rev ? rc : fw;
                                sam += '\t';
                                sam += hq ? (rev ? qr : qf) : std::string("*");
                                snprintf(num, sizeof num, "\tAS:i:%d\n", sc);
                                sam += num;
                                snprintf(num, sizeof num, "l_seq %d name %d cigar %s rev %d qual %d AS %d pos %d", l, ln, cs.c_str(),
                                         rev, hq, sc, pos);
                                what.push_back(num);
                            }
            }
        }
    }
    G.cases = k;
    const char *refs[3] = {"lr0", "lr1", "lr2"};
    uint8_t *want = nullptr;
    int64_t want_len = 0, n_rec = 0;
    if (pr_sam_encode(sam.data(), (int64_t)sam.size(), refs, 3, 4, &want, &want_len, &n_rec) != 0 || n_rec != k) {
        G.mismatches = -1;
        G.first = "pr_sam_encode failed: " + g_error;
        return G;
    }
    // record by record (sizes from the expected stream)
    int64_t o = 0, i = 0;
    for (; o + 4 <= want_len && i < k; ++i) {
        const int64_t sz = 4 + (int64_t)bam_rd32(want + o);
        const bool same = o + sz <= (int64_t)got.size() && memcmp(want + o, got.data() + o, (size_t)sz) == 0;
        if (!same) {
            if (!G.mismatches) G.first = what[(size_t)i];
            ++G.mismatches;
            // (sizes may differ from here on: stop at the first record that does not line up)
            if (o + 4 > (int64_t)got.size() || bam_rd32(got.data() + o) != bam_rd32(want + o)) break;
        }
        o += sz;
    }
    if (!G.mismatches && (int64_t)got.size() != want_len) {
        G.mismatches = 1;
        G.first = "stream lengths differ";
    }
    free(want);
    return G;
}

}   // namespace

extern "C" {

const char *bam_enc_last_error() { return g_error.c_str(); }

// one record into out[cap]; returns its size, -1 when a guard byte was touched, -2 when cap is short
int64_t bam_enc_record(int32_t rid, int32_t pos, int32_t flag, int32_t score, const char *name, int32_t l_name,
                       const uint32_t *cig, int32_t n_cigar, const uint8_t *seq, const uint8_t *qual, int32_t l_seq, int rev,
                       int nl, int align, uint8_t *out, int64_t cap) {
    std::vector<uint8_t> v;
    const int64_t sz = encode_one(rid, pos, flag, score, name, l_name, cig, n_cigar, seq, qual, l_seq, rev, nl, align, v);
    if (sz < 0) return -1;
    if (sz > cap) return -2;
    memcpy(out, v.data(), (size_t)sz);
    return sz;
}

// the grid by nl lanes: returns the mismatching records (0: every byte equal), -1 on an oracle error
int64_t bam_enc_grid(int nl, int64_t *cases, int64_t *guards) {
    const GridResult G = run_grid(nl);
    *cases = G.cases;
    *guards = G.guards;
    if (G.mismatches) g_error = G.first;
    return G.mismatches;
}
}

#ifdef BAM_ENC_MAIN
int main() {
    for (int nl : {1, 16}) {
        const GridResult G = run_grid(nl);
        printf("lanes %d: %lld cases, %lld mismatches, %lld guard hits%s%s\n", nl, (long long)G.cases, (long long)G.mismatches,
               (long long)G.guards, G.first.empty() ? "" : ", first: ", G.first.c_str());
        if (G.mismatches || G.guards || !G.cases) return 1;
    }
    printf("all equal\n");
    return 0;
}
#endif

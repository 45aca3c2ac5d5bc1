// BAM record decoding shared by the device decoder (bam_kernels.hip), its host entry
// (bam_api.cpp) and host builds (tests/native/bam_core_host.cpp): what pr_bam_decode_alns
// (bam_codec.cpp) reads of a record -- the fixed fields, the aux walk for the last AS tag, SEQ as
// SAM prints it, QUAL as phred+33, the CIGAR ops.
//
// A record starts at its block_size word; every field behind the read name sits at an arbitrary
// byte offset, so multi-byte fields are read bytewise (never a misaligned word load).  Outputs go
// to the pools in 16-byte chunks cut at 16-byte-aligned destination addresses: a full chunk is
// one aligned 16-byte store, the partial chunks at the two ends of a record are byte stores.  The
// unpack functions take (lane, nlanes): lane l handles chunks l, l + nlanes, ..; the kernels
// call them with a 16-lane group per record, the host with nlanes = 1 or lane by lane.
//
// The second half of the file is PR_BAM_RESTORE_SEQ's: the key of a record, the donor table, the
// CIGAR walk and the unpack of a slice of another record's SEQ / QUAL in either orientation
// (host build: tests/native/bam_restore_host.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/prgpu.h"

#if defined(__HIPCC__)
#define BAM_HD __host__ __device__ inline
#else
#define BAM_HD inline
#endif

namespace prgpu {
namespace bam {

// private flag beside the PR_ALN_* bits: the last AS tag is a string (AS:Z / AS:H); its score is
// Perl's numification of the text, which the host computes (bam_codec.cpp perl_number)
enum { BAM_AS_TEXT = 0x80 };
// scan / walk results
enum { BAM_OK = 0, BAM_TRUNCATED = 1, BAM_BAD_SIZE = 2, BAM_FIELDS_EXCEED = 3, BAM_BAD_AUX = 4 };

struct Fixed {
    int32_t block_size, rid, pos, l_read_name, n_cigar, l_seq;
};

struct alignas(16) Chunk {
    uint32_t w[4];
};

BAM_HD uint32_t bam_rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
BAM_HD uint32_t bam_rd32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// the fixed fields of the record at rec (its block_size word first)
BAM_HD Fixed bam_fixed(const uint8_t *rec) {
    Fixed f;
    f.block_size = (int32_t)bam_rd32(rec);
    f.rid = (int32_t)bam_rd32(rec + 4);
    f.pos = (int32_t)bam_rd32(rec + 8);
    f.l_read_name = rec[12];
    f.n_cigar = (int32_t)bam_rd16(rec + 16);
    f.l_seq = (int32_t)bam_rd32(rec + 20);
    return f;
}

// bam_codec.cpp:491-500 for the record at offset o of a stream of len bytes: BAM_OK and *next
BAM_HD int bam_check_record(const uint8_t *recs, int64_t len, int64_t o, int64_t *next) {
    if (len - o < 4) return BAM_TRUNCATED;
    const int32_t bs = (int32_t)bam_rd32(recs + o);
    if (bs < 32 || o + 4 + (int64_t)bs > len) return BAM_BAD_SIZE;
    const Fixed f = bam_fixed(recs + o);
    const int64_t need = 32 + (int64_t)f.l_read_name + 4 * (int64_t)f.n_cigar + ((int64_t)f.l_seq + 1) / 2 + f.l_seq;
    if (f.l_seq < 0 || need > bs) return BAM_FIELDS_EXCEED;
    *next = o + 4 + (int64_t)bs;
    return BAM_OK;
}

BAM_HD const char *bam_error_text(int e) {
    return e == BAM_TRUNCATED ? "truncated BAM record"
         : e == BAM_BAD_SIZE ? "bad BAM record size"
         : e == BAM_FIELDS_EXCEED ? "BAM record fields exceed its size"
         : e == BAM_BAD_AUX ? "bad BAM aux field" : "";
}

// where the parts of a checked record start
BAM_HD const uint8_t *bam_cigar_at(const uint8_t *rec, const Fixed &f) { return rec + 36 + f.l_read_name; }
BAM_HD const uint8_t *bam_seq_at(const uint8_t *rec, const Fixed &f) { return bam_cigar_at(rec, f) + 4 * (int64_t)f.n_cigar; }
BAM_HD const uint8_t *bam_qual_at(const uint8_t *rec, const Fixed &f) { return bam_seq_at(rec, f) + (f.l_seq + 1) / 2; }
BAM_HD const uint8_t *bam_aux_at(const uint8_t *rec, const Fixed &f) { return bam_qual_at(rec, f) + f.l_seq; }
BAM_HD const uint8_t *bam_end_of(const uint8_t *rec, const Fixed &f) { return rec + 4 + (int64_t)f.block_size; }

BAM_HD int bam_int_size(uint8_t t) {
    return (t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I') ? 4 : 0;
}

// The aux fields [a, end): the last AS tag wins.  *score / *flags get the value and
// PR_ALN_HAS_SCORE; a text AS sets BAM_AS_TEXT and *text = the offset of its first character from
// a0 (the value stays 0 until the host fills it).  Every read is checked against end first.
BAM_HD int bam_aux_walk(const uint8_t *a, const uint8_t *end, double *score, uint32_t *flags, int32_t *text) {
    const uint8_t *a0 = a;
    double sc = 0.0;
    uint32_t fl = 0;
    int32_t tx = 0;
    while (a < end) {
        if (end - a < 3) return BAM_BAD_AUX;
        const bool as = a[0] == 'A' && a[1] == 'S';
        const uint8_t t = a[2];
        a += 3;
        const int sz = bam_int_size(t);
        if (sz) {
            if (end - a < sz) return BAM_BAD_AUX;
            if (as) {
                int64_t v;
                switch (t) {
                    case 'c': v = (int8_t)a[0]; break;
                    case 'C': v = a[0]; break;
                    case 's': v = (int16_t)bam_rd16(a); break;
                    case 'S': v = (int64_t)bam_rd16(a); break;
                    case 'i': v = (int32_t)bam_rd32(a); break;
                    default: v = (int64_t)bam_rd32(a); break;
                }
                sc = (double)v;
                fl = PR_ALN_HAS_SCORE;
            }
            a += sz;
        } else if (t == 'A' || t == 'f') {
            const int w = t == 'A' ? 1 : 4;
            if (end - a < w) return BAM_BAD_AUX;
            if (as && t == 'f') {
                const uint32_t u = bam_rd32(a);
                float f;
                memcpy(&f, &u, 4);
                sc = (double)f;
                fl = PR_ALN_HAS_SCORE;
            }
            a += w;
        } else if (t == 'Z' || t == 'H') {
            const uint8_t *z = a;
            while (z < end && *z) ++z;
            if (z >= end) return BAM_BAD_AUX;
            if (as) {
                sc = 0.0;
                fl = PR_ALN_HAS_SCORE | BAM_AS_TEXT;
                tx = (int32_t)(a - a0);
            }
            a = z + 1;
        } else if (t == 'B') {
            if (end - a < 5) return BAM_BAD_AUX;
            const uint8_t st = a[0];
            const int32_t cnt = (int32_t)bam_rd32(a + 1);
            const int es = st == 'f' ? 4 : bam_int_size(st);
            if (!es || cnt < 0 || (int64_t)(end - a) < 5 + (int64_t)cnt * es) return BAM_BAD_AUX;
            a += 5 + (int64_t)cnt * es;
        } else {
            return BAM_BAD_AUX;
        }
    }
    *score = sc;
    *flags = fl;
    *text = tx;
    return BAM_OK;
}

// PR_ALN_NO_SEQ / PR_ALN_NO_QUAL of a checked record
BAM_HD uint32_t bam_seq_flags(const uint8_t *rec, const Fixed &f) {
    if (f.l_seq == 0) return PR_ALN_NO_SEQ;
    return bam_qual_at(rec, f)[0] == 0xFF ? PR_ALN_NO_QUAL : 0;
}

// "=ACMGRSVTWYHKDBN"[x] from two 64-bit words (no table in memory)
BAM_HD uint32_t bam_nt16_char(uint32_t x) {
    const uint64_t lo = 0x565352474d43413dull;   // = A C M G R S V
    const uint64_t hi = 0x4e42444b48595754ull;   // T W Y H K D B N
    return (uint32_t)(((x & 8) ? hi : lo) >> (8 * (x & 7))) & 255u;
}
BAM_HD uint32_t bam_base(const uint8_t *sb, int32_t k) { return bam_nt16_char((sb[k >> 1] >> (4 * (1 - (k & 1)))) & 15u); }

BAM_HD void bam_store_chunk(uint8_t *dst, const Chunk &c) { *reinterpret_cast<Chunk *>(dst) = c; }

// chunks of a destination [dst, dst + n): chunk c holds the bytes k of [16 c - a0, 16 c - a0 + 16)
// inside [0, n), a0 = dst's offset in its 16-byte line
BAM_HD int32_t bam_line_offset(const uint8_t *dst) { return (int32_t)((uintptr_t)dst & 15u); }
BAM_HD int32_t bam_chunks(int32_t a0, int32_t n) { return n > 0 ? (a0 + n + 15) >> 4 : 0; }

// SEQ: l_seq bases from the 4-bit codes at sb, as characters at dst
BAM_HD void bam_unpack_seq(const uint8_t *sb, int32_t l_seq, uint8_t *dst, int lane, int nlanes) {
    const int32_t a0 = bam_line_offset(dst), nc = bam_chunks(a0, l_seq);
    for (int32_t c = lane; c < nc; c += nlanes) {
        const int32_t k0 = 16 * c - a0;
        if (k0 >= 0 && k0 + 16 <= l_seq) {
            // 16 bases from the 8 or 9 bytes that hold them
            const uint8_t *p = sb + (k0 >> 1);
            uint64_t v = 0;   // the nibbles of bases k0 .. k0 + 15, base j at bits 4 j
            if (k0 & 1) {
                uint32_t prev = p[0];
                for (int j = 0; j < 8; ++j) {
                    const uint32_t b = p[j + 1];
                    v |= (uint64_t)((prev & 15u) | (b & 0xf0u)) << (8 * j);   // low nibble of byte j, high of j + 1
                    prev = b;
                }
            } else {
                for (int j = 0; j < 8; ++j) {
                    const uint32_t b = p[j];
                    v |= (uint64_t)(((b >> 4) & 15u) | ((b & 15u) << 4)) << (8 * j);
                }
            }
            Chunk o;
            for (int w = 0; w < 4; ++w) {
                uint32_t x = 0;
                for (int j = 0; j < 4; ++j) x |= bam_nt16_char((uint32_t)(v >> (4 * (4 * w + j))) & 15u) << (8 * j);
                o.w[w] = x;
            }
            bam_store_chunk(dst + k0, o);
        } else {
            const int32_t lo = k0 < 0 ? 0 : k0, hi = k0 + 16 < l_seq ? k0 + 16 : l_seq;
            for (int32_t k = lo; k < hi; ++k) dst[k] = (uint8_t)bam_base(sb, k);
        }
    }
}

// QUAL: phred + 33 (modulo 256, as the host decoder's uint8 sum), or '!' x l_seq when absent
BAM_HD void bam_unpack_qual(const uint8_t *qb, int32_t l_seq, bool no_qual, uint8_t *dst, int lane, int nlanes) {
    const int32_t a0 = bam_line_offset(dst), nc = bam_chunks(a0, l_seq);
    for (int32_t c = lane; c < nc; c += nlanes) {
        const int32_t k0 = 16 * c - a0;
        if (k0 >= 0 && k0 + 16 <= l_seq) {
            Chunk o;
            for (int w = 0; w < 4; ++w) {
                const uint32_t q = no_qual ? 0u : bam_rd32(qb + k0 + 4 * w);
                o.w[w] = ((q & 0x7f7f7f7fu) + 0x21212121u) ^ (q & 0x80808080u);   // bytewise + 33, no carries across bytes
            }
            bam_store_chunk(dst + k0, o);
        } else {
            const int32_t lo = k0 < 0 ? 0 : k0, hi = k0 + 16 < l_seq ? k0 + 16 : l_seq;
            for (int32_t k = lo; k < hi; ++k) dst[k] = no_qual ? (uint8_t)'!' : (uint8_t)(qb[k] + 33);
        }
    }
}

// CIGAR: n ops (len << 4 | op) from the unaligned words at c; returns the lane's sum of the
// insertion lengths (the consensus's output capacity counts them)
BAM_HD int64_t bam_copy_cigar(const uint8_t *c, int32_t n, uint32_t *dst, int lane, int nlanes) {
    int64_t ins = 0;
    for (int32_t j = lane; j < n; j += nlanes) {
        const uint32_t op = bam_rd32(c + 4 * (int64_t)j);
        dst[j] = op;
        if ((op & 15u) == 1u) ins += op >> 4;
    }
    return ins;
}

// ---------------------------------------------------------------------------------------------
// SEQ of records that have none (PR_BAM_RESTORE_SEQ; stock `bwa mem -a` and minimap2 print `*` on
// FLAG 0x100 records).  The rule, for a kept record r with l_seq == 0:
//   1. key    the QNAME bytes plus FLAG & 0xC0 (first / second mate).
//   2. donor  the record of the whole stream (kept or not, on any reference) with the same key,
//             l_seq > 0, FLAG & 0x904 == 0 (not secondary, supplementary or unmapped) and no H op
//             in its CIGAR; of several the lowest record index.  None: PR_ERR_NOSEQ.
//   3. length q = the sum of r's M, I, S, =, X lengths, hl / ht = the length of a leading /
//             trailing H op of r (a lone H op is the leading one).  hl + q + ht must be the
//             donor's l_seq, else PR_ERR_SAM.
//   4. o      the donor's SEQ when (r.FLAG ^ donor.FLAG) & 0x10 == 0; otherwise reversed with
//             A<->T and C<->G exchanged and every other letter kept (Fasta::Seq's
//             Reverse_complement: no IUPAC complement).  QUAL is reversed alike.
//   5. result r's SEQ is o[hl : hl + q], QUAL the same slice ('!' fill and PR_ALN_NO_QUAL when
//             the donor has none); the column's l_seq is q and PR_ALN_NO_SEQ is cleared.
enum { BAM_DONOR_EXCLUDED = 0x904, BAM_MATE_BITS = 0xC0, BAM_REVERSE = 0x10 };

BAM_HD uint32_t bam_flag(const uint8_t *rec) { return bam_rd16(rec + 18); }
BAM_HD const uint8_t *bam_name_at(const uint8_t *rec) { return rec + 36; }

// FNV-1a over the name bytes (the NUL included) and the mate bits, then a 64-bit finalizer
BAM_HD uint64_t bam_key_hash(const uint8_t *rec, const Fixed &f) {
    uint64_t h = 0xcbf29ce484222325ull;
    const uint8_t *nm = bam_name_at(rec);
    for (int32_t k = 0; k < f.l_read_name; ++k) h = (h ^ nm[k]) * 0x100000001b3ull;
    h = (h ^ (bam_flag(rec) & BAM_MATE_BITS)) * 0x100000001b3ull;
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    return h;
}

// the same key: name length, name bytes, mate bits
BAM_HD bool bam_key_equal(const uint8_t *a, const Fixed &fa, const uint8_t *b, const Fixed &fb) {
    if (fa.l_read_name != fb.l_read_name || ((bam_flag(a) ^ bam_flag(b)) & BAM_MATE_BITS)) return false;
    const uint8_t *na = bam_name_at(a), *nb = bam_name_at(b);
    for (int32_t k = 0; k < fa.l_read_name; ++k)
        if (na[k] != nb[k]) return false;
    return true;
}

struct CigarSpan {
    int64_t q;         // M, I, S, =, X lengths
    int64_t hl, ht;    // leading / trailing H
    bool has_h;        // an H op anywhere
};

BAM_HD CigarSpan bam_cigar_span(const uint8_t *rec, const Fixed &f) {
    CigarSpan s;
    s.q = s.hl = s.ht = 0;
    s.has_h = false;
    const uint8_t *c = bam_cigar_at(rec, f);
    for (int32_t j = 0; j < f.n_cigar; ++j) {
        const uint32_t op = bam_rd32(c + 4 * (int64_t)j), t = op & 15u;
        const int64_t l = op >> 4;
        if (t == 0u || t == 1u || t == 4u || t == 7u || t == 8u) s.q += l;
        if (t == 5u) {
            s.has_h = true;
            if (j == 0) s.hl = l;
            else if (j == f.n_cigar - 1) s.ht = l;
        }
    }
    return s;
}

// a record that may lend its SEQ
BAM_HD bool bam_is_donor(const uint8_t *rec, const Fixed &f) {
    return f.l_seq > 0 && !(bam_flag(rec) & BAM_DONOR_EXCLUDED) && !bam_cigar_span(rec, f).has_h;
}

// the 4-bit codes of bases first .. first + 15 (all inside the SEQ), base j at bits 4 j, from the
// 8 or 9 bytes that hold them
BAM_HD uint64_t bam_codes16(const uint8_t *sb, int32_t first) {
    const uint8_t *p = sb + (first >> 1);
    uint64_t v = 0;
    if (first & 1) {
        uint32_t prev = p[0];
        for (int j = 0; j < 8; ++j) {
            const uint32_t b = p[j + 1];
            v |= (uint64_t)((prev & 15u) | (b & 0xf0u)) << (8 * j);
            prev = b;
        }
    } else {
        for (int j = 0; j < 8; ++j) {
            const uint32_t b = p[j];
            v |= (uint64_t)(((b >> 4) & 15u) | ((b & 15u) << 4)) << (8 * j);
        }
    }
    return v;
}

// A<->T (1, 8), C<->G (2, 4), every other code itself
BAM_HD uint32_t bam_code_complement(uint32_t x) { return (uint32_t)(0xFEDCBA9176523480ull >> (4 * x)) & 15u; }

// sixteen 4-bit codes in the opposite order
BAM_HD uint64_t bam_reverse_codes(uint64_t v) {
    v = ((v & 0x00000000ffffffffull) << 32) | (v >> 32);
    v = ((v & 0x0000ffff0000ffffull) << 16) | ((v >> 16) & 0x0000ffff0000ffffull);
    v = ((v & 0x00ff00ff00ff00ffull) << 8) | ((v >> 8) & 0x00ff00ff00ff00ffull);
    return ((v & 0x0f0f0f0f0f0f0f0full) << 4) | ((v >> 4) & 0x0f0f0f0f0f0f0f0full);
}

// base k of the slice [start, start + n) of a donor's SEQ of dl bases in the record's orientation
BAM_HD uint32_t bam_base_from(const uint8_t *sb, int32_t dl, int32_t start, bool rev, int32_t k) {
    const int32_t s = rev ? dl - 1 - (start + k) : start + k;
    const uint32_t x = (sb[s >> 1] >> (4 * (1 - (s & 1)))) & 15u;
    return bam_nt16_char(rev ? bam_code_complement(x) : x);
}

// SEQ from a donor: n bases o[start : start + n) at dst, o = the donor's dl bases at sb or (rev)
// their reverse complement; start + n <= dl.  The chunks are those of bam_unpack_seq.
BAM_HD void bam_unpack_seq_from(const uint8_t *sb, int32_t dl, int32_t start, int32_t n, bool rev, uint8_t *dst, int lane,
                                int nlanes) {
    const int32_t a0 = bam_line_offset(dst), nc = bam_chunks(a0, n);
    for (int32_t c = lane; c < nc; c += nlanes) {
        const int32_t k0 = 16 * c - a0;
        if (k0 >= 0 && k0 + 16 <= n) {
            // forward: bases start + k0 ..; reverse: bases dl - 1 - (start + k0) downwards
            const uint64_t v = rev ? bam_reverse_codes(bam_codes16(sb, dl - 16 - (start + k0))) : bam_codes16(sb, start + k0);
            Chunk o;
            for (int w = 0; w < 4; ++w) {
                uint32_t x = 0;
                for (int j = 0; j < 4; ++j) {
                    const uint32_t code = (uint32_t)(v >> (4 * (4 * w + j))) & 15u;
                    x |= bam_nt16_char(rev ? bam_code_complement(code) : code) << (8 * j);
                }
                o.w[w] = x;
            }
            bam_store_chunk(dst + k0, o);
        } else {
            const int32_t lo = k0 < 0 ? 0 : k0, hi = k0 + 16 < n ? k0 + 16 : n;
            for (int32_t k = lo; k < hi; ++k) dst[k] = (uint8_t)bam_base_from(sb, dl, start, rev, k);
        }
    }
}

// QUAL from a donor, the same slice and orientation (never complemented); '!' x n when absent
BAM_HD void bam_unpack_qual_from(const uint8_t *qb, int32_t dl, int32_t start, int32_t n, bool rev, bool no_qual,
                                 uint8_t *dst, int lane, int nlanes) {
    const int32_t a0 = bam_line_offset(dst), nc = bam_chunks(a0, n);
    for (int32_t c = lane; c < nc; c += nlanes) {
        const int32_t k0 = 16 * c - a0;
        if (k0 >= 0 && k0 + 16 <= n) {
            Chunk o;
            for (int w = 0; w < 4; ++w) {
                uint32_t q = 0u;
                if (!no_qual) {
                    if (rev) {
                        const uint8_t *p = qb + (dl - 1 - (start + k0 + 4 * w));   // the word's first byte, read downwards
                        q = (uint32_t)p[0] | ((uint32_t)p[-1] << 8) | ((uint32_t)p[-2] << 16) | ((uint32_t)p[-3] << 24);
                    } else {
                        q = bam_rd32(qb + start + k0 + 4 * w);
                    }
                }
                o.w[w] = ((q & 0x7f7f7f7fu) + 0x21212121u) ^ (q & 0x80808080u);
            }
            bam_store_chunk(dst + k0, o);
        } else {
            const int32_t lo = k0 < 0 ? 0 : k0, hi = k0 + 16 < n ? k0 + 16 : n;
            for (int32_t k = lo; k < hi; ++k)
                dst[k] = no_qual ? (uint8_t)'!' : (uint8_t)(qb[rev ? dl - 1 - (start + k) : start + k] + 33);
        }
    }
}

// The donor table: open addressing with linear probing over record indices, BAM_SLOT_EMPTY where
// free; a power of two of slots, at least twice the donors, so a probe always ends.
static const unsigned long long BAM_SLOT_EMPTY = ~0ull;

BAM_HD int64_t bam_table_slots(int64_t eligible) {
    int64_t cap = 16;
    while (cap < 2 * eligible) cap <<= 1;
    return cap;
}

// Donor record i (at r) into the table.  A free slot is claimed by a 64-bit compare-and-swap on
// the index; an occupant of the same key keeps the lower index (a minimum: the slot's key never
// changes); any other occupant, a hash collision included, costs one more probe.  On the device
// many lanes insert at once; a host build inserts one record after the other.
BAM_HD void bam_table_insert(unsigned long long *tab, int64_t mask, const uint8_t *recs, const int64_t *off, int64_t i,
                             const uint8_t *r, const Fixed &fr) {
    for (int64_t h = (int64_t)(bam_key_hash(r, fr) & (uint64_t)mask), step = 0; step <= mask; h = (h + 1) & mask, ++step) {
#if defined(__HIP_DEVICE_COMPILE__)
        const unsigned long long v = atomicCAS(tab + h, BAM_SLOT_EMPTY, (unsigned long long)i);
#else
        const unsigned long long v = tab[h];
        if (v == BAM_SLOT_EMPTY) tab[h] = (unsigned long long)i;
#endif
        if (v == BAM_SLOT_EMPTY) return;
        const uint8_t *o = recs + off[v];
        if (bam_key_equal(o, bam_fixed(o), r, fr)) {
#if defined(__HIP_DEVICE_COMPILE__)
            atomicMin(tab + h, (unsigned long long)i);
#else
            if ((unsigned long long)i < tab[h]) tab[h] = (unsigned long long)i;
#endif
            return;
        }
    }
}

// The donor of record r in a filled table (its key hashed and compared by full name), or -1
BAM_HD int64_t bam_table_find(const unsigned long long *tab, int64_t mask, const uint8_t *recs, const int64_t *off,
                              const uint8_t *r, const Fixed &fr) {
    for (int64_t h = (int64_t)(bam_key_hash(r, fr) & (uint64_t)mask), step = 0; step <= mask; h = (h + 1) & mask, ++step) {
        const unsigned long long v = tab[h];
        if (v == BAM_SLOT_EMPTY) return -1;
        const uint8_t *o = recs + off[v];
        if (bam_key_equal(o, bam_fixed(o), r, fr)) return (int64_t)v;
    }
    return -1;
}

}   // namespace bam
}   // namespace prgpu

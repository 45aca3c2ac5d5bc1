// BAM record encoding shared by the device encoder (bam_enc_kernels.hip), its host entry
// (bam_api.cpp) and host builds (tests/native/bam_enc_host.cpp): the inverse of bam_core.h.  One
// record is what pr_sam_encode (bam_codec.cpp) makes of the SAM line pr_sw_sam prints for an
// alignment of the hand-off: the fixed fields, the read name, the CIGAR ops as the SW stage left
// them (len << 4 | op), SEQ as 4-bit codes from the short read's nt4 bases, QUAL as phred, and one
// aux field, AS, in the smallest integer type that holds the score.
//
//   enc_layout       where the parts of a record start, and its size
//   enc_span_part    a lane's share of the CIGAR's reference span (the bin needs the sum)
//   enc_write        the record's bytes, by one lane or spread over nl lanes
//
// A record lands at an arbitrary byte offset of the stream, so its bytes are written as the
// decoder's unpack pass writes its pools: the destination is cut into 16-byte chunks at 16-byte
// aligned addresses, lane l takes chunks l, l + nl, ..; a chunk that lies inside the record is one
// aligned 16-byte store, the partial chunks at the record's two ends are byte stores.  No word is
// ever stored at a misaligned address, and no byte outside the record is touched.
//
// The short reads are held as nt4 (A 0, C 1, G 2, T 3, anything else 4): a base that is not
// A, C, G or T is written as N (code 15) on both strands.
#pragma once
#include <stdint.h>

#include "bam_core.h"

namespace prgpu {
namespace bam {

// one alignment of the hand-off, as the encoder reads it
struct EncRec {
    int32_t rid;            // refID: the long read's index
    int32_t pos;            // 0-based leftmost position
    int32_t flag;           // SAM FLAG
    int32_t score;          // AS
    int32_t l_name;         // bytes of the read name (without the NUL), 1 .. 254
    int32_t n_cigar, l_seq;
    int32_t rev;            // reverse strand: SEQ reverse-complemented, QUAL reversed
    const uint8_t *name;
    const uint32_t *cig;    // n_cigar ops (4-byte aligned)
    const uint8_t *seq;     // l_seq nt4 bases, in the read's own direction
    const uint8_t *qual;    // l_seq bytes phred + 33, in the read's own direction, or NULL
};

// byte offsets of a record's parts from its block_size word
struct EncLayout {
    int32_t cig, seq, qual, aux, size;
    int32_t as_width;       // 1, 2 or 4
    uint8_t as_type;        // c C s S i
};

// pr_sam_encode's choice for an :i: value (bam_codec.cpp:155-165); an int32 never needs 'I'
BAM_HD uint8_t enc_as_type(int32_t v) {
    return (v >= -128 && v <= 127) ? 'c' : (v >= 0 && v <= 255) ? 'C' : (v >= -32768 && v <= 32767) ? 's'
         : (v >= 0 && v <= 65535) ? 'S' : 'i';
}

BAM_HD EncLayout enc_layout(int32_t l_name, int32_t n_cigar, int32_t l_seq, int32_t score) {
    EncLayout L;
    L.as_type = enc_as_type(score);
    L.as_width = bam_int_size(L.as_type);
    L.cig = 36 + l_name + 1;
    L.seq = L.cig + 4 * n_cigar;
    L.qual = L.seq + (l_seq + 1) / 2;
    L.aux = L.qual + l_seq;
    L.size = L.aux + 3 + L.as_width;
    return L;
}

// the size of one record, its block_size word included
BAM_HD int64_t enc_size(int32_t l_name, int32_t n_cigar, int32_t l_seq, int32_t score) {
    return enc_layout(l_name, n_cigar, l_seq, score).size;
}

// bam_codec.cpp:52-60
BAM_HD uint32_t enc_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// a lane's share of the reference span: the lengths of its M, D, N, = and X ops
BAM_HD int64_t enc_span_part(const uint32_t *cig, int32_t n, int lane, int nl) {
    int64_t s = 0;
    for (int32_t j = lane; j < n; j += nl) {
        const uint32_t x = cig[j], op = x & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) s += x >> 4;
    }
    return s;
}

// word w (0 .. 8) of the 36 fixed bytes
BAM_HD uint32_t enc_fixed_word(const EncRec &R, const EncLayout &L, int64_t span, int w) {
    switch (w) {
        case 0: return (uint32_t)(L.size - 4);
        case 1: return (uint32_t)R.rid;
        case 2: return (uint32_t)R.pos;
        case 3: {
            const uint32_t bin = R.pos >= 0 ? enc_reg2bin(R.pos, (int64_t)R.pos + (span ? span : 1)) : 4680u;
            const uint32_t mapq = (R.flag & 0x100) ? 0u : 60u;
            return (uint32_t)(R.l_name + 1) | (mapq << 8) | (bin << 16);
        }
        case 4: return ((uint32_t)R.n_cigar & 0xffffu) | (((uint32_t)R.flag & 0xffffu) << 16);
        case 5: return (uint32_t)R.l_seq;
        case 6: return 0xffffffffu;   // next_refID -1
        case 7: return 0xffffffffu;   // next_pos -1
        default: return 0u;           // tlen
    }
}

// Byte k of the record is made of at most two source bytes: a name byte, a byte of a CIGAR op, two
// bases, or a quality.  enc_sources says where they are -- both pointers are always readable, a
// byte that needs no source points at the name -- and enc_value makes the byte of them.  Split so
// that a chunk's 32 loads are issued together, with no branch between them, and waited for once:
// with a load inside each part's branch every byte of a chunk waits for memory in turn.
BAM_HD int32_t enc_src_index(const EncRec &R, int32_t i) { return R.rev ? R.l_seq - 1 - i : i; }
BAM_HD void enc_sources(const EncRec &R, const EncLayout &L, int32_t k, const uint8_t *&pa, const uint8_t *&pb) {
    pa = pb = R.name;
    if (k >= 36 && k < L.cig - 1) {
        pa = R.name + (k - 36);
    } else if (k >= L.cig && k < L.seq) {
        pa = reinterpret_cast<const uint8_t *>(R.cig) + (k - L.cig);   // (little-endian words, as the record holds them)
    } else if (k >= L.seq && k < L.qual) {
        const int32_t i = 2 * (k - L.seq);
        pa = R.seq + enc_src_index(R, i);
        pb = R.seq + enc_src_index(R, i + 1 < R.l_seq ? i + 1 : i);
    } else if (k >= L.qual && k < L.aux && R.qual) {
        pa = R.qual + enc_src_index(R, k - L.qual);
    }
}
// 4-bit code of an nt4 base: A C G T -> 1 2 4 8 (8 4 2 1 on the reverse strand), anything else 15
BAM_HD uint32_t enc_code(const EncRec &R, uint32_t b) {
    return ((R.rev ? 0xF1248u : 0xF8421u) >> (4 * (b > 4u ? 4u : b))) & 15u;
}
BAM_HD uint32_t enc_value(const EncRec &R, const EncLayout &L, int64_t span, int32_t k, uint32_t a, uint32_t b) {
    if (k < 36) return (enc_fixed_word(R, L, span, k >> 2) >> (8 * (k & 3))) & 255u;
    if (k < L.cig) return k < L.cig - 1 ? a : 0u;
    if (k < L.seq) return a;
    if (k < L.qual) return (enc_code(R, a) << 4) | (2 * (k - L.seq) + 1 < R.l_seq ? enc_code(R, b) : 0u);
    if (k < L.aux) return R.qual ? (a - 33u) & 255u : 0xFFu;
    const int32_t x = k - L.aux;
    if (x < 3) return x == 0 ? 'A' : x == 1 ? 'S' : L.as_type;
    return ((uint32_t)R.score >> (8 * (x - 3))) & 255u;
}

// the 16 bytes k0 .. k0 + 15 of the record (positions outside the record repeat its nearest byte)
BAM_HD Chunk enc_chunk(const EncRec &R, const EncLayout &L, int64_t span, int32_t k0) {
    uint32_t a[16], b[16];
    for (int j = 0; j < 16; ++j) {
        const int32_t k = k0 + j < 0 ? 0 : (k0 + j < L.size ? k0 + j : L.size - 1);
        const uint8_t *pa, *pb;
        enc_sources(R, L, k, pa, pb);
        a[j] = *pa;
        b[j] = *pb;
    }
    Chunk o;
    for (int w = 0; w < 4; ++w) {
        uint32_t x = 0;
        for (int j = 0; j < 4; ++j) {
            const int32_t k = k0 + 4 * w + j < 0 ? 0 : (k0 + 4 * w + j < L.size ? k0 + 4 * w + j : L.size - 1);
            x |= enc_value(R, L, span, k, a[4 * w + j], b[4 * w + j]) << (8 * j);
        }
        o.w[w] = x;
    }
    return o;
}

// The record's bytes at dst.  span: the CIGAR's reference span (the sum of enc_span_part over the
// lanes).  Lane `lane` of `nl` writes chunks lane, lane + nl, ..
BAM_HD void enc_write(const EncRec &R, int64_t span, uint8_t *dst, int lane, int nl) {
    const EncLayout L = enc_layout(R.l_name, R.n_cigar, R.l_seq, R.score);
    const int32_t a0 = bam_line_offset(dst), nc = bam_chunks(a0, L.size);
    for (int32_t c = lane; c < nc; c += nl) {
        const int32_t k0 = 16 * c - a0;
        const Chunk o = enc_chunk(R, L, span, k0);
        if (k0 >= 0 && k0 + 16 <= L.size) {
            bam_store_chunk(dst + k0, o);
        } else {   // the record's first or last chunk: its own bytes only
            const int32_t lo = k0 < 0 ? 0 : k0, hi = k0 + 16 < L.size ? k0 + 16 : L.size;
            for (int32_t k = lo; k < hi; ++k) dst[k] = (uint8_t)(o.w[(k - k0) >> 2] >> (8 * ((k - k0) & 3)));
        }
    }
}

}   // namespace bam
}   // namespace prgpu

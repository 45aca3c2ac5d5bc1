// Sam::Seq's State_matrix / state_matrix_consensus (Seq.pm:232-467, 1568-1654), stated once for
// the stages that port it: ccs-1 (ccs_core.h) and the unitig consensus (utg_core.h).  HIP-free;
// everything is CC_HD, so the host paths, the kernels and the host tests run the same code.
// DESIGN.md §15 names the pieces.
//
//   trim    prep_trim: the head and tail trim of an alignment, the skips of Seq.pm:354 and :384
//   states  entry_of_op: the state a CIGAR op gives a column, and its weight (Seq.pm:396-459)
//   vote    decide_col over a source of alignments, pick_len / pick_emit (Seq.pm:1568-1650)
//
// A stage differs only in where a column's states come from.  It hands decide_col a source:
//   int     count()                   the alignments, in arrival order
//   ColEnt  entry(int k, int c)       the state of alignment k in column c, slen < 0 where none
//   Read    read(int k)               the query of alignment k in its aligned orientation
//   bool    ignored(int c)            the alignments add nothing to column c
//   int64_t first_seen(x, xo, n)      rank of the insertion state x[xo, xo + n): lower wins a tie
//
// What keeps the vote byte-identical to the Perl:
//   - the reference's own weight is added first, and only when use_ref_qual && ref.qual and it
//     is not zero
//   - the alignments are added in source order into six separate doubles
//   - the fixed states are argmaxed by "first index strictly greater" over A T G C - N
//   - an insertion state is skipped if an earlier alignment carries the same state; otherwise it
//     is summed from its first carrier onwards in source order
//   - max_ins_length (0: none) filters the insertion states by slen
//   - an equal, non-zero sum of two insertion states goes to the lower first_seen
//   - bases are read through base_at (rev-aware) in the vote, in same_state and in the emit
//   - no arithmetic on doubles is reordered or fused: the build keeps -ffp-contract=off
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define CC_HD __host__ __device__ inline
#else
#define CC_HD inline
#endif

namespace prgpu {
namespace sm {

enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4, OP_H = 5 };

// what the trim, the states and the vote read; a stage fills it once from its public params
struct Params {
    int32_t trim, min_aln_length, phred_offset, ref_phred_offset;
    double indel_taboo;           // InDelTaboo, used when indel_taboo_length is 0
    int32_t indel_taboo_length;
    int32_t use_ref_qual, qual_weighted, max_ins_length;
};

// a sequence in an orientation: rev reads the reverse complement, qualities reversed
struct Read {
    const uint8_t *seq, *qual;
    int32_t len, rev;
};
CC_HD uint8_t comp_of(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
CC_HD uint8_t base_at(const Read &r, int x) { return r.rev ? comp_of(r.seq[r.len - 1 - x]) : r.seq[x]; }
CC_HD uint8_t qual_at(const Read &r, int x) { return r.rev ? r.qual[r.len - 1 - x] : r.qual[x]; }

// Seq.pm:151-156 Phreds2freqs, :136-142 Freqs2phreds
CC_HD double phred2freq(int p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double x = __dadd_rn(__dmul_rn(__ddiv_rn(__dmul_rn((double)p, (double)p), 120.0), 100.0), 0.5);
    return __ddiv_rn((double)(long long)x, 100.0);
#else
    const double x = ((double)p * (double)p / 120.0) * 100.0 + 0.5;
    return (double)(long long)x / 100.0;
#endif
}
CC_HD int freq2phred(double f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double x = __dadd_rn(__dsqrt_rn(__dmul_rn(f, 120.0)), 0.5);
#else
    const double x = std::sqrt(f * 120.0) + 0.5;
#endif
    const long long p = (long long)x;
    return p > 40 ? 40 : (int)p;
}
// Seq.pm:531-539: A T G C - N
CC_HD int fixed_idx(uint8_t c) { return c == 'A' ? 0 : c == 'T' ? 1 : c == 'G' ? 2 : c == 'C' ? 3 : c == '-' ? 4 : 5; }
CC_HD uint8_t fixed_chr(int idx) { return (uint8_t)("ATGC-N"[idx]); }

struct AlnView {
    Read q;   // in the aligned orientation
    int32_t pos;
    const uint32_t *cig;
    int32_t ncig;
};
// what State_matrix keeps of an alignment: CIGAR ops [cb, ce), query window [wb, we), first column
struct Prep {
    int32_t use;   // 1 added, 0 skipped (Seq.pm:277, 354, 384), -1 malformed or leaving the reference
    int32_t cb, ce, wb, we, rpos, lead;
};
// one state of an alignment in a reference column: the query bytes [qoff, qoff + slen) of the
// aligned orientation; slen 0 a deletion, -1 no state; w its weight
struct ColEnt {
    int32_t qoff, slen;
    double w;
};

// the trim of State_matrix (Seq.pm:316-385) over the ops [cb, ce) left after the clips were
// stripped, query window [wb, we)
CC_HD Prep prep_trim(const Params &p, const AlnView &a, int ref_len, int cb, int ce, int wb, int we) {
    Prep r = {0, 0, 0, 0, 0, 0, 0};
    const int orig = a.q.len;
    long rpos = a.pos;
    if (p.trim) {
        long mc = 0, dc = 0, ic = 0;
        const long taboo = p.indel_taboo_length ? (long)p.indel_taboo_length : (long)((double)orig * p.indel_taboo + 0.5);
        for (int i = cb; i < ce; ++i) {
            const int op = (int)(a.cig[i] & 15);
            const long n = (long)(a.cig[i] >> 4);
            if (op == OP_M) {
                if (mc + ic + n > taboo) {
                    if (i > cb) cb = i, rpos += mc + dc, wb += (int)(mc + ic);
                    break;
                }
                mc += n;
            } else if (op == OP_D) {
                dc += n;
            } else {
                ic += n;
            }
        }
        if (we - wb < 50 || ((double)(we - wb) / (double)orig) < 0.7) return r;   // Seq.pm:354
        long tail = 0;
        for (int i = ce - 1; i != cb; --i) {   // never visits the first op
            const int op = (int)(a.cig[i] & 15);
            const long n = (long)(a.cig[i] >> 4);
            if (op == OP_M) {
                tail += n;
                if (tail > taboo) {
                    if (i < ce - 1) ce = i + 1, we -= (int)(tail - n);
                    break;
                }
            } else if (op == OP_I) {
                tail += n;
            }
        }
        if (we - wb < p.min_aln_length || ((double)(we - wb) / (double)orig) < 0.7) return r;   // Seq.pm:384
    }
    r.cb = cb, r.ce = ce, r.wb = wb, r.we = we, r.rpos = (int32_t)rpos, r.lead = (a.cig[cb] & 15) == OP_I;
    long cols = r.lead, q = 0;
    for (int i = cb; i < ce; ++i) {
        const int op = (int)(a.cig[i] & 15);
        if (op != OP_I) cols += (long)(a.cig[i] >> 4);
        if (op != OP_D) q += (long)(a.cig[i] >> 4);
    }
    r.use = (rpos < 0 || rpos + cols > ref_len || q != we - wb) ? -1 : 1;
    return r;
}

// min(Phreds2freqs(quals)) of the query bytes [qoff, qoff + n)
CC_HD double state_weight(const Params &p, const Read &q, int qoff, int n) {
    double m = 0.0;
    for (int t = 0; t < n; ++t) {
        const double f = phred2freq((int)qual_at(q, qoff + t) - p.phred_offset);
        if (t == 0 || f < m) m = f;
    }
    return m;
}
// Seq.pm:402-408: the lesser of the qualities around a deletion at window position qpos
CC_HD double del_weight(const Params &p, const Read &q, const Prep &pr, int qpos) {
    const int n = pr.we - pr.wb;
    const int xb = qpos > 1 ? qpos - 1 : qpos, xa = qpos < n ? qpos : qpos - 1;
    const int qb = (xb >= 0 && xb < n) ? (int)qual_at(q, pr.wb + xb) : 0;
    const int qa = (xa >= 0 && xa < n) ? (int)qual_at(q, pr.wb + xa) : 0;
    const int c = qb < qa ? qb : qa;
    return c ? phred2freq(c - p.phred_offset) : 0.0;
}
// the insertions that follow op i join the state before them (Seq.pm:412-424)
CC_HD int ins_after(const AlnView &a, const Prep &pr, int i) {
    int tot = 0;
    for (int k = i + 1; k < pr.ce && (a.cig[k] & 15) == OP_I; ++k) tot += (int)(a.cig[k] >> 4);
    return tot;
}
// first column / window position of the op after op i
CC_HD void advance_op(const AlnView &a, const Prep &pr, int i, int &r, int &q) {
    const int op = (int)(a.cig[i] & 15), n = (int)(a.cig[i] >> 4);
    if (op != OP_I) r += n;
    else if (i == pr.cb) r += 1;
    if (op != OP_D) q += n;
}

// the state op i (first column r, window position q) gives column c: query bytes
// [qoff, qoff + slen), slen 0 a deletion (Seq.pm:396-432; a leading insertion is a column of
// its own, the insertions behind an op join its last column, D+I is one replaced state)
CC_HD ColEnt state_of_op(const AlnView &a, const Prep &pr, int i, int r, int q, int c) {
    const int op = (int)(a.cig[i] & 15), n = (int)(a.cig[i] >> 4);
    if (op == OP_I) return ColEnt{pr.wb + q, n + ins_after(a, pr, i), 0.0};
    const int ins = c - r == n - 1 ? ins_after(a, pr, i) : 0;
    if (op == OP_M) return ColEnt{pr.wb + q + (c - r), 1 + ins, 0.0};
    return ColEnt{pr.wb + q, ins, 0.0};
}
// ... with its weight: min(Phreds2freqs) or 1 (Seq.pm:450-459)
CC_HD ColEnt entry_of_op(const Params &p, const AlnView &a, const Prep &pr, int i, int r, int q, int c) {
    ColEnt e = state_of_op(a, pr, i, r, q, c);
    if (!p.qual_weighted) e.w = 1.0;
    else if (e.slen > 0) e.w = state_weight(p, a.q, e.qoff, e.slen);
    else e.w = del_weight(p, a.q, pr, q);
    return e;
}

CC_HD bool same_state(const Read &x, int xo, const Read &y, int yo, int n) {
    for (int t = 0; t < n; ++t)
        if (base_at(x, xo + t) != base_at(y, yo + t)) return false;
    return true;
}

// the consensus state of a column: kind 0 uncovered (the reference base), 1 a fixed state
// (idx; 4 is the gap), 2 the bytes [qoff, qoff + slen) of the source's alignment k; f its sum
struct Pick {
    int32_t kind, idx, k;
    double f;
    int32_t qoff, slen;
};
template <class Src>
CC_HD Pick decide_col(const Params &p, const Read &ref, int c, const Src &src) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0;
    auto add = [&](int idx, double w) {
        s0 += idx == 0 ? w : 0.0, s1 += idx == 1 ? w : 0.0, s2 += idx == 2 ? w : 0.0;
        s3 += idx == 3 ? w : 0.0, s4 += idx == 4 ? w : 0.0, s5 += idx == 5 ? w : 0.0;
    };
    if (p.use_ref_qual && ref.qual) {   // Seq.pm:256-266
        const double fr = phred2freq((int)ref.qual[c] - p.ref_phred_offset);
        if (fr != 0.0) add(fixed_idx(ref.seq[c]), fr);
    }
    const int m = src.ignored(c) ? 0 : src.count();
    bool multi = false;
    for (int k = 0; k < m; ++k) {
        const Read q = src.read(k);   // asked for before the state, so that a source's loads for the two overlap
        const ColEnt e = src.entry(k, c);
        if (e.slen == 0) add(4, e.w);
        else if (e.slen == 1) add(fixed_idx(base_at(q, e.qoff)), e.w);
        else if (e.slen > 1) multi = true;
    }
    Pick pk = {0, 0, -1, 0.0, 0, 0};
    const double s[6] = {s0, s1, s2, s3, s4, s5};
    for (int i = 0; i < 6; ++i)
        if (s[i] > pk.f) pk.f = s[i], pk.kind = 1, pk.idx = i;
    if (!multi) return pk;
    for (int k = 0; k < m; ++k) {
        const Read x = src.read(k);
        const ColEnt e = src.entry(k, c);
        if (e.slen <= 1 || (p.max_ins_length && e.slen > p.max_ins_length)) continue;   // Seq.pm:1607
        bool seen = false;
        double sum = 0.0;
        for (int j = 0; j < m && !seen; ++j) {
            const Read y = src.read(j);
            const ColEnt g = src.entry(j, c);
            if (g.slen != e.slen || !same_state(y, g.qoff, x, e.qoff, e.slen)) continue;
            if (j < k) seen = true;
            else sum += g.w;
        }
        if (seen) continue;
        if (sum > pk.f) {
            pk.f = sum, pk.kind = 2, pk.k = k, pk.qoff = e.qoff, pk.slen = e.slen;
        } else if (sum == pk.f && sum > 0.0 && pk.kind == 2) {
            // equal sums of two insertion states: the lower state index wins, the index is the
            // rank of the state's first occurrence (Seq.pm:441-448, 1593-1611)
            if (src.first_seen(x, e.qoff, e.slen) < src.first_seen(src.read(pk.k), pk.qoff, pk.slen))
                pk.k = k, pk.qoff = e.qoff, pk.slen = e.slen;
        }
    }
    return pk;
}
// bases and trace characters a column emits (Seq.pm:1616-1650)
CC_HD void pick_len(const Pick &pk, int &nseq, int &ntrace) {
    if (pk.kind == 1 && pk.idx == 4) nseq = 0, ntrace = 1;
    else if (pk.kind == 2) nseq = ntrace = pk.slen;
    else nseq = ntrace = 1;
}
template <class Src>
CC_HD void pick_emit(const Params &p, const Pick &pk, const Read &ref, int c, const Src &src, uint8_t *seq, uint8_t *qual,
                     uint8_t *trace) {
    if (pk.kind == 1 && pk.idx == 4) {
        trace[0] = 'I';
        return;
    }
    const uint8_t ph = (uint8_t)(freq2phred(pk.f) + p.phred_offset);
    trace[0] = 'M';
    if (pk.kind == 2) {
        const Read q = src.read(pk.k);
        for (int t = 0; t < pk.slen; ++t) {
            seq[t] = base_at(q, pk.qoff + t), qual[t] = ph;
            if (t) trace[t] = 'D';
        }
    } else {
        seq[0] = pk.kind == 1 ? fixed_chr(pk.idx) : ref.seq[c];
        qual[0] = ph;
    }
}

}   // namespace sm
}   // namespace prgpu

// ccs-1 (bin/ccseq): the rules of the stage, shared by the host path (ccs_api.cpp), the kernels
// (ccs_kernels.hip) and the host tests.  HIP-free; DESIGN.md §13 states the same rules in prose.
//
//   grouping   ccseq:237-299 and :356-363, restated line by line (group_ids)
//   mapping    replaces bwa-proovread: exact seeds (maximal runs of matching cells, length >= k)
//              vote per orientation and per bucket of w diagonals; the longest seed of the best
//              pair of adjacent buckets gives the band centre d0; one banded local alignment
//              over |(i - j) - d0| <= w with ksw_global2's cell (oracle/sw_oracle.c: gaps open
//              from the diagonal value, M >= E >= F, extend only when strictly better than
//              open), H floored at 0, first maximal cell in (i, j) order, traceback until H = 0
//   consensus  Sam::Seq State_matrix / state_matrix_consensus (Seq.pm:232-467, 1568-1654) with
//              Trim 1, InDelTaboo 0.001, use_ref_qual, qual_weighted: per alignment a column
//              map (query offset, state length, weight); per column the six fixed states in
//              registers and the insertion states compared as strings, sums in double in
//              arrival order, ties between insertion states by global first-seen rank
// The pieces marked CC_HD are the ones the kernels call.
#pragma once
#include <stdint.h>

#include "../../include/prgpu.h"

#if defined(__HIPCC__)
#define CC_HD __host__ __device__ inline
#else
#define CC_HD inline
#endif

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace prgpu {
namespace ccs {

constexpr int NEG = -0x40000000;
enum { DIR_SRC = 3, DIR_EEXT = 4, DIR_FEXT = 8, DIR_STOP = 16 };
enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4 };

// a subread in an orientation: rev reads the reverse complement, qualities reversed
struct Read {
    const uint8_t *seq, *qual;
    int32_t len, rev;
};
CC_HD int code_of(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }
CC_HD uint8_t comp_of(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
CC_HD uint8_t base_at(const Read &r, int x) { return r.rev ? comp_of(r.seq[r.len - 1 - x]) : r.seq[x]; }
CC_HD uint8_t qual_at(const Read &r, int x) { return r.rev ? r.qual[r.len - 1 - x] : r.qual[x]; }
CC_HD int code_at(const Read &r, int x) { return code_of(base_at(r, x)); }
// osw_fill_scmat: match a, mismatch -b, any N -1
CC_HD int score_of(const pr_ccs_params &p, int r, int q) { return (r > 3 || q > 3) ? -1 : (r == q ? p.a : -p.b); }

// ---------------------------------------------------------------------------
// grouping (ccseq:237-299, :356-363)

// length of the ZMW part of a PacBio subread id, ^(m[^/]+/\d+)/(\d+_\d+), or -1
inline int zmw_prefix(const char *s, int n) {
    int i = 0;
    if (n < 1 || s[0] != 'm') return -1;
    for (i = 1; i < n && s[i] != '/'; ++i) {}
    if (i < 2 || i >= n) return -1;
    int j = i + 1, d0 = j;
    while (j < n && s[j] >= '0' && s[j] <= '9') ++j;
    if (j == d0 || j >= n || s[j] != '/') return -1;
    const int zl = j;
    int k = j + 1, d1 = k;
    while (k < n && s[k] >= '0' && s[k] <= '9') ++k;
    if (k == d1 || k >= n || s[k] != '_') return -1;
    return (k + 1 < n && s[k + 1] >= '0' && s[k + 1] <= '9') ? zl : -1;
}

// role / group of every record; returns the number of groups, or -1 with the offending record
inline int group_ids(int32_t n, const char *ids, const int64_t *id_off, const int32_t *len, int32_t *role, int32_t *group,
                     int32_t *bad_kind, int32_t *bad_index) {
    *bad_kind = PR_CCS_ID_OK;
    *bad_index = -1;
    std::vector<std::string> seen;
    seen.reserve((size_t)n);
    std::vector<int32_t> cache;   // @sr_cache
    std::string cid;
    int32_t ng = 0;
    auto close_group = [&]() {
        // ccseq:356-363: two subreads, the first only if strictly longer; more, the second
        const int32_t ref = cache.size() == 2 ? (len[cache[0]] > len[cache[1]] ? cache[0] : cache[1]) : cache[1];
        for (int32_t s : cache) group[s] = ng;
        role[ref] = PR_CCS_PRIMARY;
        ++ng;
    };
    {
        std::vector<std::string> sorted;
        for (int32_t r = 0; r < n; ++r) {
            const char *s = ids + id_off[r];
            const int l = (int)(id_off[r + 1] - id_off[r]);
            if (zmw_prefix(s, l) < 0) {
                *bad_kind = PR_CCS_ID_NOT_SUBREAD, *bad_index = r;
                break;
            }
            sorted.emplace_back(s, (size_t)l);
        }
        // ccseq:243: the first record whose id was seen before (the check follows the pattern's)
        const int32_t upto = *bad_index < 0 ? n : *bad_index;
        std::vector<int32_t> ord((size_t)upto);
        for (int32_t r = 0; r < upto; ++r) ord[r] = r;
        std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return sorted[x] < sorted[y]; });
        int32_t dup = -1;
        for (int32_t q = 1; q < upto; ++q)
            if (sorted[ord[q]] == sorted[ord[q - 1]] && (dup < 0 || ord[q] < dup)) dup = ord[q];
        if (dup >= 0) *bad_kind = PR_CCS_ID_NOT_UNIQUE, *bad_index = dup;
        if (*bad_index >= 0) return -1;
    }
    for (int32_t r = 0; r < n; ++r) {
        const char *s = ids + id_off[r];
        const int l = (int)(id_off[r + 1] - id_off[r]);
        const std::string id(s, (size_t)zmw_prefix(s, l));
        role[r] = PR_CCS_SECONDARY;
        group[r] = -1;
        if (r && id == cid) {
            cache.push_back(r);
        } else {
            if (cache.size() > 1) close_group();
            else if (cache.size() == 1) role[cache[0]] = PR_CCS_SINGLE;
            cid = id;
            cache.assign(1, r);
        }
    }
    // ccseq:296-299: no elsif, so a lone last record stays 'secondary' and is never written
    if (cache.size() > 1) close_group();
    return ng;
}

// ---------------------------------------------------------------------------
// seeds and band centre

struct Centre {
    int32_t found, rev, d0;
};
// order key of a seed inside a bucket: longest, then smallest i, then smallest diagonal
CC_HD uint64_t seed_key(int len, int i, int dshift) {
    return (uint64_t)len << 40 | (uint64_t)(0xFFFFF - i) << 20 | (uint64_t)(0xFFFFF - dshift);
}
CC_HD int key_dshift(uint64_t key) { return 0xFFFFF - (int)(key & 0xFFFFF); }
// diagonal d = i - j as dshift = d + lq - 1 in [0, lr + lq - 2]; bucket = dshift / w
CC_HD int n_buckets(int lr, int lq, int w) { return (lr + lq - 2) / w + 1; }

// every maximal run of matching cells of diagonal d with length >= k: emit(i, len)
template <class RF, class QF, class Emit>
CC_HD void diag_seeds(RF rc, int lr, QF qc, int lq, int d, int k, Emit emit) {
    int i = d > 0 ? d : 0, j = i - d, run = 0;
    for (; i < lr && j < lq; ++i, ++j) {
        const int a = rc(i), b = qc(j);
        if (a < 4 && a == b) {
            ++run;
        } else {
            if (run >= k) emit(i - run, run);
            run = 0;
        }
    }
    if (run >= k) emit(i - run, run);
}

// the winner among pair sums in (orientation, bucket) order: strictly greater replaces
struct PairBest {
    uint32_t sum;
    int32_t rev, b;
};
CC_HD bool pair_better(const PairBest &x, const PairBest &y) {   // x before y
    if (x.sum != y.sum) return x.sum > y.sum;
    if (x.rev != y.rev) return x.rev < y.rev;
    return x.b < y.b;
}

// sum / key: [2][nb + 1] per orientation, entry nb zero
inline Centre pick_centre(const uint32_t *sum, const uint64_t *key, int nb, int lq) {
    PairBest best = {0, 0, 0};
    for (int o = 0; o < 2; ++o)
        for (int b = 0; b < nb; ++b) {
            const PairBest c = {sum[o * (nb + 1) + b] + sum[o * (nb + 1) + b + 1], o, b};
            if (c.sum > best.sum) best = c;
        }
    Centre c = {0, 0, 0};
    if (!best.sum) return c;
    const uint64_t k0 = key[best.rev * (nb + 1) + best.b], k1 = key[best.rev * (nb + 1) + best.b + 1];
    c.found = 1, c.rev = best.rev, c.d0 = key_dshift(k0 > k1 ? k0 : k1) - (lq - 1);
    return c;
}

inline Centre centre_host(const pr_ccs_params &p, const Read &R, const Read &Qf) {
    const int lr = R.len, lq = Qf.len;
    Centre none = {0, 0, 0};
    if (lr < 1 || lq < 1) return none;
    const int nb = n_buckets(lr, lq, p.w);
    std::vector<uint32_t> sum((size_t)2 * (nb + 1), 0);
    std::vector<uint64_t> key((size_t)2 * (nb + 1), 0);
    std::vector<uint8_t> rc((size_t)lr), qc((size_t)lq);
    for (int i = 0; i < lr; ++i) rc[i] = (uint8_t)code_at(R, i);
    for (int o = 0; o < 2; ++o) {
        Read Q = Qf;
        Q.rev = o;
        for (int j = 0; j < lq; ++j) qc[j] = (uint8_t)code_at(Q, j);
        for (int d = -(lq - 1); d <= lr - 1; ++d) {
            const int ds = d + lq - 1, b = ds / p.w;
            diag_seeds([&](int i) { return (int)rc[i]; }, lr, [&](int j) { return (int)qc[j]; }, lq, d, p.k,
                       [&](int i, int len) {
                           sum[o * (nb + 1) + b] += (uint32_t)len;
                           key[o * (nb + 1) + b] = std::max(key[o * (nb + 1) + b], seed_key(len, i, ds));
                       });
        }
    }
    return pick_centre(sum.data(), key.data(), nb, lq);
}

// ---------------------------------------------------------------------------
// banded local alignment

struct Cell {
    int32_t h, e, f;   // H(i, j); E arriving at (i + 1, j); F arriving at (i, j + 1)
    uint8_t d;
};
// hd = H(i-1, j-1), e = E arriving at (i, j), f = F arriving at (i, j), s = the cell's score
CC_HD Cell dp_cell(const pr_ccs_params &p, int hd, int e, int f, int s) {
    Cell c;
    const int mm = hd + s;
    uint8_t d = mm >= e ? 0 : 1;
    int h = mm >= e ? mm : e;
    d = h >= f ? d : 2;
    h = h >= f ? h : f;
    if (h <= 0) h = 0, d |= DIR_STOP;
    int t = mm - (p.o_del + p.e_del);
    e -= p.e_del;
    if (e > t) d |= DIR_EEXT;
    c.e = e > t ? e : t;
    t = mm - (p.o_ins + p.e_ins);
    f -= p.e_ins;
    if (f > t) d |= DIR_FEXT;
    c.f = f > t ? f : t;
    c.h = h, c.d = d;
    return c;
}
// rows of the band: the reference positions that have a cell
CC_HD int row_lo(int d0, int w) { return d0 - w > 0 ? d0 - w : 0; }
CC_HD int row_hi(int lr, int lq, int d0, int w) { return lr - 1 < lq - 1 + d0 + w ? lr - 1 : lq - 1 + d0 + w; }
// one step of the traceback in a cell with direction byte d: the op consumed, or -1 at H = 0
CC_HD int tb_step(int &state, uint8_t d) {
    if (state == 0) {
        if (d & DIR_STOP) return -1;
        state = d & DIR_SRC;
    } else if (state == 1) {
        state = (d & DIR_EEXT) ? 1 : 0;
    } else {
        state = (d & DIR_FEXT) ? 2 : 0;
    }
    return state == 0 ? OP_M : state == 1 ? OP_D : OP_I;
}

struct Aln {
    int32_t mapped, strand, pos, score, n_cigar;
};

// the alignment of Q (oriented) to R around diagonal d0; cigar: the subread's slot
inline Aln align_host(const pr_ccs_params &p, const Read &R, const Read &Q, int d0, std::vector<uint8_t> &dir,
                      uint32_t *cigar) {
    const int lr = R.len, lq = Q.len, w = p.w, W = 2 * w + 1;
    const int i0 = row_lo(d0, w), i1 = row_hi(lr, lq, d0, w);
    Aln out = {0, Q.rev, 0, 0, 0};
    if (i1 < i0) return out;
    dir.assign((size_t)(i1 - i0 + 1) * W, DIR_STOP);
    std::vector<int32_t> H[2], E[2];
    for (int q = 0; q < 2; ++q) H[q].assign((size_t)W + 1, 0), E[q].assign((size_t)W + 1, NEG);
    int best = 0, ie = -1, je = -1;
    for (int i = i0; i <= i1; ++i) {
        std::vector<int32_t> &Hp = H[(i - i0) & 1], &Ep = E[(i - i0) & 1], &Hn = H[(i - i0 + 1) & 1], &En = E[(i - i0 + 1) & 1];
        const int rcode = code_at(R, i), jbase = i - d0 - w;
        int f = NEG;
        for (int b = 0; b < W; ++b) {
            const int j = jbase + b;
            if (j < 0 || j >= lq) {
                Hn[b] = 0, En[b] = NEG;
                continue;
            }
            const Cell c = dp_cell(p, Hp[b], Ep[b + 1], f, score_of(p, rcode, code_at(Q, j)));
            Hn[b] = c.h, En[b] = c.e, f = c.f;
            dir[(size_t)(i - i0) * W + b] = c.d;
            if (c.h > best) best = c.h, ie = i, je = j;
        }
        Hn[W] = 0, En[W] = NEG;
    }
    if (best <= 0) return out;
    int i = ie, j = je, state = 0, n = 0;
    auto push = [&](int op, int len) {
        if (n && (int)(cigar[n - 1] & 15) == op) cigar[n - 1] += (uint32_t)len << 4;
        else cigar[n++] = (uint32_t)len << 4 | (uint32_t)op;
    };
    if (lq - 1 - je > 0) push(OP_S, lq - 1 - je);
    while (i >= i0 && j >= 0) {
        const int b = j - (i - d0 - w);
        if (b < 0 || b >= W) break;
        const int op = tb_step(state, dir[(size_t)(i - i0) * W + b]);
        if (op < 0) break;
        push(op, 1);
        if (op != OP_I) --i;
        if (op != OP_D) --j;
    }
    if (j + 1 > 0) push(OP_S, j + 1);
    std::reverse(cigar, cigar + n);
    out.mapped = 1, out.pos = i + 1, out.score = best, out.n_cigar = n;
    return out;
}

// ---------------------------------------------------------------------------
// consensus

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
// stripped, query window [wb, we); taboo_len: InDelTabooLength, 0 for the InDelTaboo fraction
CC_HD Prep prep_trim(const pr_ccs_params &p, const AlnView &a, int ref_len, int cb, int ce, int wb, int we, int taboo_len) {
    Prep r = {0, 0, 0, 0, 0, 0, 0};
    const int orig = a.q.len;
    long rpos = a.pos;
    if (p.trim) {
        long mc = 0, dc = 0, ic = 0;
        const long taboo = taboo_len ? (long)taboo_len : (long)((double)orig * p.indel_taboo + 0.5);
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

CC_HD Prep prep_aln(const pr_ccs_params &p, const AlnView &a, int ref_len) {
    Prep r = {-1, 0, 0, 0, 0, 0, 0};
    const int orig = a.q.len;
    if (a.ncig <= 0) return r;
    long qsum = 0;
    for (int i = 0; i < a.ncig; ++i) {
        const int op = (int)(a.cig[i] & 15), n = (int)(a.cig[i] >> 4);
        if (n <= 0) return r;
        if (op == OP_S) {
            if (i != 0 && i != a.ncig - 1) return r;
            qsum += n;
        } else if (op == OP_M || op == OP_I) {
            qsum += n;
        } else if (op != OP_D) {
            return r;
        }
    }
    if (qsum != orig) return r;
    r.use = 0;
    if (!(orig > p.min_aln_length)) return r;   // Seq.pm:277
    int cb = 0, ce = a.ncig, wb = 0, we = orig;
    if ((a.cig[0] & 15) == OP_S) wb = (int)(a.cig[0] >> 4), cb = 1;
    if (ce > cb && (a.cig[ce - 1] & 15) == OP_S) we -= (int)(a.cig[ce - 1] >> 4), --ce;
    if (ce <= cb) {
        r.use = -1;
        return r;
    }
    return prep_trim(p, a, ref_len, cb, ce, wb, we, 0);
}

// min(Phreds2freqs(quals)) of the query bytes [qoff, qoff + n)
CC_HD double state_weight(const pr_ccs_params &p, const Read &q, int qoff, int n) {
    double m = 0.0;
    for (int t = 0; t < n; ++t) {
        const double f = phred2freq((int)qual_at(q, qoff + t) - p.phred_offset);
        if (t == 0 || f < m) m = f;
    }
    return m;
}
// Seq.pm:402-408: the lesser of the qualities around a deletion at window position qpos
CC_HD double del_weight(const pr_ccs_params &p, const Read &q, const Prep &pr, int qpos) {
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
// the columns op i fills; r its first column, q its window position
CC_HD void fill_op(const pr_ccs_params &p, const AlnView &a, const Prep &pr, int i, int r, int q, ColEnt *col) {
    const int op = (int)(a.cig[i] & 15), n = (int)(a.cig[i] >> 4);
    if (op == OP_I) {
        if (i != pr.cb) return;
        const int tot = n + ins_after(a, pr, i);   // a leading insertion is a state of its own column
        col[r] = ColEnt{pr.wb + q, tot, state_weight(p, a.q, pr.wb + q, tot)};
        return;
    }
    const int ins = ins_after(a, pr, i);
    if (op == OP_M) {
        for (int t = 0; t < n; ++t) {
            const int sl = t == n - 1 ? 1 + ins : 1;
            col[r + t] = ColEnt{pr.wb + q + t, sl, state_weight(p, a.q, pr.wb + q + t, sl)};
        }
        return;
    }
    const double wd = del_weight(p, a.q, pr, q);
    for (int t = 0; t < n; ++t) col[r + t] = ColEnt{pr.wb + q, 0, wd};
    if (ins) col[r + n - 1] = ColEnt{pr.wb + q, ins, state_weight(p, a.q, pr.wb + q, ins)};   // D+I: one replaced state
}
// first column / window position of the op after op i
CC_HD void advance_op(const AlnView &a, const Prep &pr, int i, int &r, int &q) {
    const int op = (int)(a.cig[i] & 15), n = (int)(a.cig[i] >> 4);
    if (op != OP_I) r += n;
    else if (i == pr.cb) r += 1;
    if (op != OP_D) q += n;
}

CC_HD bool same_state(const Read &x, int xo, const Read &y, int yo, int n) {
    for (int t = 0; t < n; ++t)
        if (base_at(x, xo + t) != base_at(y, yo + t)) return false;
    return true;
}
// global rank of an insertion state: its first occurrence in (alignment, column) order
CC_HD int64_t first_seen(const ColEnt *slab, int L, int m, const Read *reads, const Read &x, int xo, int n) {
    for (int a = 0; a < m; ++a)
        for (int c = 0; c < L; ++c) {
            const ColEnt &e = slab[(size_t)a * L + c];
            if (e.slen == n && same_state(reads[a], e.qoff, x, xo, n)) return (int64_t)a * L + c;
        }
    return -1;
}

// the consensus state of a column: kind 0 uncovered (the reference base), 1 a fixed state
// (idx; 4 is the gap), 2 the state of alignment a at this column
struct Choice {
    int32_t kind, idx, a;
    double f;
};
CC_HD Choice decide_col(const pr_ccs_params &p, const Read &ref, int c, const ColEnt *slab, int L, int m, const Read *reads) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0;
    auto add = [&](int idx, double w) {
        s0 += idx == 0 ? w : 0.0, s1 += idx == 1 ? w : 0.0, s2 += idx == 2 ? w : 0.0;
        s3 += idx == 3 ? w : 0.0, s4 += idx == 4 ? w : 0.0, s5 += idx == 5 ? w : 0.0;
    };
    const double fr = phred2freq((int)ref.qual[c] - p.phred_offset);
    if (fr != 0.0) add(fixed_idx(ref.seq[c]), fr);
    bool multi = false;
    for (int a = 0; a < m; ++a) {
        const ColEnt &e = slab[(size_t)a * L + c];
        if (e.slen == 0) add(4, e.w);
        else if (e.slen == 1) add(fixed_idx(base_at(reads[a], e.qoff)), e.w);
        else if (e.slen > 1) multi = true;
    }
    Choice ch = {0, 0, -1, 0.0};
    const double s[6] = {s0, s1, s2, s3, s4, s5};
    for (int i = 0; i < 6; ++i)
        if (s[i] > ch.f) ch.f = s[i], ch.kind = 1, ch.idx = i;
    if (!multi) return ch;
    for (int a = 0; a < m; ++a) {
        const ColEnt &e = slab[(size_t)a * L + c];
        if (e.slen <= 1) continue;
        bool seen = false;
        for (int b = 0; b < a && !seen; ++b) {
            const ColEnt &g = slab[(size_t)b * L + c];
            seen = g.slen == e.slen && same_state(reads[b], g.qoff, reads[a], e.qoff, e.slen);
        }
        if (seen) continue;
        double sum = 0.0;
        for (int b = a; b < m; ++b) {
            const ColEnt &g = slab[(size_t)b * L + c];
            if (g.slen == e.slen && same_state(reads[b], g.qoff, reads[a], e.qoff, e.slen)) sum += g.w;
        }
        if (sum > ch.f) {
            ch.f = sum, ch.kind = 2, ch.a = a;
        } else if (sum == ch.f && sum > 0.0 && ch.kind == 2) {
            // equal sums of two insertion states: the lower state index wins, the index is the
            // rank of the state's first occurrence anywhere in the read (Seq.pm:441-443)
            const ColEnt &g = slab[(size_t)ch.a * L + c];
            if (first_seen(slab, L, m, reads, reads[a], e.qoff, e.slen) <
                first_seen(slab, L, m, reads, reads[ch.a], g.qoff, g.slen))
                ch.a = a;
        }
    }
    return ch;
}
// bases and trace characters a column emits (Seq.pm:1620-1650)
CC_HD void choice_len(const Choice &ch, const ColEnt *slab, int L, int c, int &nseq, int &ntrace) {
    if (ch.kind == 1 && ch.idx == 4) nseq = 0, ntrace = 1;
    else if (ch.kind == 2) nseq = ntrace = slab[(size_t)ch.a * L + c].slen;
    else nseq = ntrace = 1;
}
CC_HD void choice_emit(const pr_ccs_params &p, const Choice &ch, const Read &ref, const ColEnt *slab, int L, int c,
                       const Read *reads, uint8_t *seq, uint8_t *qual, uint8_t *trace) {
    if (ch.kind == 1 && ch.idx == 4) {
        trace[0] = 'I';
        return;
    }
    const uint8_t ph = (uint8_t)(freq2phred(ch.f) + p.phred_offset);
    trace[0] = 'M';
    if (ch.kind == 2) {
        const ColEnt &e = slab[(size_t)ch.a * L + c];
        for (int t = 0; t < e.slen; ++t) {
            seq[t] = base_at(reads[ch.a], e.qoff + t), qual[t] = ph;
            if (t) trace[t] = 'D';
        }
    } else {
        seq[0] = ch.kind == 1 ? fixed_chr(ch.idx) : ref.seq[c];
        qual[0] = ph;
    }
}

}   // namespace ccs
}   // namespace prgpu

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
//   consensus  Sam::Seq State_matrix / state_matrix_consensus with Trim 1, InDelTaboo 0.001,
//              use_ref_qual, qual_weighted: the rules are sm_core.h's; here an alignment is
//              expanded into a column map (query offset, state length, weight per column, the
//              slab), which is the source of the vote
// The pieces marked CC_HD are the ones the kernels call.
#pragma once
#include <stdint.h>

#include "../../include/prgpu.h"
#include "sm_core.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace prgpu {
namespace ccs {

using namespace sm;

constexpr int NEG = -0x40000000;
enum { DIR_SRC = 3, DIR_EEXT = 4, DIR_FEXT = 8, DIR_STOP = 16 };

CC_HD int code_of(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }
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
// consensus: the State_matrix of sm_core.h over a slab of per-column entries

// ccseq's settings of Sam::Seq (ccseq:214-217): InDelTabooLength unset, MaxInsLength 0,
// use_ref_qual and qual_weighted, one phred offset
CC_HD Params sm_params(const pr_ccs_params &p) {
    Params s = {};
    s.trim = p.trim, s.min_aln_length = p.min_aln_length, s.phred_offset = s.ref_phred_offset = p.phred_offset;
    s.indel_taboo = p.indel_taboo, s.use_ref_qual = s.qual_weighted = 1;
    return s;
}

CC_HD Prep prep_aln(const Params &p, const AlnView &a, int ref_len) {
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
    return prep_trim(p, a, ref_len, cb, ce, wb, we);
}

// op i expanded into the columns it covers (a leading insertion one, M and D their length; an
// insertion behind another op is part of that op's last column); r its first column, q its
// window position
CC_HD void fill_op(const Params &p, const AlnView &a, const Prep &pr, int i, int r, int q, ColEnt *col) {
    const bool ins = (a.cig[i] & 15) == OP_I;
    if (ins && i != pr.cb) return;
    const int n = ins ? 1 : (int)(a.cig[i] >> 4);
    for (int t = 0; t < n; ++t) col[r + t] = entry_of_op(p, a, pr, i, r, q, r + t);
}

// the vote's source: alignment k's entries for the L columns at slab[k * L]
struct SlabSrc {
    const ColEnt *slab;
    int L, m;
    const Read *reads;
    CC_HD int count() const { return m; }
    CC_HD ColEnt entry(int k, int c) const { return slab[(size_t)k * L + c]; }
    CC_HD Read read(int k) const { return reads[k]; }
    CC_HD bool ignored(int) const { return false; }
    // the state's first occurrence among all entries in (alignment, column) order
    CC_HD int64_t first_seen(const Read &x, int xo, int n) const {
        for (int a = 0; a < m; ++a)
            for (int c = 0; c < L; ++c) {
                const ColEnt &e = slab[(size_t)a * L + c];
                if (e.slen == n && same_state(reads[a], e.qoff, x, xo, n)) return (int64_t)a * L + c;
            }
        return -1;
    }
};

// the host path of one group's consensus from the alignments in A; slab is the caller's scratch
inline void cns_group_host(const pr_ccs_params &cp, const pr_ccs_batch *b, int g, const pr_ccs_alns *A, pr_ccs_out *O,
                           std::vector<ColEnt> &slab) {
    const Params p = sm_params(cp);
    auto read_of = [&](int s, int rev) {
        return Read{b->seq + b->off[s], b->qual + b->off[s], (int32_t)(b->off[s + 1] - b->off[s]), rev};
    };
    const int r = b->grp_ref[g];
    const Read ref = read_of(r, 0);
    const int L = ref.len;
    std::vector<Read> reads;
    std::vector<Prep> preps;
    std::vector<AlnView> views;
    O->seq_len[g] = O->trace_len[g] = 0;
    for (int s = b->grp_off[g]; s < b->grp_off[g + 1]; ++s) {
        if (s == r || !A->mapped[s]) continue;
        const AlnView v = {read_of(s, A->strand[s] ? 1 : 0), A->pos[s], A->cigar + b->cig_off[s], A->n_cigar[s]};
        const Prep pr = v.ncig > b->cig_off[s + 1] - b->cig_off[s] ? Prep{-1, 0, 0, 0, 0, 0, 0} : prep_aln(p, v, L);
        if (pr.use < 0) {
            O->status[g] = PR_CCS_BAD_ALN;
            return;
        }
        if (pr.use == 1) reads.push_back(v.q), preps.push_back(pr), views.push_back(v);
    }
    const int m = (int)reads.size();
    slab.assign((size_t)m * L, ColEnt{-1, -1, 0.0});
    for (int a = 0; a < m; ++a) {
        int rr = preps[a].rpos, q = 0;
        for (int i = preps[a].cb; i < preps[a].ce; ++i) {
            fill_op(p, views[a], preps[a], i, rr, q, slab.data() + (size_t)a * L);
            advance_op(views[a], preps[a], i, rr, q);
        }
    }
    const SlabSrc src = {slab.data(), L, m, reads.data()};
    uint8_t *seq = O->seq + b->out_off[g], *qual = O->qual + b->out_off[g], *trace = O->trace + b->out_off[g];
    int ns = 0, nt = 0;
    for (int c = 0; c < L; ++c) {
        const Pick pk = decide_col(p, ref, c, src);
        int a = 0, t = 0;
        pick_len(pk, a, t);
        pick_emit(p, pk, ref, c, src, seq + ns, qual + ns, trace + nt);
        ns += a, nt += t;
    }
    O->seq_len[g] = ns, O->trace_len[g] = nt;
}

}   // namespace ccs
}   // namespace prgpu

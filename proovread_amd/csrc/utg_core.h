// The unitig consensus (bam2cns --utg-mode): the rules of the stage, shared by the host path
// (utg_api.cpp), the kernels (utg_kernels.hip) and the host tests.  HIP-free; DESIGN.md §14
// states the same rules in prose.
//
//   step 1  --min-ncscore      Seq.pm:919-927 with Alignment.pm:417-431, 525-546
//   step 2  --rep-coverage     filter_rep_region_alns, Seq.pm:949-999
//   step 3  contained hits     filter_contained_alns, Seq.pm:1001-1047
//   step 4  overlap windows    bam2cns:398-422
//   step 5  consensus          Seq.pm:232-467 (State_matrix), 1568-1654 (state_matrix_consensus)
//
// The map from (alignment, column) to a state is never stored: every CIGAR op keeps its first
// column and its first query position (op_r, op_q), a column finds its op by bisection and the
// state and its weight follow from the op (OpSrc).  Memory grows with the ops, not the spans.
// The trim, the states and the vote of step 5 are sm_core.h's; OpSrc is the vote's source here.
// The pieces marked CC_HD are the ones the kernels call.
#pragma once
#include <stdint.h>

#include "../../include/prgpu.h"
#include "sm_core.h"

#include <algorithm>
#include <vector>

namespace prgpu {
namespace utg {

using namespace sm;

// per alignment: alive after step 1, after step 2, after step 3; ncscore of a length 0
enum { F_ALIVE1 = 1, F_ALIVE2 = 2, F_KEPT = 4, F_DIV0 = 8 };
constexpr int FILTER_LDS = 2048;   // alignments of a read the contained filter sorts on chip

// the batch (quality pool with every '*' filled in), the outputs and the scratch of one call;
// every pointer is valid where the code runs
struct View {
    pr_utg_params p;
    Params sp;                // what sm_core.h's pieces read of p
    pr_utg_batch b;
    pr_utg_out o;
    const int32_t *aln_read;  // [n_alns] the read of an alignment
    Prep *prep;               // [n_alns]
    int32_t *alen;            // [n_alns] Sam::Alignment::length
    int32_t *span_e;          // [n_alns] one past the last column (prep.rpos is the first)
    double *sc;               // [n_alns] Sam::Alignment::score, 0 where undefined
    uint8_t *flag;            // [n_alns] F_*
    int32_t *op_r, *op_q;     // first column / window position of every CIGAR op
    int32_t *cov;             // read r: L + 1 entries at read_off[r] + r, difference array then coverage
    int32_t *ulist, *rlist;   // [n_alns] per read: the alignments of the consensus / of the state ranks
    int32_t *n_u, *n_r;       // [n_reads]
    int32_t *f_pos, *f_len, *f_id;   // [n_alns] the contained filter's queue when it outgrows the chip
    double *f_sc;
};

CC_HD Params sm_params(const pr_utg_params &p) {
    Params s = {};
    s.trim = p.trim, s.min_aln_length = p.min_aln_length, s.phred_offset = p.phred_offset, s.ref_phred_offset = p.ref_phred_offset;
    s.indel_taboo = p.indel_taboo, s.indel_taboo_length = p.indel_taboo_length;
    s.use_ref_qual = p.use_ref_qual, s.qual_weighted = p.qual_weighted, s.max_ins_length = p.max_ins_length;
    return s;
}
CC_HD double ddiv(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
CC_HD double dmul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}

CC_HD int read_len(const pr_utg_batch &b, int r) { return (int)(b.read_off[r + 1] - b.read_off[r]); }
CC_HD Read ref_of(const pr_utg_batch &b, int r) {
    return Read{b.ref_seq + b.read_off[r], b.ref_qual ? b.ref_qual + b.read_off[r] : nullptr, read_len(b, r), 0};
}
CC_HD AlnView view_of(const pr_utg_batch &b, int64_t a) {
    const Read q = {b.seq + b.seq_off[a], b.qual + b.seq_off[a], (int32_t)(b.seq_off[a + 1] - b.seq_off[a]), 0};
    return AlnView{q, b.pos[a] - 1, b.cigar + b.cig_off[a], (int32_t)(b.cig_off[a + 1] - b.cig_off[a])};
}

// Seq.pm:275-385: the length skip comes first, then the clips in the reference's order (S at
// either end, then H at either end, Seq.pm:290-310); what is left must be M, I and D
CC_HD Prep prep_utg(const View &V, const AlnView &a, int ref_len) {
    const Prep bad = {-1, 0, 0, 0, 0, 0, 0}, skip = {0, 0, 0, 0, 0, 0, 0};
    const int orig = a.q.len;
    if (!(orig > V.p.min_aln_length)) return skip;   // Seq.pm:277
    auto op = [&](int i) { return (int)(a.cig[i] & 15); };
    auto len = [&](int i) { return (long)(a.cig[i] >> 4); };
    int cb = 0, ce = a.ncig;
    long wb = 0, we = orig;
    if (ce > cb && op(cb) == OP_S) wb = len(cb), ++cb;
    if (ce > cb && op(ce - 1) == OP_S) we -= len(ce - 1), --ce;
    if (ce > cb && op(cb) == OP_H) ++cb;
    if (ce > cb && op(ce - 1) == OP_H) --ce;
    if (ce <= cb) return bad;   // "Empty Cigar"
    for (int i = 0; i < a.ncig; ++i)
        if (len(i) <= 0) return bad;
    long qsum = 0;
    for (int i = cb; i < ce; ++i) {
        if (op(i) == OP_M || op(i) == OP_I) qsum += len(i);
        else if (op(i) != OP_D) return bad;   // "Unknown Cigar"
    }
    if (we < wb || qsum != we - wb) return bad;
    return prep_trim(V.sp, a, ref_len, cb, ce, (int)wb, (int)we);
}

// Alignment.pm:417-431
CC_HD long aln_length(const AlnView &a) {
    const bool clipped = a.ncig > 0 && ((a.cig[0] & 15) == OP_S || (a.cig[a.ncig - 1] & 15) == OP_S);
    if (!clipped) return a.q.len;
    long l = 0;
    for (int i = 0; i < a.ncig; ++i)
        if ((a.cig[i] & 15) == OP_M || (a.cig[i] & 15) == OP_D) l += (long)(a.cig[i] >> 4);
    return l;
}

// everything a thread per alignment does: the trim, the op prefixes, length, score and step 1
CC_HD void prep_one(const View &V, int64_t a, int ref_len) {
    const AlnView v = view_of(V.b, a);
    const Prep pr = prep_utg(V, v, ref_len);
    V.prep[a] = pr;
    int r = pr.rpos, q = 0;
    if (pr.use == 1)
        for (int i = pr.cb; i < pr.ce; ++i) {
            V.op_r[V.b.cig_off[a] + i] = r, V.op_q[V.b.cig_off[a] + i] = q;
            advance_op(v, pr, i, r, q);
        }
    V.span_e[a] = r;
    const long len = aln_length(v);
    V.alen[a] = (int32_t)len;
    // Alignment.pm:525-546; an undefined score compares as 0 in Seq.pm:1036
    const bool has = V.b.has_score[a] != 0;
    const double sc = has ? (V.p.invert_scores ? dmul(V.b.score[a], -1.0) : V.b.score[a]) : 0.0;
    V.sc[a] = sc;
    int f = F_ALIVE1;
    if (V.p.has_min_ncscore) {   // Seq.pm:919-927
        if (!has) f = 0;
        else if (len == 0) f = F_DIV0;
        else if (dmul(ddiv(sc, (double)len), ddiv((double)len, (double)(40 + len))) < V.p.min_ncscore) f = 0;
    }
    V.flag[a] = (uint8_t)f;
}

// Seq.pm:977-991 on the runs of step 4: every run widened by -150 / +300, the first clamped at
// 0, the last shortened by 1 when it overhangs (Seq.pm:989 assigns the comparison's result)
struct Win {
    long s, l;
};
CC_HD Win rwin_of(const int32_t *win, int k, int nw, int L) {
    Win w = {(long)win[2 * k] - 150, (long)win[2 * k + 1] + 300};
    if (k == 0 && w.s < 0) w.l += w.s, w.s = 0;
    if (k == nw - 1 && L - (w.s + w.l) < 0) w.l -= 1;
    return w;
}
// Seq.pm:996: [POS, length] inside one window; POS stays 1-based
CC_HD bool in_rwins(const int32_t *win, int nw, int L, long pos, long len) {
    const long c1 = pos, c2 = pos + len - 1;
    for (int k = 0; k < nw; ++k) {
        const Win w = rwin_of(win, k, nw, L);
        if (c1 >= w.s && c1 < w.s + w.l && c2 >= w.s && c2 < w.s + w.l) return true;
    }
    return false;
}

// Seq.pm:1017-1046 over the queue sorted by length, descending: fp / fl the coordinates, fs the
// scores (never popped: indexed by the sorted position), fi the ids.  in_range(pos, len, n)
// tests the popped range against the n remaining ones, remove(id) drops an alignment.
template <class InRange, class Remove>
CC_HD void contained_pop(int n, int32_t *fp, int32_t *fl, const double *fs, int32_t *fi, InRange in_range, Remove remove) {
    while (n > 1) {
        int iid = fi[n - 1];
        long cp = fp[n - 1], cl = fl[n - 1];
        --n;
        if (cl < 21) {   // very short hits; the elsif of Seq.pm:1023 cannot be reached
            cp += cl / 2, cl = 1;
        } else {
            const long ad = (long)dmul((double)cl, 0.1);
            cp += ad, cl -= 2 * ad;
        }
        if (in_range(cp, cl, n)) {
            if (cl > (long)fl[n - 1] - 40 && fs[n] > fs[n - 1]) {   // almost identical length: by score
                const int restore = iid;
                iid = fi[n - 1];
                fi[n - 1] = restore, fp[n - 1] = (int32_t)cp, fl[n - 1] = (int32_t)cl;
            }
            remove(iid);
        }
    }
}
CC_HD bool range_inside(long cp, long cl, long rp, long rl) {
    const long c2 = cp + cl - 1;
    return cp >= rp && cp < rp + rl && c2 >= rp && c2 < rp + rl;
}

// the ignored columns of the consensus: the MCR ranges, then the overlap windows (bam2cns:436)
CC_HD bool ignored(const View &V, int r, int c) {
    for (int64_t k = V.b.ign_off[r]; k < V.b.ign_off[r + 1]; ++k)
        if (c >= V.b.ign[2 * k] && (long)c < (long)V.b.ign[2 * k] + V.b.ign[2 * k + 1]) return true;
    const int32_t *w = V.o.win + 2 * V.b.win_off[r];
    for (int k = 0; k < V.o.n_win[r]; ++k)
        if (c >= w[2 * k] && c < w[2 * k] + w[2 * k + 1]) return true;
    return false;
}

// the op of column c: the last one that starts at or before it (an insertion behind another op
// starts where the next op does and is never the last)
CC_HD int op_of_col(const Prep &pr, const int32_t *opr, int c) {
    int lo = pr.cb, hi = pr.ce;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (opr[mid] <= c) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// the vote's source: the alignments lst[0, m) of read r in arrival order; a column finds its op
// in each by bisection, an alignment that does not span the column has no state there
struct OpSrc {
    const View &V;
    int r;
    const int32_t *lst;
    int m;
    CC_HD int count() const { return m; }
    CC_HD Read read(int k) const { return view_of(V.b, lst[k]).q; }
    CC_HD bool ignored(int c) const { return utg::ignored(V, r, c); }
    CC_HD ColEnt entry(int k, int c) const {
        const int64_t a = lst[k];
        if (c < V.prep[a].rpos || c >= V.span_e[a]) return ColEnt{0, -1, 0.0};
        const int32_t *opr = V.op_r + V.b.cig_off[a], *opq = V.op_q + V.b.cig_off[a];
        const int i = op_of_col(V.prep[a], opr, c);
        return entry_of_op(V.sp, view_of(V.b, a), V.prep[a], i, opr[i], opq[i], c);
    }
    // Seq.pm:446-448: the state's first occurrence over the alignments of rlist (step 2's matrix
    // when it ran, which had no ignored columns) in (alignment, column) order
    CC_HD int64_t first_seen(const Read &x, int xo, int n) const {
        const int32_t *rlist = V.rlist + V.b.aln_off[r];
        const bool ign = !V.p.has_rep_coverage;
        for (int k = 0; k < V.n_r[r]; ++k) {
            const int64_t a = rlist[k];
            const AlnView v = view_of(V.b, a);
            const Prep pr = V.prep[a];
            const int32_t *opr = V.op_r + V.b.cig_off[a], *opq = V.op_q + V.b.cig_off[a];
            for (int i = pr.cb; i < pr.ce; ++i) {
                const int op = (int)(v.cig[i] & 15);
                if (op == OP_I && i != pr.cb) continue;
                const int c = op == OP_I ? opr[i] : opr[i] + (int)(v.cig[i] >> 4) - 1;
                const ColEnt e = state_of_op(v, pr, i, opr[i], opq[i], c);
                if (e.slen != n || !same_state(v.q, e.qoff, x, xo, n)) continue;
                if (ign && utg::ignored(V, r, c)) continue;
                return (int64_t)k << 32 | (int64_t)c;
            }
        }
        return INT64_MAX;
    }
};

// which alignments a State_matrix pass parses: those of the ranks (step 2's matrix when it ran)
// and those of the consensus; a malformed one among them is the read's PR_UTG_BAD_ALN
CC_HD bool in_rank_pass(const View &V, int64_t a) { return V.p.has_rep_coverage ? (V.flag[a] & F_ALIVE1) != 0 : (V.flag[a] & F_KEPT) != 0; }

// ---------------------------------------------------------------------------
// the host path of one read (bam2cns:375-455); V's scratch is sized for the batch
inline void run_read_host(const View &V, int r) {
    const pr_utg_batch &b = V.b;
    const int L = read_len(b, r);
    const int64_t a0 = b.aln_off[r], a1 = b.aln_off[r + 1];
    const int na = (int)(a1 - a0);
    int32_t *win = V.o.win + 2 * b.win_off[r];
    V.o.n_win[r] = 0, V.o.seq_len[r] = 0, V.o.trace_len[r] = 0;
    bool bad = false;
    for (int64_t a = a0; a < a1; ++a) {
        prep_one(V, a, L);
        bad |= (V.flag[a] & F_DIV0) != 0;
    }
    if (V.p.has_rep_coverage && !bad) {
        // step 2 and step 4: the coverage of the unweighted matrix over the alignments alive now
        int32_t *cov = V.cov + b.read_off[r] + r;
        std::fill(cov, cov + L + 1, 0);
        for (int64_t a = a0; a < a1; ++a)
            if (V.flag[a] & F_ALIVE1) {
                bad |= V.prep[a].use < 0;
                if (V.prep[a].use == 1) ++cov[V.prep[a].rpos], --cov[V.span_e[a]];
            }
        int nw = 0, run = 0;
        bool high = false;
        for (int c = 0; c < L && !bad; ++c) {
            run += cov[c];
            const bool h = !(run < V.p.rep_coverage);
            if (h && !high) win[2 * nw] = c;
            if (!h && high) win[2 * nw + 1] = c - win[2 * nw], ++nw;
            high = h;
        }
        if (high) win[2 * nw + 1] = L - win[2 * nw], ++nw;
        V.o.n_win[r] = bad ? 0 : nw;
        for (int64_t a = a0; a < a1 && !bad; ++a)
            if ((V.flag[a] & F_ALIVE1) && !(nw && in_rwins(win, nw, L, b.pos[a], V.alen[a]))) V.flag[a] |= F_ALIVE2;
    } else {
        // without step 2 no matrix exists when bam2cns:403 asks for the coverage: no windows
        for (int64_t a = a0; a < a1; ++a)
            if (V.flag[a] & F_ALIVE1) V.flag[a] |= F_ALIVE2;
    }
    if (!bad) {
        // step 3: ties in length go in arrival order
        std::vector<int32_t> ord;
        for (int k = 0; k < na; ++k)
            if (V.flag[a0 + k] & F_ALIVE2) ord.push_back(k), V.flag[a0 + k] |= F_KEPT;
        std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return V.alen[a0 + x] > V.alen[a0 + y]; });
        const int n = (int)ord.size();
        std::vector<int32_t> fp((size_t)n + 1), fl((size_t)n + 1), fi((size_t)n + 1);
        std::vector<double> fs((size_t)n + 1);
        for (int k = 0; k < n; ++k) fp[k] = b.pos[a0 + ord[k]], fl[k] = V.alen[a0 + ord[k]], fs[k] = V.sc[a0 + ord[k]], fi[k] = ord[k];
        contained_pop(
            n, fp.data(), fl.data(), fs.data(), fi.data(),
            [&](long cp, long cl, int m) {
                for (int k = 0; k < m; ++k)
                    if (range_inside(cp, cl, fp[k], fl[k])) return true;
                return false;
            },
            [&](int id) { V.flag[a0 + id] &= (uint8_t)~F_KEPT; });
    }
    int nu = 0, nr = 0;
    for (int64_t a = a0; a < a1 && !bad; ++a) {
        const bool kept = (V.flag[a] & F_KEPT) != 0;
        V.o.kept[a] = kept;
        if (kept) bad |= V.prep[a].use < 0;
        if (kept && V.prep[a].use == 1) V.ulist[a0 + nu++] = (int32_t)a;
        if (in_rank_pass(V, a) && V.prep[a].use == 1) V.rlist[a0 + nr++] = (int32_t)a;
    }
    V.n_u[r] = nu, V.n_r[r] = nr;
    if (bad) {
        for (int64_t a = a0; a < a1; ++a) V.o.kept[a] = 0;
        V.o.status[r] = PR_UTG_BAD_ALN, V.o.n_win[r] = 0;
        return;
    }
    const Read ref = ref_of(b, r);
    uint8_t *seq = V.o.seq + b.out_off[r], *qual = V.o.qual + b.out_off[r], *trace = V.o.trace + b.out_off[r];
    // the alignments are few against the columns: those that span a column, by a sweep
    std::vector<int32_t> live;
    int next = 0, ns = 0, nt = 0;
    std::vector<int32_t> byStart(V.ulist + a0, V.ulist + a0 + nu);
    std::stable_sort(byStart.begin(), byStart.end(), [&](int32_t x, int32_t y) { return V.prep[x].rpos < V.prep[y].rpos; });
    for (int c = 0; c < L; ++c) {
        bool changed = false;
        while (next < nu && V.prep[byStart[next]].rpos <= c) live.push_back(byStart[next++]), changed = true;
        const size_t before = live.size();
        live.erase(std::remove_if(live.begin(), live.end(), [&](int32_t a) { return V.span_e[a] <= c; }), live.end());
        if (changed || before != live.size()) std::sort(live.begin(), live.end());   // arrival order
        const OpSrc src = {V, r, live.data(), (int)live.size()};
        const Pick pk = decide_col(V.sp, ref, c, src);
        int a = 0, t = 0;
        pick_len(pk, a, t);
        pick_emit(V.sp, pk, ref, c, src, seq + ns, qual + ns, trace + nt);
        ns += a, nt += t;
    }
    V.o.seq_len[r] = ns, V.o.trace_len[r] = nt;
}

}   // namespace utg
}   // namespace prgpu

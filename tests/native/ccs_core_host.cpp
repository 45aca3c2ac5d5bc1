// Stand-alone host program over csrc/ccs_core.h (no HIP, no library): reads one group from a
// text file and prints its alignments and consensus as the host path of pr_ccs_run computes
// them (ccs::cns_group_host).  It also holds the two sources of the State_matrix vote against
// each other: every entry of the slab against the same state found by bisection over the ops
// (utg::op_of_col + sm::entry_of_op), and the vote over either source.
// tests/test_ccs_core_host.py builds it with AddressSanitizer and UBSan and compares the output
// with the library's.
//
//   line 1: k w ref_index [trim]
//   then one line per subread: "SEQ QUAL" (the program maps it) or "SEQ QUAL strand pos CIGAR"
//   (the alignment is given; SEQ and QUAL as sequenced)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../proovread_amd/csrc/ccs_core.h"
#include "../../proovread_amd/csrc/utg_core.h"

using namespace prgpu::ccs;

namespace {

// the states of the group's alignments by bisection; ranks over the same domain as the slab's
struct BisectSrc {
    const Params &p;
    int L;
    const std::vector<AlnView> &views;
    const std::vector<Prep> &preps;
    std::vector<std::vector<int32_t>> op_r, op_q;
    std::vector<int32_t> span_e;
    BisectSrc(const Params &p_, int L_, const std::vector<AlnView> &v, const std::vector<Prep> &pr) : p(p_), L(L_), views(v), preps(pr) {
        for (size_t a = 0; a < v.size(); ++a) {
            op_r.emplace_back((size_t)v[a].ncig), op_q.emplace_back((size_t)v[a].ncig);
            int r = pr[a].rpos, q = 0;
            for (int i = pr[a].cb; i < pr[a].ce; ++i) {
                op_r[a][i] = r, op_q[a][i] = q;
                advance_op(v[a], pr[a], i, r, q);
            }
            span_e.push_back(r);
        }
    }
    int count() const { return (int)views.size(); }
    Read read(int k) const { return views[k].q; }
    bool ignored(int) const { return false; }
    ColEnt entry(int k, int c) const {
        if (c < preps[k].rpos || c >= span_e[k]) return ColEnt{-1, -1, 0.0};
        const int i = prgpu::utg::op_of_col(preps[k], op_r[k].data(), c);
        return entry_of_op(p, views[k], preps[k], i, op_r[k][i], op_q[k][i], c);
    }
    int64_t first_seen(const Read &x, int xo, int n) const {
        for (int a = 0; a < count(); ++a)
            for (int c = 0; c < L; ++c) {
                const ColEnt e = entry(a, c);
                if (e.slen == n && same_state(views[a].q, e.qoff, x, xo, n)) return (int64_t)a * L + c;
            }
        return -1;
    }
};

bool same_bits(double x, double y) { return std::memcmp(&x, &y, sizeof x) == 0; }

// 0, or 4 with the first (alignment, column) at which the two sources differ
int check_sources(const Params &p, const Read &R, const std::vector<AlnView> &views, const std::vector<Prep> &preps,
                  const std::vector<Read> &reads, const std::vector<ColEnt> &slab) {
    const int L = R.len, m = (int)views.size();
    const BisectSrc bis(p, L, views, preps);
    const SlabSrc src = {slab.data(), L, m, reads.data()};
    for (int a = 0; a < m; ++a)
        for (int c = 0; c < L; ++c) {
            const ColEnt e = bis.entry(a, c), s = src.entry(a, c);
            if (e.qoff != s.qoff || e.slen != s.slen || !same_bits(e.w, s.w)) {
                std::fprintf(stderr, "entry differs: alignment %d column %d\n", a, c);
                return 4;
            }
        }
    for (int c = 0; c < L; ++c) {
        const Pick x = decide_col(p, R, c, bis), y = decide_col(p, R, c, src);
        if (x.kind != y.kind || x.idx != y.idx || x.k != y.k || !same_bits(x.f, y.f) || x.qoff != y.qoff || x.slen != y.slen) {
            std::fprintf(stderr, "vote differs: alignment %d column %d\n", y.k, c);
            return 4;
        }
    }
    return 0;
}

}   // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    pr_ccs_params p = {9, 300, 5, 11, 2, 1, 4, 3, 1, 50, 33, 0, 0.001};
    int ref = 0;
    std::string line;
    std::getline(in, line);
    std::istringstream head(line);
    head >> p.k >> p.w >> ref;
    if (int trim; head >> trim) p.trim = trim;
    std::vector<std::string> seq, qual, given;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string s, q, rest;
        if (!(ls >> s >> q)) continue;
        std::getline(ls, rest);
        seq.push_back(s), qual.push_back(q), given.push_back(rest);
    }
    const int n = (int)seq.size();
    if (ref < 0 || ref >= n) return 2;
    // the group as a batch of one; exact sizes, so the sanitizer sees an index past an array's end
    const int L = (int)seq[ref].size();
    std::string bases, quals;
    std::vector<int64_t> off(1, 0), cig_off(1, 0);
    for (int s = 0; s < n; ++s) {
        bases += seq[s], quals += qual[s];
        off.push_back((int64_t)bases.size());
        cig_off.push_back(cig_off.back() + (int64_t)seq[s].size() + L + 2);
    }
    const int32_t grp_off[2] = {0, n}, grp_ref[1] = {ref};
    const int64_t out_off[2] = {0, (int64_t)bases.size()};
    const pr_ccs_batch b = {1, n, grp_off, grp_ref, off.data(), (const uint8_t *)bases.data(), (const uint8_t *)quals.data(), cig_off.data(), out_off};
    std::vector<int32_t> mapped((size_t)n, 0), strand((size_t)n, 0), pos((size_t)n, 0), score((size_t)n, 0), n_cigar((size_t)n, 0);
    std::vector<uint32_t> cigar((size_t)cig_off[n], 0);
    const pr_ccs_alns A = {mapped.data(), strand.data(), pos.data(), score.data(), n_cigar.data(), cigar.data()};
    auto read_of = [&](int s, int rev) {
        return Read{b.seq + off[s], b.qual + off[s], (int32_t)seq[s].size(), rev};
    };
    const Read R = read_of(ref, 0);
    std::vector<uint8_t> dir;
    for (int s = 0; s < n; ++s) {
        if (s == ref) continue;
        uint32_t *cig = cigar.data() + cig_off[s];
        std::istringstream gs(given[s]);
        std::string text;
        if (gs >> strand[s] >> pos[s] >> text) {
            uint32_t len = 0;
            for (char ch : text) {
                if (ch >= '0' && ch <= '9') len = len * 10 + (uint32_t)(ch - '0');
                else cig[n_cigar[s]++] = len << 4 | (uint32_t)(std::strchr("MIDNS", ch) - "MIDNS"), len = 0;
            }
            mapped[s] = 1;
        } else {
            const Centre c = centre_host(p, R, read_of(s, 0));
            if (c.found) {
                const Aln a = align_host(p, R, read_of(s, c.rev), c.d0, dir, cig);
                mapped[s] = a.mapped, strand[s] = a.mapped ? a.strand : 0, pos[s] = a.pos, score[s] = a.score, n_cigar[s] = a.n_cigar;
            }
        }
        std::printf("aln %d %d %d %d ", mapped[s], strand[s], pos[s], score[s]);
        for (int k = 0; k < n_cigar[s]; ++k) std::printf("%u%c", cig[k] >> 4, "MIDNS"[cig[k] & 15]);
        std::printf("\n");
    }
    int32_t status = 0, seq_len = 0, trace_len = 0;
    std::string oseq(bases.size(), ' '), oqual(bases.size(), ' '), otrace(bases.size(), ' ');
    pr_ccs_out O = {&status, &seq_len, &trace_len, (uint8_t *)&oseq[0], (uint8_t *)&oqual[0], (uint8_t *)&otrace[0]};
    std::vector<ColEnt> slab;
    cns_group_host(p, &b, 0, &A, &O, slab);
    if (status) return 3;
    // the alignments behind the slab's rows, as cns_group_host lists them
    const Params sp = sm_params(p);
    std::vector<Read> reads;
    std::vector<Prep> preps;
    std::vector<AlnView> views;
    for (int s = 0; s < n; ++s) {
        if (s == ref || !mapped[s]) continue;
        const AlnView v = {read_of(s, strand[s]), pos[s], cigar.data() + cig_off[s], n_cigar[s]};
        const Prep pr = prep_aln(sp, v, L);
        if (pr.use == 1) reads.push_back(v.q), preps.push_back(pr), views.push_back(v);
    }
    if (slab.size() != views.size() * (size_t)L) return 4;
    if (const int rc = check_sources(sp, R, views, preps, reads, slab)) return rc;
    std::printf("seq %s\nqual %s\ntrace %s\n", oseq.substr(0, seq_len).c_str(), oqual.substr(0, seq_len).c_str(), otrace.substr(0, trace_len).c_str());
    // the grouping on the ids of a small input
    const char ids[] = "m1/1/0_9m1/1/20_40m1/2/0_5";
    const int64_t id_off[] = {0, 8, 18, 26};
    const int32_t len[] = {9, 20, 5};
    int32_t role[3], grp[3], kind, idx;
    const int ng = group_ids(3, ids, id_off, len, role, grp, &kind, &idx);
    std::printf("groups %d roles %d %d %d\n", ng, role[0], role[1], role[2]);
    return 0;
}

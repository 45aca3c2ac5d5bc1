// Stand-alone host program over csrc/ccs_core.h (no HIP, no library): reads one group from a
// text file and prints its alignments and consensus as the host path of pr_ccs_run computes
// them.  tests/test_ccs_core_host.py builds it with AddressSanitizer and UBSan and compares the
// output with the library's.
//
//   line 1: k w ref_index       then one "SEQ QUAL" line per subread
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

#include "../../proovread_amd/csrc/ccs_core.h"

using namespace prgpu::ccs;

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    pr_ccs_params p = {9, 300, 5, 11, 2, 1, 4, 3, 1, 50, 33, 0, 0.001};
    int ref = 0;
    in >> p.k >> p.w >> ref;
    std::vector<std::string> seq, qual;
    for (std::string s, q; in >> s >> q;) seq.push_back(s), qual.push_back(q);
    const int n = (int)seq.size();
    if (ref < 0 || ref >= n) return 2;
    auto read_of = [&](int s, int rev) {
        return Read{(const uint8_t *)seq[s].data(), (const uint8_t *)qual[s].data(), (int32_t)seq[s].size(), rev};
    };
    const Read R = read_of(ref, 0);
    const int L = R.len;
    std::vector<std::vector<uint32_t>> cig((size_t)n);
    std::vector<Aln> alns((size_t)n, Aln{0, 0, 0, 0, 0});
    std::vector<uint8_t> dir;
    for (int s = 0; s < n; ++s) {
        if (s == ref) continue;
        cig[s].assign(seq[s].size() + (size_t)L + 2, 0);
        const Centre c = centre_host(p, R, read_of(s, 0));
        if (c.found) alns[s] = align_host(p, R, read_of(s, c.rev), c.d0, dir, cig[s].data());
        std::printf("aln %d %d %d %d ", alns[s].mapped, alns[s].mapped ? alns[s].strand : 0, alns[s].pos, alns[s].score);
        for (int k = 0; k < alns[s].n_cigar; ++k) std::printf("%u%c", cig[s][k] >> 4, "MIDNS"[cig[s][k] & 15]);
        std::printf("\n");
    }
    std::vector<Read> reads;
    std::vector<Prep> preps;
    std::vector<AlnView> views;
    for (int s = 0; s < n; ++s) {
        if (s == ref || !alns[s].mapped) continue;
        const AlnView v = {read_of(s, alns[s].strand), alns[s].pos, cig[s].data(), alns[s].n_cigar};
        const Prep pr = prep_aln(p, v, L);
        if (pr.use < 0) return 3;
        if (pr.use == 1) reads.push_back(v.q), preps.push_back(pr), views.push_back(v);
    }
    const int m = (int)reads.size();
    std::vector<ColEnt> slab((size_t)m * L, ColEnt{-1, -1, 0.0});
    for (int a = 0; a < m; ++a) {
        int rr = preps[a].rpos, q = 0;
        for (int i = preps[a].cb; i < preps[a].ce; ++i) {
            fill_op(p, views[a], preps[a], i, rr, q, slab.data() + (size_t)a * L);
            advance_op(views[a], preps[a], i, rr, q);
        }
    }
    size_t total = (size_t)L;
    for (const auto &s : seq) total += s.size();
    std::string oseq(total, ' '), oqual(total, ' '), otrace(total, ' ');
    int ns = 0, nt = 0;
    for (int c = 0; c < L; ++c) {
        const Choice ch = decide_col(p, R, c, slab.data(), L, m, reads.data());
        int a = 0, t = 0;
        choice_len(ch, slab.data(), L, c, a, t);
        choice_emit(p, ch, R, slab.data(), L, c, reads.data(), (uint8_t *)&oseq[ns], (uint8_t *)&oqual[ns], (uint8_t *)&otrace[nt]);
        ns += a, nt += t;
    }
    std::printf("seq %s\nqual %s\ntrace %s\n", oseq.substr(0, ns).c_str(), oqual.substr(0, ns).c_str(), otrace.substr(0, nt).c_str());
    // the grouping on the ids of a small input
    const char ids[] = "m1/1/0_9m1/1/20_40m1/2/0_5";
    const int64_t off[] = {0, 8, 18, 26};
    const int32_t len[] = {9, 20, 5};
    int32_t role[3], grp[3], kind, idx;
    const int ng = group_ids(3, ids, off, len, role, grp, &kind, &idx);
    std::printf("groups %d roles %d %d %d\n", ng, role[0], role[1], role[2]);
    return 0;
}

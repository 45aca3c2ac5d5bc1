// Stand-alone host program over csrc/utg_core.h (no HIP, no library): reads the cases of a
// file in the format tests/utg_cases.py describes, runs the host path of one read at a time
// (utg::run_read_host) and prints the records of tests/golden/utg_expected.txt.
// tests/test_utg_host.py builds it with AddressSanitizer and UBSan and compares the output with
// the golden file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../proovread_amd/csrc/utg_core.h"

using namespace prgpu::utg;

namespace {

struct Case {
    std::string name, flags, cfg;
    std::vector<std::string> ref, sam;
};

std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> out;
    std::string cur;
    for (char c : s) {
        if (c == sep) out.push_back(cur), cur.clear();
        else cur += c;
    }
    out.push_back(cur);
    return out;
}

void run_case(const Case &c) {
    pr_utg_params p = {1, 7, 50, 33, 33, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0.1, 0.0};
    bool ignore_hcr = false;
    std::istringstream fs(c.flags);
    for (std::string k; fs >> k;) {
        if (k == "--qual-weighted") p.qual_weighted = 1;
        else if (k == "--no-use-ref-qual") p.use_ref_qual = 0;
        else if (k == "--invert-scores") p.invert_scores = 1;
        else if (k == "--ignore-hcr") ignore_hcr = true;
        else if (k == "--rep-coverage") fs >> p.rep_coverage, p.has_rep_coverage = 1;
        else if (k == "--min-ncscore") fs >> p.min_ncscore, p.has_min_ncscore = 1;
        else if (k == "--fallback-phred") fs >> p.fallback_phred;
        else if (k == "--max-ins-length") fs >> p.max_ins_length;
        else if (k == "--coverage") fs >> k;
    }
    std::istringstream cs(c.cfg);
    for (std::string kv; cs >> kv;) {
        const size_t eq = kv.find('=');
        const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
        if (k == "sr-trim") p.trim = std::atoi(v.c_str());
        else if (k == "sr-indel-taboo-length") p.indel_taboo_length = std::atoi(v.c_str());
        else if (k == "sr-indel-taboo") p.indel_taboo = std::atof(v.c_str());
    }
    const bool fasta = c.ref[0][0] == '>';
    if (fasta) p.use_ref_qual = 0, ignore_hcr = true;
    const std::string head = c.ref[0].substr(1), rid = head.substr(0, head.find(' '));
    const std::string rseq = c.ref[1];
    std::vector<int32_t> ign;
    if (!ignore_hcr)
        for (size_t at = head.find("MCR"); at != std::string::npos; at = head.find("MCR", at + 3)) {
            size_t q = at + 3;
            while (q < head.size() && isdigit((unsigned char)head[q])) ++q;
            int o = 0, l = 0;
            if (q > at + 3 && std::sscanf(head.c_str() + q, ":%d,%d", &o, &l) == 2) ign.push_back(o), ign.push_back(l);
        }
    const int64_t na = (int64_t)c.sam.size();
    std::vector<std::string> names;
    std::vector<int32_t> pos;
    std::vector<double> score;
    std::vector<uint8_t> has_score, seq, qual;
    std::vector<int64_t> seq_off(1, 0), cig_off(1, 0);
    std::vector<uint32_t> cigar;
    for (const std::string &line : c.sam) {
        const std::vector<std::string> f = split(line, '\t');
        names.push_back(f[0]);
        pos.push_back(std::atoi(f[3].c_str()));
        uint32_t n = 0;
        for (char ch : f[5]) {
            if (isdigit((unsigned char)ch)) n = n * 10 + (uint32_t)(ch - '0');
            else {
                const char *ops = "MIDNSHP=X", *at = std::strchr(ops, ch);
                cigar.push_back(n << 4 | (uint32_t)(at ? at - ops : 15));
                n = 0;
            }
        }
        cig_off.push_back((int64_t)cigar.size());
        const bool star = f[10] == "*";
        for (size_t i = 0; i < f[9].size(); ++i) {
            seq.push_back((uint8_t)f[9][i]);
            qual.push_back(star ? (uint8_t)(p.fallback_phred + p.phred_offset) : (uint8_t)f[10][i]);
        }
        seq_off.push_back((int64_t)seq.size());
        double sc = 0;
        bool has = false;
        for (size_t i = 11; i < f.size(); ++i)
            if (f[i].compare(0, 5, "AS:i:") == 0) sc = std::atof(f[i].c_str() + 5), has = true;
        score.push_back(sc), has_score.push_back(has);
    }
    // exact sizes: the sanitizer sees every index past an array's end
    const int L = (int)rseq.size();
    const int64_t read_off[2] = {0, L}, aln_off[2] = {0, na}, ign_off[2] = {0, (int64_t)ign.size() / 2};
    const int64_t out_off[2] = {0, L + (int64_t)seq.size()}, win_off[2] = {0, std::max<int64_t>(na, 1)};
    std::vector<uint8_t> oseq((size_t)out_off[1]), oqual((size_t)out_off[1]), otrace((size_t)out_off[1]), kept((size_t)na);
    std::vector<int32_t> win((size_t)(2 * win_off[1]));
    int32_t status = 0, seq_len = 0, trace_len = 0, n_win = 0, n_u = 0, n_r = 0;
    std::vector<Prep> prep((size_t)na);
    std::vector<int32_t> alen((size_t)na), span_e((size_t)na), op_r(cigar.size()), op_q(cigar.size()), cov((size_t)L + 1), ulist((size_t)na),
        rlist((size_t)na);
    std::vector<double> sc((size_t)na);
    std::vector<uint8_t> flag((size_t)na);
    View V = {};
    V.p = p, V.sp = sm_params(p);
    V.b.n_reads = 1, V.b.n_alns = na, V.b.read_off = read_off, V.b.ref_seq = (const uint8_t *)rseq.data();
    V.b.ref_qual = fasta ? nullptr : (const uint8_t *)c.ref[3].data();
    V.b.aln_off = aln_off, V.b.pos = pos.data(), V.b.score = score.data(), V.b.has_score = has_score.data();
    V.b.seq_off = seq_off.data(), V.b.seq = seq.data(), V.b.qual = qual.data(), V.b.cig_off = cig_off.data(), V.b.cigar = cigar.data();
    V.b.ign_off = ign_off, V.b.ign = ign.data(), V.b.out_off = out_off, V.b.win_off = win_off;
    V.o.status = &status, V.o.seq_len = &seq_len, V.o.trace_len = &trace_len, V.o.n_win = &n_win;
    V.o.seq = oseq.data(), V.o.qual = oqual.data(), V.o.trace = otrace.data(), V.o.kept = kept.data(), V.o.win = win.data();
    V.prep = prep.data(), V.alen = alen.data(), V.span_e = span_e.data(), V.sc = sc.data(), V.flag = flag.data();
    V.op_r = op_r.data(), V.op_q = op_q.data(), V.cov = cov.data(), V.ulist = ulist.data(), V.rlist = rlist.data();
    V.n_u = &n_u, V.n_r = &n_r;
    run_read_host(V, 0);
    std::printf(">>CASE %s\n", c.name.c_str());
    if (status) {
        std::printf(">>ERROR 1\n>>END\n");
        return;
    }
    std::printf(">>FASTQ\n@%s\n%s\n+\n%s\n>>TRACE\n%s\n>>KEPT\n", rid.c_str(), std::string(oseq.begin(), oseq.begin() + seq_len).c_str(),
                std::string(oqual.begin(), oqual.begin() + seq_len).c_str(), std::string(otrace.begin(), otrace.begin() + trace_len).c_str());
    bool first = true;
    for (int64_t a = 0; a < na; ++a)
        if (kept[a]) std::printf("%s%s", first ? "" : " ", names[a].c_str()), first = false;
    std::printf("\n>>WIN\n");
    for (int k = 0; k < n_win; ++k) std::printf("%s%d,%d", k ? " " : "", win[2 * k], win[2 * k + 1]);
    std::printf("\n>>END\n");
}

}   // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    Case c;
    std::string sect;
    for (std::string line; std::getline(in, line);) {
        if (line.compare(0, 1, "#") == 0 && sect.empty()) continue;
        if (line.compare(0, 7, ">>CASE ") == 0) c = Case(), c.name = line.substr(7), sect = "head";
        else if (line.compare(0, 13, ">>PARAM flags") == 0) c.flags = line.size() > 14 ? line.substr(14) : "";
        else if (line.compare(0, 11, ">>PARAM cfg") == 0) c.cfg = line.size() > 12 ? line.substr(12) : "";
        else if (line == ">>REF") sect = "ref";
        else if (line == ">>SAM") sect = "sam";
        else if (line == ">>END") run_case(c), sect.clear();
        else if (sect == "ref") c.ref.push_back(line);
        else if (sect == "sam" && !line.empty()) c.sam.push_back(line);
    }
    return 0;
}

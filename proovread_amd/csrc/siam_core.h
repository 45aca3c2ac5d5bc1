// siamaera's self-alignments (bin/siamaera:490-579) without blastn, shared by the host path
// (siam_api.cpp) and the kernels (siam_kernels.hip).
//
// A read S of length L in nt4 codes.  Cell (i, p) matches iff both bases are ACGT and
// S[i] == comp(S[p]); a minus-strand self-alignment walks i up and p down.
//   seeds      maximal runs (i + t, p - t) of matching cells, length >= word
//   order      (len desc, i asc, p asc); a seed whose box lies inside the box of an alignment
//              already produced for the read is skipped
//   extension  ksw_extend2 as oracle/sw_oracle.c osw_extend restates it (end_bonus 0), left
//              then right, every DP value carrying (matches, cols) of the predecessor the
//              oracle's comparisons pick
//   identity   kept iff 100 * matches >= min_idy * length
//   culling    -culling_limit 1: dropped when the query interval is enveloped by that of a
//              higher-scoring kept alignment (equal score: the earlier one wins)
// The host forms are plain loops; the device forms of seed search and extension are in
// siam_kernels.hip and use the pieces marked SM_HD here.
#pragma once
#include <stdint.h>

#include "../../include/prgpu.h"

#if defined(__HIPCC__)
#define SM_HD __host__ __device__ inline
#else
#define SM_HD inline
#endif

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace prgpu {
namespace siam {

struct Ext {
    int32_t score, qle, tle, m, c;   // ksw_extend2's max, its cell, (matches, cols) at that cell
};
struct Seed {
    int32_t i, p, len;
};
struct Cell {
    int32_t v, m, c;   // value, matches, columns
};

SM_HD int comp(int c) { return c < 4 ? 3 - c : c; }
SM_HD bool cell_match(const uint8_t *s, int i, int p) { return s[i] < 4 && s[p] < 4 && s[i] + s[p] == 3; }
// osw_fill_scmat: match a, mismatch -b, any N -1
SM_HD int sc(const pr_siam_aligner &al, int q, int t) { return (q > 3 || t > 3) ? -1 : (q == t ? al.a : -al.b); }
SM_HD int is_match(int q, int t) { return q < 4 && q == t; }

// osw_extend's band cap by the longest possible gap (end_bonus 0; o_del == o_ins, e_del == e_ins)
SM_HD int band(const pr_siam_aligner &al, int qlen) {
    int mx = al.a > 0 ? al.a : 0;
    int g = (int)((double)(qlen * mx - al.o) / al.e + 1.);
    g = g > 1 ? g : 1;
    return al.w < g ? al.w : g;
}
// osw_extend's first row in closed form: eh[j].h before any row touched column j
SM_HD int first_row(int h0, int oe, int e, int j) {
    if (j == 0) return h0;
    const int v1 = h0 - oe;
    if (j == 1) return v1 > 0 ? v1 : 0;
    const long prev = (long)v1 - (long)(j - 2) * e;   // eh[j-1].h while the row is still positive
    return prev > e ? (int)(prev - e) : 0;
}
// the first column of row i when the band still touches column 0
SM_HD int first_col(int h0, int o, int e, int i) {
    const int v = h0 - (o + e * (i + 1));
    return v > 0 ? v : 0;
}

// the seed's box inside the box of alignment h
SM_HD bool seed_inside(const pr_siam_hsp &h, int i, int p, int len) {
    return i + 1 >= h.qas && i + len <= h.qae && p - len + 2 >= h.sae && p + 1 <= h.sas;
}
SM_HD pr_siam_hsp make_hsp(int read, int i, int p, int len, const Ext &l, const Ext &r) {
    pr_siam_hsp h;
    h.read = read;
    h.qas = i - l.qle + 1;
    h.qae = i + len + r.qle;
    h.sas = p + l.tle + 1;
    h.sae = p - len - r.tle + 2;
    h.length = len + l.c + r.c;
    h.matches = len + l.m + r.m;
    h.score = r.score;
    return h;
}
// (len desc, i asc, p asc) as one ascending key; len, i, p < 2^18
SM_HD uint64_t seed_key(int i, int p, int len) {
    return (uint64_t)(0x3FFFF - len) << 36 | (uint64_t)i << 18 | (uint64_t)p;
}

// ------------------------------------------------------------------ seeds
// Bit planes of a read: plane c (0..3) has bit i set iff S[i] == c, plane 4 + c has bit k set
// iff comp(S[L-1-k]) == c (the reverse complement); N sets no bit, and bits past L are 0.
// pl[c * nw + w] holds bits 64 w .. 64 w + 63; nw = plane_words(L).  With them, cell
// (i, p) on anti-diagonal d = i + p matches iff planes c and 4 + c agree at i and i + sh,
// sh = L - 1 - d, so one AND per base decides 64 cells.
SM_HD int plane_words(int L) { return (L + 63) >> 6; }
SM_HD void build_plane_word(const uint8_t *s, int L, int nw, int w, uint64_t *pl) {
    uint64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < 64; ++b) {
        const int i = 64 * w + b;
        if (i >= L) break;
        const int x = s[i], y = comp(s[L - 1 - i]);
        if (x < 4) v[x] |= 1ull << b;
        if (y < 4) v[4 + y] |= 1ull << b;
    }
    for (int c = 0; c < 8; ++c) pl[(int64_t)c * nw + w] = v[c];
}
// 64 bits of a plane from bit position `pos` on (any position; outside the plane: 0)
SM_HD uint64_t plane_bits(const uint64_t *pl, int nw, long pos) {
    const long w = pos >> 6;
    const int b = (int)(pos & 63);
    const uint64_t lo = (w >= 0 && w < nw) ? pl[w] : 0, hi = (w + 1 >= 0 && w + 1 < nw) ? pl[w + 1] : 0;
    return b ? (lo >> b | hi << (64 - b)) : lo;
}
// bit q set iff bits q .. q + n - 1 of x are set (n >= 1)
SM_HD uint64_t runs_of(uint64_t x, int n) {
    for (int len = 1; len < n;) {
        const int k = len < n - len ? len : n - len;
        x &= x >> k;
        len += k;
    }
    return x;
}
// Every seed of anti-diagonal d = L - 1 - sh: emit(i, p, len).  The match bits are tested in
// 64-cell windows 32 apart (a run of up to 33 lies inside one of them); a window with a run
// of min(word, 33) has it grown cell by cell to the maximal run, which is emitted once.
template <class Emit>
SM_HD void seeds_of_diagonal(const uint8_t *s, int L, const uint64_t *pl, int nw, int sh, int word, Emit emit) {
    const int d = L - 1 - sh;
    const int lo = sh < 0 ? -sh : 0, hi = sh > 0 ? L - 1 - sh : L - 1;   // cells i of the diagonal
    if (hi - lo + 1 < word) return;
    const int nn = word < 33 ? word : 33;
    const int w0 = lo >> 6, w1 = hi >> 6;
    int done = lo;   // cells below belong to a run already seen
    uint64_t prev = 0;
    for (int w = w0; w <= w1 + 1; ++w) {
        uint64_t cur = 0;
        if (w <= w1)
            for (int c = 0; c < 4; ++c)
                cur |= pl[(int64_t)c * nw + w] & plane_bits(pl + (int64_t)(4 + c) * nw, nw, 64l * w + sh);
        if (w > w0) {
            for (int half = 0; half < 2; ++half) {
                const int base = (w - 1) * 64 + 32 * half;
                uint64_t y = runs_of(half ? (prev >> 32 | cur << 32) : prev, nn);
                while (y) {
                    const int a = base + __builtin_ctzll(y);
                    if (a >= done) {
                        int st = a, en = a + nn;
                        while (st > lo && cell_match(s, st - 1, d - (st - 1))) --st;
                        while (en <= hi && cell_match(s, en, d - en)) ++en;
                        if (en - st >= word) emit(st, d - st, en - st);
                        done = en;
                    }
                    const int k = done - base;
                    y = k >= 64 ? 0 : y & (~0ull << k);
                }
            }
        }
        prev = cur;
    }
}

// ------------------------------------------------------------------ host forms
// every seed of the read, unordered
inline void seeds_host(const uint8_t *s, int L, int word, std::vector<Seed> &out) {
    out.clear();
    if (L < word || L < 1) return;
    const int nw = plane_words(L);
    std::vector<uint64_t> pl((size_t)8 * nw);
    for (int w = 0; w < nw; ++w) build_plane_word(s, L, nw, w, pl.data());
    for (int sh = -(L - 1); sh <= L - 1; ++sh)
        seeds_of_diagonal(s, L, pl.data(), nw, sh, word, [&](int i, int p, int len) { out.push_back({i, p, len}); });
}
inline void sort_seeds(std::vector<Seed> &v) {
    std::sort(v.begin(), v.end(),
              [](const Seed &a, const Seed &b) { return seed_key(a.i, a.p, a.len) < seed_key(b.i, b.p, b.len); });
}

// osw_extend with counts; qa(j) / ta(i) give the bases
template <class Q, class T>
inline Ext extend_host(const pr_siam_aligner &al, int qlen, Q qa, int tlen, T ta, int h0) {
    Ext r = {h0, 0, 0, 0, 0};
    if (qlen <= 0 || tlen <= 0) return r;
    const int oe = al.o + al.e;
    std::vector<Cell> H((size_t)qlen + 1), E((size_t)qlen + 1, Cell{0, 0, 0});
    for (int j = 0; j <= qlen; ++j) {
        const int v = first_row(h0, oe, al.e, j);
        H[j] = v ? Cell{v, 0, j} : Cell{0, 0, 0};
    }
    const int w = band(al, qlen);
    int max = h0, max_i = -1, max_j = -1, beg = 0, end = qlen;
    Cell best = {h0, 0, 0};
    for (int i = 0; i < tlen; ++i) {
        Cell f = {0, 0, 0}, mcell = {0, 0, 0};
        int mm = 0, mj = -1;
        const int tb = ta(i);
        if (beg < i - w) beg = i - w;
        if (end > i + w + 1) end = i + w + 1;
        if (end > qlen) end = qlen;
        Cell h1 = {0, 0, 0};
        if (beg == 0) h1 = Cell{first_col(h0, al.o, al.e, i), 0, i + 1};
        int j;
        for (j = beg; j < end; ++j) {
            Cell M = H[j], e = E[j];
            H[j] = h1;
            const int qb = qa(j);
            if (M.v) {
                M.v += sc(al, qb, tb);
                M.m += is_match(qb, tb);
                M.c += 1;
            } else {
                M = Cell{0, 0, 0};
            }
            Cell h = M.v > e.v ? M : e;
            h = h.v > f.v ? h : f;
            h1 = h;
            if (!(mm > h.v)) mj = j, mcell = h;
            mm = mm > h.v ? mm : h.v;
            int t = M.v - oe;
            t = t > 0 ? t : 0;
            e.v -= al.e;
            if (e.v > t) e.c += 1; else e = Cell{t, M.m, M.c + 1};
            E[j] = e;
            f.v -= al.e;
            if (f.v > t) f.c += 1; else f = Cell{t, M.m, M.c + 1};
        }
        H[end] = h1;
        E[end] = Cell{0, 0, 0};
        if (mm == 0) break;
        if (mm > max) {
            max = mm, max_i = i, max_j = mj, best = mcell;
        } else if (al.zdrop > 0) {
            if (i - max_i > mj - max_j) {
                if (max - mm - ((i - max_i) - (mj - max_j)) * al.e > al.zdrop) break;
            } else {
                if (max - mm - ((mj - max_j) - (i - max_i)) * al.e > al.zdrop) break;
            }
        }
        for (j = beg; j < end && H[j].v == 0 && E[j].v == 0; ++j) {}
        beg = j;
        for (j = end; j >= beg && H[j].v == 0 && E[j].v == 0; --j) {}
        end = j + 2 < qlen ? j + 2 : qlen;
    }
    r.score = max, r.qle = max_j + 1, r.tle = max_i + 1, r.m = best.m, r.c = best.c;
    return r;
}

// the left and right extension of one seed of read s
inline pr_siam_hsp extend_seed_host(const pr_siam_aligner &al, const uint8_t *s, int L, int read, const Seed &sd) {
    const int i = sd.i, p = sd.p, len = sd.len;
    Ext l = extend_host(al, i, [&](int j) { return (int)s[i - 1 - j]; }, L - 1 - p,
                        [&](int k) { return comp(s[p + 1 + k]); }, len * al.a);
    Ext r = extend_host(al, L - i - len, [&](int j) { return (int)s[i + len + j]; }, p - len + 1,
                        [&](int k) { return comp(s[p - len - k]); }, l.score);
    return make_hsp(read, i, p, len, l, r);
}

// every alignment produced for one read, in order of production; returns the PR_SIAM_* flags
// (a flagged read has no alignments)
inline int produce_host(const pr_siam_aligner &al, const uint8_t *s, int64_t L, int read, std::vector<pr_siam_hsp> &out) {
    out.clear();
    if (L > PR_SIAM_MAX_LEN) return PR_SIAM_TOO_LONG;
    std::vector<Seed> seeds;
    seeds_host(s, (int)L, al.word, seeds);
    if (seeds.size() > PR_SIAM_MAX_SEEDS) return PR_SIAM_SEED_OVERFLOW;
    sort_seeds(seeds);
    for (const Seed &sd : seeds) {
        bool skip = false;
        for (const pr_siam_hsp &h : out) skip = skip || seed_inside(h, sd.i, sd.p, sd.len);
        if (skip) continue;
        if (out.size() == PR_SIAM_MAX_HSPS) {
            out.clear();
            return PR_SIAM_HSP_OVERFLOW;
        }
        out.push_back(extend_seed_host(al, s, (int)L, read, sd));
    }
    return 0;
}

// identity threshold, then -culling_limit 1; appends the kept alignments to `out`
inline void select_hsps(const pr_siam_hsp *h, int n, double min_idy, std::vector<pr_siam_hsp> &out) {
    std::vector<int> ok;
    for (int k = 0; k < n; ++k)
        if (100.0 * h[k].matches >= min_idy * h[k].length) ok.push_back(k);
    for (int x : ok) {
        bool culled = false;
        for (int y : ok) {
            if (y == x || h[y].qas > h[x].qas || h[y].qae < h[x].qae) continue;
            if (h[y].score > h[x].score || (h[y].score == h[x].score && y < x)) culled = true;
        }
        if (!culled) out.push_back(h[x]);
    }
}

// siamaera:277-312 / :320-355, the spurious-hit filter
inline std::vector<pr_siam_hsp> spurious_filter(const std::vector<pr_siam_hsp> &b, int L, int seq_min_len) {
    std::vector<pr_siam_hsp> bs;
    int t = (int)(0.05 * L + 0.5);
    if (!t) t = 1;
    ++t;
    for (size_t k = 0; k < b.size(); ++k) {
        if (b[k].qas == b[k].sae && b[k].qae == b[k].sas) {
            if ((double)(b[k].qae - b[k].qas) > 0.7 * seq_min_len) bs.push_back(b[k]);
        } else {
            for (size_t i = 0; i < b.size(); ++i) {
                if (i == k) continue;
                if (std::abs(b[k].qas - b[i].sae) < t && std::abs(b[k].qae - b[i].sas) < t) bs.push_back(b[k]);
            }
        }
    }
    return bs;
}

// siamaera:276-312: pass 1's list after the first filter; true when pass 2 is wanted (:314)
inline bool after_pass1(const pr_siam_params &P, int L, std::vector<pr_siam_hsp> &b) {
    if (b.size() > 2) b = spurious_filter(b, L, P.seq_min_len);
    return b.size() > 2;
}

inline int clampi(long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// siamaera:314-448 from pass 1's filtered list `b` and pass 2's list (used when b has more than 2)
inline pr_siam_decision decide(const pr_siam_params &P, int L, std::vector<pr_siam_hsp> b,
                               const std::vector<pr_siam_hsp> &pass2, int *inconclusive) {
    pr_siam_decision d = {PR_SIAM_KEEP, 0, L};
    *inconclusive = 0;
    if (b.size() > 2 && !pass2.empty()) b = pass2;
    if (b.size() > 2) b = spurious_filter(b, L, P.seq_min_len);
    const int til = P.term_ignore_len + 1;
    if (b.size() == 1) {
        const pr_siam_hsp &h = b[0];
        const double mid = (double)(h.qae - h.qas - 1) / 2 + h.qas;
        if (h.qas <= til) {
            d = {PR_SIAM_TRIM, clampi((long)(mid + P.trim + 0.5), 0, L), L};
        } else if (h.qae > L - til) {
            d = {PR_SIAM_TRIM, 0, clampi((long)(mid - P.trim + 0.5), 0, L)};
        }
    } else if (b.size() == 2) {
        for (const pr_siam_hsp &h : b) {
            if (h.qas <= til) {
                d = {PR_SIAM_TRIM, clampi((long)h.sae - 1 + P.trim, 0, L), L};
                break;
            } else if (h.qae > L - til) {
                d = {PR_SIAM_TRIM, 0, clampi((long)h.sas - P.trim, 0, L)};
                break;
            }
        }
    } else if (b.size() > 2) {
        *inconclusive = 1;
        if (P.filter_inconclusive) d.action = PR_SIAM_DROP;
    }
    return d;
}
}   // namespace siam
}   // namespace prgpu

// Planning of the SW -> consensus hand-off's coordinate sort (the driver in iter_api.cpp, the
// kernels in pipe_kernels.hip and pipe_big.hip): which long reads sort in LDS and which take the
// HBM path, the runs and merge passes of the latter, its scratch and the LDS bytes of both, as
// plain functions of the per-read alignment counts the host already holds.  No HIP here:
// tests/native/handoff_plan_host.cpp drives these on the host.
#pragma once
#include <stdint.h>

#include <vector>

namespace prgpu {
namespace handp {

// keys (8 bytes) one workgroup sorts in LDS: 128 KB of the CU's 160 KB
constexpr int LDS_KEYS = 16384;
// alignments per long read: the consensus kernel's index width (cns_kernels.hip, i >= 1 << 20)
constexpr int64_t MAX_ALNS = (int64_t)1 << 20;
// outputs a workgroup of a merge pass writes (256 threads x 8 keys)
constexpr int MERGE_TILE = 2048;

inline bool is_big(int64_t n) { return n > LDS_KEYS; }
inline bool refused(int64_t n) { return n > MAX_ALNS; }
inline int pow2_cover(int64_t n) {
    int s = 1;
    while (s < n) s <<= 1;
    return s;
}
// sorted runs of at most LDS_KEYS keys a big read is cut into
inline int64_t runs(int64_t n) { return (n + LDS_KEYS - 1) / LDS_KEYS; }
// pairwise merge passes until one run is left
inline int merge_passes(int64_t n_runs) {
    int p = 0;
    while (((int64_t)1 << p) < n_runs) ++p;
    return p;
}

struct Plan {
    int64_t max_count = 0;      // most alignments on one read (the consensus K pool's bound)
    int sort_cap = 1;           // LDS sort: power of two covering the largest read it takes
    int lds_bytes = 8;          // its dynamic LDS
    int64_t n_big = 0;          // reads on the HBM path
    int64_t big_keys = 0;       // their counts summed
    int64_t max_big = 0;        // the largest of them
    int max_runs = 0;
    int passes = 0;             // merge passes (the largest read's; shorter reads are copied along)
    int lds_big_bytes = 0;      // LDS of the run sort
    int64_t scratch_bytes = 0;  // two key buffers (ping-pong)
    int refused_lr = -1;        // first read beyond MAX_ALNS, and its count
    int64_t refused_count = 0;
    std::vector<int32_t> big_lr;    // [n_big] the big reads
    std::vector<int64_t> big_off;   // [n_big + 1] first key of each in a scratch buffer
};

// counts: per long read, the alignments before the -T / -b/-l predicate (upper bounds)
template <class T>
inline Plan plan(const T *counts, int64_t n) {
    Plan p;
    int64_t small_max = 0;
    p.big_off.push_back(0);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t k = (int64_t)counts[i];
        if (k > p.max_count) p.max_count = k;
        if (refused(k)) {
            if (p.refused_lr < 0) p.refused_lr = (int)i, p.refused_count = k;
        } else if (is_big(k)) {
            p.big_lr.push_back((int32_t)i);
            p.big_keys += k;
            p.big_off.push_back(p.big_keys);
            if (k > p.max_big) p.max_big = k;
        } else if (k > small_max) {
            small_max = k;
        }
    }
    p.n_big = (int64_t)p.big_lr.size();
    p.sort_cap = pow2_cover(small_max);
    p.lds_bytes = p.sort_cap * 8;
    if (p.n_big) {
        p.max_runs = (int)runs(p.max_big);
        p.passes = merge_passes(p.max_runs);
        p.lds_big_bytes = LDS_KEYS * 8;
        p.scratch_bytes = 2 * 8 * p.big_keys;
    }
    return p;
}

}  // namespace handp
}  // namespace prgpu

// Device-side descriptors of the siamaera kernels (siam_kernels.hip).
#pragma once
#include <stdint.h>

#include "siam_core.h"

namespace prgpu {

struct SiamDev {
    int32_t n;                 // reads
    const int64_t *off;        // [n+1] read offsets into seq
    const uint8_t *seq;        // nt4 codes
    uint64_t *planes;          // scratch: read r's bit planes, 8 * plane_words(len) words at plane_off[r]
    const int64_t *plane_off;  // [n]
    siam::Seed *seeds;         // [n * PR_SIAM_MAX_SEEDS] per-read seed slices, unordered
    int32_t *n_seeds;          // [n] seeds found (may exceed the slice; zeroed by the launch)
    pr_siam_hsp *hsps;         // [n * PR_SIAM_MAX_HSPS] alignments in order of production
    int32_t *n_hsps;           // [n]
    int32_t *status;           // [n] PR_SIAM_* flags
    pr_siam_aligner al;
};

// a batch of plain extensions (pr_siam_extend_gpu)
struct SiamPairs {
    int32_t n;
    const uint8_t *q, *t;
    const int64_t *q_off, *t_off;   // [n+1]
    const int32_t *h0;              // [n]
    int32_t *out;                   // [5 n] score, qle, tle, matches, cols
    pr_siam_aligner al;
};

// Enqueue seed search and extension of D.n reads on `stream` (hipStream_t).  Returns a hipError_t.
int siam_launch(const SiamDev &D, void *stream);
int siam_pairs_launch(const SiamPairs &D, void *stream);

}   // namespace prgpu

// Device-side descriptors of the ccs-1 kernels (ccs_kernels.hip).
#pragma once
#include <stdint.h>

#include "ccs_core.h"

namespace prgpu {

// the batch and its alignments in device memory (pr_ccs_batch / pr_ccs_alns)
struct CcsDev {
    pr_ccs_params p;
    const uint8_t *seq, *qual;
    const int64_t *off;                 // [n_sub + 1]
    const int32_t *grp_off, *grp_ref;   // [n_groups + 1], [n_groups]
    const int64_t *cig_off;             // [n_sub + 1]
    int32_t *mapped, *strand, *pos, *score, *n_cigar;   // [n_sub]
    uint32_t *cigar;
};

// mapping: pair k is subread pair_sub[k] against reference subread pair_ref[k]
struct CcsMapDev {
    int32_t n_pairs;
    const int32_t *pair_sub, *pair_ref;
    uint32_t *bsum;          // per pair 2 * (buckets + 1) seed length sums at b_off[k], zeroed
    uint64_t *bkey;          // ... and best seed keys
    const int64_t *b_off;    // [n_pairs]
    ccs::Centre *centre;     // [n_pairs]
    uint8_t *dir;            // direction bytes, rows x (2 w + 1) of pair k at dir_off[k]
    const int64_t *dir_off;  // [n_pairs] (valid for the pairs of the current chunk)
    int32_t first, count;    // the chunk of pairs the alignment launch covers
};

// consensus: block k works on group glist[k]
struct CcsCnsDev {
    int32_t n;
    const int32_t *glist;
    ccs::ColEnt *slab;         // (subreads - 1) x reference length entries of block k at slab_off[k]
    const int64_t *slab_off;   // [n]
    int32_t *op_r, *op_q;      // first column / window position of every CIGAR op (slots of cig_off)
    const int64_t *out_off;    // [n_groups + 1]
    uint8_t *seq, *qual, *trace;
    int32_t *status, *seq_len, *trace_len;   // [n_groups]
};

// Enqueue on `stream` (hipStream_t); return a hipError_t.
int ccs_seeds_launch(const CcsDev &D, const CcsMapDev &M, void *stream);
int ccs_align_launch(const CcsDev &D, const CcsMapDev &M, void *stream);
int ccs_cns_launch(const CcsDev &D, const CcsCnsDev &C, void *stream);

}   // namespace prgpu

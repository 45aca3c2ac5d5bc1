// Device-side descriptor of the BAM record decoder (bam_kernels.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace prgpu {

// error bits of BamDev.err[0]
enum { BAM_E_AUX = 1, BAM_E_RID = 2, BAM_E_ORDER = 4, BAM_E_NOSEQ = 8 };

struct BamDev {
    const uint8_t *recs;         // the record stream (block_size-prefixed records)
    const int64_t *off;          // [n] start of every record (host pre-pass)
    int64_t n;                   // records
    const int32_t *ref_to_lr;    // [n_ref] reference id -> long read of the batch or -1; NULL: keep every record
    int32_t n_ref;
    // field pass, file order
    double *f_score;             // [n]
    uint8_t *f_flags;            // [n] PR_ALN_* | BAM_AS_TEXT
    int32_t *f_keep;             // [n + 1] 1: the record is kept (entry n: 0)
    unsigned long long *cnt_ref; // [n_ref] kept records per reference id (zeroed by the caller)
    int32_t *err;                // [0] BAM_E_* bits, [1] records with a text AS (both zeroed by the caller)
    int32_t *text_list;          // [n] their record indices, unordered
    // placement: kept record i goes to column kidx[i] + delta[rid]
    const int64_t *kidx;         // [n + 1] exclusive scan of f_keep
    const int64_t *ref_start;    // [n_ref + 1] exclusive scan of cnt_ref (NULL with ref_to_lr NULL)
    const int64_t *delta;        // [n_ref] first column of the reference's long read - ref_start (NULL: 0)
    int64_t n_kept;
    int32_t *a_rid;              // [n_kept] or NULL
    int32_t *a_pos;              // [n_kept] POS + 1
    double *a_score;
    uint8_t *a_flags;
    int32_t *a_lseq, *a_ncig;    // [n_kept + 1] (entry n_kept: 0)
    int64_t *a_src;              // [n_kept] the record of a column
    // unpack pass
    const int64_t *seq_off, *cig_off;   // [n_kept + 1] exclusive scans of a_lseq / a_ncig
    uint8_t *seq, *qual;         // pools (qual may be NULL)
    uint32_t *cig;
    unsigned long long *ins;     // [n_lr] inserted bases of a long read's alignments (zeroed by the caller), or NULL
};

size_t bam_scan_temp_bytes(int64_t n);
// each returns a hipError_t; all enqueue on `stream`
int bam_field_pass(const BamDev &D, int64_t *kidx_out, void *temp, size_t temp_bytes, void *stream);
int bam_place_pass(const BamDev &D, int64_t *seq_off_out, int64_t *cig_off_out, void *temp, size_t temp_bytes, void *stream);
int bam_unpack_pass(const BamDev &D, void *stream);

}   // namespace prgpu

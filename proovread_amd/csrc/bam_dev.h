// Device-side descriptor of the BAM record decoder (bam_kernels.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace prgpu {

// error bits of BamDev.err[0]
enum { BAM_E_AUX = 1, BAM_E_RID = 2, BAM_E_ORDER = 4, BAM_E_NOSEQ = 8,
       BAM_E_NODONOR = 16, BAM_E_DONORLEN = 32 };   // PR_BAM_RESTORE_SEQ only (bam_core.h states the rule)

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
    // PR_BAM_RESTORE_SEQ (all NULL / 0 without it: the three kernels above never read them)
    unsigned long long *tab;     // [tab_mask + 1] the donor table: record indices, BAM_SLOT_EMPTY where free
    int64_t tab_mask;
    unsigned long long *rst;     // [0] lowest record without a donor, [1] lowest record whose lengths differ from
                                 // its donor's (both ~0 from the caller), [2] restored columns (zeroed)
    int64_t *a_seq_src;          // [n_kept] the record whose SEQ / QUAL a column takes (its own, or the donor)
    int32_t *a_hl;               // [n_kept] first base of the slice in the record's orientation (the leading H)
    uint8_t *a_rc;               // [n_kept] 1: the donor lies on the other strand
};

size_t bam_scan_temp_bytes(int64_t n);
// each returns a hipError_t; all enqueue on `stream`
int bam_field_pass(const BamDev &D, int64_t *kidx_out, void *temp, size_t temp_bytes, void *stream);
int bam_place_pass(const BamDev &D, int64_t *seq_off_out, int64_t *cig_off_out, void *temp, size_t temp_bytes, void *stream);
int bam_unpack_pass(const BamDev &D, void *stream);
// PR_BAM_RESTORE_SEQ: the donor table of the stream; bam_place_pass with the lookup of every
// column without SEQ between the placement and the scans; bam_unpack_pass reading SEQ / QUAL
// through a_seq_src
int bam_donor_pass(const BamDev &D, void *stream);
int bam_place_restore_pass(const BamDev &D, int64_t *seq_off_out, int64_t *cig_off_out, void *temp, size_t temp_bytes, void *stream);
int bam_unpack_restore_pass(const BamDev &D, void *stream);

}   // namespace prgpu

// Device-side descriptor of the BAM record encoder (bam_enc_kernels.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace prgpu {

struct BamEncDev {
    // the exported range: hand-off alignments [g0, g0 + n) of long reads [lr_first, lr_first + lr_count)
    int64_t g0, n;
    int32_t lr_first, lr_count;
    const int64_t *aln_off;      // [n_lr + 1] first hand-off alignment of every long read
    // the hand-off's columns (PipeDev::a_*), indexed by hand-off alignment
    const int32_t *a_pos;        // POS + 1
    const double *a_score;
    const int32_t *a_lseq, *a_ncig;
    const int32_t *a_task;       // the alignment's index among its long read's grouped alignments
    // the SW stage's alignments grouped by long read (SwPtrs after the regrouping)
    const int64_t *task_off;     // [n_lr + 1]
    const int32_t *t_sr;         // short read
    const uint8_t *strand;
    const int64_t *cig_at;       // first op in the SW CIGAR pool
    const int32_t *glist;        // the SW task that reported the grouped alignment
    const uint32_t *cig;         // SW CIGAR pool
    const uint8_t *sr;           // short reads, nt4
    const int64_t *sr_off;       // [n_sr + 1]
    // the FLAG column: SAM order in, by SW task out
    const int32_t *alist;        // [n_sam] the SW task of every alignment in SAM order
    const int32_t *aflag;        // [n_sam] its FLAG
    int64_t n_sam;
    uint16_t *flag_by_task;      // [n_task]
    // the call's uploads
    const uint8_t *names;
    const int64_t *name_off;     // [n_sr + 1]
    const uint8_t *qual;         // phred + 33 in sr_off layout, or NULL
    // per exported alignment
    int32_t *e_lr;               // [n] long read
    int32_t *e_j;                // [n] grouped index
    int64_t *e_size;             // [n + 1] record bytes (entry n: 0)
    const int64_t *e_off;        // [n + 1] exclusive scan of e_size
    uint8_t *out;                // the record stream
};

size_t bam_enc_temp_bytes(int64_t n);
// each returns a hipError_t; all enqueue on `stream`
int bam_enc_flag_pass(const BamEncDev &D, void *stream);
int bam_enc_size_pass(const BamEncDev &D, int64_t *off_out, void *temp, size_t temp_bytes, void *stream);
int bam_enc_write_pass(const BamEncDev &D, void *stream);
// after the size pass: out[i] = the bytes of the records of long read lr_first + i
int bam_enc_read_bytes(const BamEncDev &D, int64_t *out, void *stream);

}   // namespace prgpu

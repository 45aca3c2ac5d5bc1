// Sizing of the resident consensus batch (the drivers in cns_api.cpp, iter_api.cpp and
// xchg_api.cpp): the device buffers whose size follows the batch, stated once, and the output
// capacities of a pipeline batch, as plain functions of the counts the host already holds.
// No HIP here: tests/native/cns_plan_host.cpp drives these on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace prgpu {

enum CnsBufId {
    CB_LR_OFF, CB_REF_SEQ, CB_REF_QUAL, CB_IGN_OFF, CB_IGN, CB_ALN_OFF, CB_POS, CB_SCORE, CB_AFLAGS,
    CB_SEQ_OFF, CB_LSEQ, CB_CIG_OFF, CB_NCIG, CB_SEQ, CB_CIG,
    CB_A_ST, CB_A_LEN, CB_A_NC, CB_A_BIN, CB_A_CB, CB_A_CE, CB_A_SB, CB_A_RPOS, CB_A_END,
    CB_SORTED, CB_LST_SCORE, CB_LST_ALN, CB_KEPT, CB_BIN_OFF, CB_BIN_BASES, CB_WORK,
    CB_OUT_OFF, CB_CHIM_OFF, CB_STATUS, CB_SEQ_LEN, CB_TRACE_LEN, CB_NCIGAR, CB_NCHIM,
    CB_O_SEQ, CB_O_QUAL, CB_O_TRACE, CB_O_CIG, CB_O_CHIM, CB_PROF, CB_RETRY, CB_K,
    CB_GSZS, CB_GSZC, CB_GSO, CB_GCO, CB_GTMP,
    CB_COUNT
};

// per-phase wall-clock ticks of the consensus kernel (CB_PROF): prep, binning, state table,
// scatter, argmax+write, cigar, chimera, idle; scatter detail: zero+ignore, group select, staging,
// walks; counts: groups, items, windows
constexpr int CNS_NPHASE = 24;

namespace cnsp {

// the batch's counts (pr_ctx: n_lr, n_aln, seq_cap, chim_cap)
struct Sizes {
    int64_t n_lr, n_aln, seq_cap, chim_cap;
};

// what a buffer's element count follows: alignments + 1, long reads + 1, output bytes + 1,
// chimera records + 1, long reads + 16 (the retry list and its counter), or nothing (elem bytes)
enum Scale { PER_ALN, PER_LR, PER_SEQ, PER_CHIM, PER_LR_RETRY, FIXED };

// the groups a caller sizes on their own (a mask): pr_cns_upload uploads the alignment offsets
// and inputs itself, an owned batch sizes the per-alignment arrays only at launch
enum Group : unsigned {
    ALN_OFF = 1,       // the alignments' per-read offsets
    ALN_IN = 2,        // per-alignment inputs (the hand-off's outputs)
    ALN_SCRATCH = 4,   // per-alignment scratch of the consensus kernel
    READ_OUT = 8,      // per-read outputs, the output pools, the small fixed buffers
    ALL = 15
};

struct Entry {
    CnsBufId id;
    unsigned group;
    Scale scale;
    size_t elem;   // bytes per element
};

constexpr Entry TABLE[] = {
    {CB_ALN_OFF, ALN_OFF, PER_LR, 8},
    {CB_POS, ALN_IN, PER_ALN, 4},
    {CB_SCORE, ALN_IN, PER_ALN, 8},
    {CB_AFLAGS, ALN_IN, PER_ALN, 1},
    {CB_SEQ_OFF, ALN_IN, PER_ALN, 8},
    {CB_LSEQ, ALN_IN, PER_ALN, 4},
    {CB_CIG_OFF, ALN_IN, PER_ALN, 8},
    {CB_NCIG, ALN_IN, PER_ALN, 4},
    {CB_A_ST, ALN_SCRATCH, PER_ALN, 4},
    {CB_A_LEN, ALN_SCRATCH, PER_ALN, 4},
    {CB_A_NC, ALN_SCRATCH, PER_ALN, 8},
    {CB_A_BIN, ALN_SCRATCH, PER_ALN, 4},
    {CB_A_CB, ALN_SCRATCH, PER_ALN, 4},
    {CB_A_CE, ALN_SCRATCH, PER_ALN, 4},
    {CB_A_SB, ALN_SCRATCH, PER_ALN, 4},
    {CB_A_RPOS, ALN_SCRATCH, PER_ALN, 4},
    {CB_A_END, ALN_SCRATCH, PER_ALN, 4},
    {CB_SORTED, ALN_SCRATCH, PER_ALN, 4},
    {CB_LST_SCORE, ALN_SCRATCH, PER_ALN, 8},
    {CB_LST_ALN, ALN_SCRATCH, PER_ALN, 4},
    {CB_KEPT, ALN_SCRATCH, PER_ALN, 1},
    {CB_WORK, READ_OUT, FIXED, 64},
    {CB_PROF, READ_OUT, FIXED, CNS_NPHASE * 8},
    {CB_RETRY, READ_OUT, PER_LR_RETRY, 4},
    {CB_STATUS, READ_OUT, PER_LR, 4},
    {CB_SEQ_LEN, READ_OUT, PER_LR, 4},
    {CB_TRACE_LEN, READ_OUT, PER_LR, 4},
    {CB_NCIGAR, READ_OUT, PER_LR, 4},
    {CB_NCHIM, READ_OUT, PER_LR, 4},
    {CB_O_SEQ, READ_OUT, PER_SEQ, 1},
    {CB_O_QUAL, READ_OUT, PER_SEQ, 1},
    {CB_O_TRACE, READ_OUT, PER_SEQ, 1},
    {CB_O_CIG, READ_OUT, PER_SEQ, 4},
    {CB_O_CHIM, READ_OUT, PER_CHIM, 16},
};
constexpr int N_TABLE = (int)(sizeof TABLE / sizeof TABLE[0]);

// bytes the entry's buffer must hold (what the caller asks DevBuf::ensure for)
inline size_t bytes(const Entry &e, const Sizes &z) {
    switch (e.scale) {
    case PER_ALN: return ((size_t)z.n_aln + 1) * e.elem;
    case PER_LR: return ((size_t)z.n_lr + 1) * e.elem;
    case PER_SEQ: return ((size_t)z.seq_cap + 1) * e.elem;
    case PER_CHIM: return ((size_t)z.chim_cap + 1) * e.elem;
    case PER_LR_RETRY: return ((size_t)z.n_lr + 16) * e.elem;
    case FIXED: break;
    }
    return e.elem;
}

// chimera records a long read of L bases can report: bins / 2 + 2, bins at the smallest bin
// size bam2cns uses (20)
inline int64_t chim_records(int64_t L) {
    const int64_t nb = (int64_t)((double)L / 20.0) + 1;
    return nb / 2 + 2;
}

// output capacities of a pipeline batch (the alignments are not known at upload): 2 L + 1024
// consensus bytes per long read, guarded in the kernel
// (out_off, chim_off: n_lr + 1 entries each)
inline void pipe_caps(const int64_t *lr_off, int n_lr, int64_t *out_off, int64_t *chim_off) {
    out_off[0] = chim_off[0] = 0;
    for (int i = 0; i < n_lr; ++i) {
        const int64_t L = lr_off[i + 1] - lr_off[i];
        out_off[i + 1] = out_off[i] + 2 * L + 1024;
        chim_off[i + 1] = chim_off[i] + chim_records(L);
    }
}

}  // namespace cnsp
}  // namespace prgpu

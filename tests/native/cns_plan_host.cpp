// proovread_amd/csrc/cns_plan.h compiled for the host (tests/test_cns_plan.py).
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../proovread_amd/csrc/cns_plan.h"

using namespace prgpu;

extern "C" {

// the id of a consensus buffer by its name in CnsBufId, -1: no such name
int cns_plan_id(const char *name) {
#define ID(x) {#x, x}
    static const struct { const char *name; int id; } ids[] = {
        ID(CB_LR_OFF), ID(CB_REF_SEQ), ID(CB_REF_QUAL), ID(CB_IGN_OFF), ID(CB_IGN), ID(CB_ALN_OFF), ID(CB_POS),
        ID(CB_SCORE), ID(CB_AFLAGS), ID(CB_SEQ_OFF), ID(CB_LSEQ), ID(CB_CIG_OFF), ID(CB_NCIG), ID(CB_SEQ), ID(CB_CIG),
        ID(CB_A_ST), ID(CB_A_LEN), ID(CB_A_NC), ID(CB_A_BIN), ID(CB_A_CB), ID(CB_A_CE), ID(CB_A_SB), ID(CB_A_RPOS),
        ID(CB_A_END), ID(CB_SORTED), ID(CB_LST_SCORE), ID(CB_LST_ALN), ID(CB_KEPT), ID(CB_BIN_OFF), ID(CB_BIN_BASES),
        ID(CB_WORK), ID(CB_OUT_OFF), ID(CB_CHIM_OFF), ID(CB_STATUS), ID(CB_SEQ_LEN), ID(CB_TRACE_LEN), ID(CB_NCIGAR),
        ID(CB_NCHIM), ID(CB_O_SEQ), ID(CB_O_QUAL), ID(CB_O_TRACE), ID(CB_O_CIG), ID(CB_O_CHIM), ID(CB_PROF), ID(CB_RETRY),
        ID(CB_K), ID(CB_GSZS), ID(CB_GSZC), ID(CB_GSO), ID(CB_GCO), ID(CB_GTMP)};
#undef ID
    static_assert(sizeof ids / sizeof ids[0] == CB_COUNT, "every CnsBufId");
    for (const auto &e : ids)
        if (strcmp(e.name, name) == 0) return e.id;
    return -1;
}

// the mask of a group by name ("aln_off", "aln_in", "aln_scratch", "read_out")
unsigned cns_plan_group(const char *name) {
    if (!strcmp(name, "aln_off")) return cnsp::ALN_OFF;
    if (!strcmp(name, "aln_in")) return cnsp::ALN_IN;
    if (!strcmp(name, "aln_scratch")) return cnsp::ALN_SCRATCH;
    if (!strcmp(name, "read_out")) return cnsp::READ_OUT;
    return 0;
}
unsigned cns_plan_all() { return cnsp::ALL; }

// the entries of `groups` in table order: ids[k], bytes[k] (up to cap); returns their number
int cns_plan_sizes(unsigned groups, int64_t n_lr, int64_t n_aln, int64_t seq_cap, int64_t chim_cap, int32_t *ids,
                   int64_t *bytes, int cap) {
    const cnsp::Sizes z = {n_lr, n_aln, seq_cap, chim_cap};
    int n = 0;
    for (const cnsp::Entry &e : cnsp::TABLE) {
        if (!(e.group & groups)) continue;
        if (n < cap) ids[n] = e.id, bytes[n] = (int64_t)cnsp::bytes(e, z);
        ++n;
    }
    return n;
}

// out_off / chim_off [n_lr + 1] of a pipeline batch
void cns_plan_pipe_caps(const int64_t *lr_off, int n_lr, int64_t *out_off, int64_t *chim_off) {
    cnsp::pipe_caps(lr_off, n_lr, out_off, chim_off);
}
}

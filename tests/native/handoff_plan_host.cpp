// proovread_amd/csrc/handoff_plan.h compiled for the host (tests/test_handoff_plan.py).
#include <stddef.h>
#include <stdint.h>

#include "../../proovread_amd/csrc/handoff_plan.h"

using namespace prgpu;

extern "C" {

int handoff_out_count() { return 13; }
int handoff_lds_keys() { return handp::LDS_KEYS; }
int64_t handoff_max_alns() { return handp::MAX_ALNS; }
int handoff_merge_tile() { return handp::MERGE_TILE; }

// out: [max_count, sort_cap, lds_bytes, n_big, big_keys, max_big, max_runs, passes, lds_big_bytes,
// scratch_bytes, refused_lr, refused_count, runs and passes of counts[0] alone];
// big_lr [n] / big_off [n + 1]: the first n_big (+ 1) entries are filled
void handoff_plan_case(const int64_t *counts, int64_t n, int64_t *out, int32_t *big_lr, int64_t *big_off) {
    const handp::Plan p = handp::plan(counts, n);
    const int64_t v[13] = {p.max_count, p.sort_cap, p.lds_bytes, p.n_big, p.big_keys, p.max_big, p.max_runs, p.passes,
                           p.lds_big_bytes, p.scratch_bytes, p.refused_lr, p.refused_count,
                           n ? handp::runs(counts[0]) * 100 + handp::merge_passes(handp::runs(counts[0])) : 0};
    for (int k = 0; k < 13; ++k) out[k] = v[k];
    for (size_t k = 0; k < p.big_lr.size(); ++k) big_lr[k] = p.big_lr[k];
    for (size_t k = 0; k < p.big_off.size(); ++k) big_off[k] = p.big_off[k];
}
}

// Host driver of seed_plan.h's pass1b_batch, out_budget and pass1_budget for tests/test_seed_plan_batch.py.
#include "../../proovread_amd/csrc/seed_plan.h"

using namespace prgpu;

// in: n_flagged, waves, scratch_cap, sb, wb, force -> out: batch, waves
extern "C" void batch_case(const int64_t *in, int64_t *out) {
    seedp::Pass1bRun r{};
    r.wb = in[4];
    const seedp::Pass1bBatch b = seedp::pass1b_batch(r, in[0], in[1], in[2], in[3], (int)in[5]);
    out[0] = b.batch;
    out[1] = b.waves;
}

extern "C" int64_t out_budget_case(int64_t free_bytes, int64_t have) { return seedp::out_budget(free_bytes, have); }
extern "C" int64_t pass1_budget_case(int64_t free_bytes, int64_t have, int64_t full) {
    return seedp::pass1_budget(free_bytes, have, full);
}
extern "C" int64_t scratch_budget_case(int64_t free_bytes, int64_t have) { return seedp::scratch_budget(free_bytes, have); }

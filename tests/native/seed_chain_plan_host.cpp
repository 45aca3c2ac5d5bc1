// Host driver of seed_plan.h's occ_pool_words for tests/test_seed_chain_plan.py.
#include "../../proovread_amd/csrc/seed_plan.h"

using namespace prgpu;

extern "C" int64_t occ_pool_words_case(int64_t n_reads, int lazy, int64_t free_bytes, int64_t have) {
    return seedp::occ_pool_words(n_reads, lazy != 0, free_bytes, have);
}
extern "C" int64_t occ_one_list_words() { return seedc::occ_words(seedc::OCC_MAX); }
extern "C" int64_t occ_words_case(int n) { return seedc::occ_words(n); }
extern "C" int occ_taken_case(int max_occ, int64_t np) {
    pr_seed_opts o{};
    o.max_occ = max_occ;
    return seedc::occ_taken(o, np);
}

// Device-side entry points of the unitig consensus kernels (utg_kernels.hip).  The descriptor is
// utg_core.h's View with device pointers.
#pragma once
#include <stdint.h>

#include "utg_core.h"

namespace prgpu {

// the outputs gathered behind each other for one download: read r's sequence and quality at
// seq_at[r], its trace at trace_at[r]
struct UtgPackDev {
    const int64_t *seq_at, *trace_at;   // [n_reads]
    uint8_t *seq, *qual, *trace;
};

// Enqueue on `stream` (hipStream_t); return a hipError_t.
int utg_prep_launch(const utg::View &V, void *stream);
int utg_cov_launch(const utg::View &V, void *stream);
int utg_contained_launch(const utg::View &V, void *stream);
int utg_cns_launch(const utg::View &V, void *stream);
int utg_pack_launch(const utg::View &V, const UtgPackDev &P, void *stream);

}   // namespace prgpu

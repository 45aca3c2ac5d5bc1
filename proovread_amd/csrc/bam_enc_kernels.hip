// The hand-off's alignments -> BAM records, on the device (bam_enc_core.h states the record
// layout and the store rule; bam_api.cpp drives the passes).
//
//   bam_enc_flag_kernel   one lane per alignment of the SW stage's final pass, SAM order: its FLAG
//                         goes to the SW task that reported it (the hand-off lists tasks through
//                         the long-read grouping, the FLAG column is in SAM order).
//   bam_enc_size_kernel   one lane per exported alignment: its long read (a search over the
//                         reads' first alignments), its index in the long-read grouping, and the
//                         record's size.
//   (scan)                sizes -> each record's offset in the exported stream.
//   bam_enc_write_kernel  one 16-lane group per record, four records per wave: the reference span
//                         of the CIGAR reduced over the group (the bin), then the record's bytes,
//                         each lane writing aligned 16-byte chunks.
//                         A record byte is made of one or two single-byte loads and a per-byte choice
//                         of its part; that, not HBM, bounds the pass (8 % of the HBM
//                         peak), which is small beside the download of the stream.
// No LDS, no MFMA.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "bam_enc_core.h"
#include "bam_enc_dev.h"

namespace prgpu {
namespace {

using namespace bam;

__global__ __launch_bounds__(256) void bam_enc_flag_kernel(BamEncDev D) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < D.n_sam; i += (int64_t)gridDim.x * 256)
        D.flag_by_task[D.alist[i]] = (uint16_t)D.aflag[i];
}

__global__ __launch_bounds__(256) void bam_enc_size_kernel(BamEncDev D) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e <= D.n; e += (int64_t)gridDim.x * 256) {
        if (e == D.n) {
            D.e_size[e] = 0;
            continue;
        }
        const int64_t g = D.g0 + e;
        // the last read of the range whose first alignment is at or before g (empty reads share
        // their successor's first alignment, so this is the read that holds g)
        int32_t lo = D.lr_first, hi = D.lr_first + D.lr_count;
        while (hi - lo > 1) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (D.aln_off[mid] <= g) lo = mid;
            else hi = mid;
        }
        const int64_t j = D.task_off[lo] + D.a_task[g];
        const int32_t sid = D.t_sr[j];
        D.e_lr[e] = lo;
        D.e_j[e] = (int32_t)j;
        D.e_size[e] = enc_size((int32_t)(D.name_off[sid + 1] - D.name_off[sid]), D.a_ncig[g], D.a_lseq[g],
                               (int32_t)D.a_score[g]);
    }
}

__global__ __launch_bounds__(256) void bam_enc_write_kernel(BamEncDev D) {
    const int lane = threadIdx.x & 15;
    for (int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; e < D.n; e += (int64_t)gridDim.x * 16) {
        const int64_t g = D.g0 + e;
        const int64_t j = D.e_j[e];
        const int32_t sid = D.t_sr[j];
        const int64_t so = D.sr_off[sid], no = D.name_off[sid];
        EncRec R;
        R.rid = D.e_lr[e];
        R.pos = D.a_pos[g] - 1;
        R.flag = D.flag_by_task[D.glist[j]];
        R.score = (int32_t)D.a_score[g];
        R.l_name = (int32_t)(D.name_off[sid + 1] - no);
        R.n_cigar = D.a_ncig[g];
        R.l_seq = D.a_lseq[g];
        R.rev = D.strand[j] ? 1 : 0;
        R.name = D.names + no;
        R.cig = D.cig + D.cig_at[j];
        R.seq = D.sr + so;
        R.qual = D.qual ? D.qual + so : nullptr;
        long long span = enc_span_part(R.cig, R.n_cigar, lane, 16);
        for (int m = 8; m; m >>= 1) span += __shfl_xor(span, m, 16);
        enc_write(R, span, D.out + D.e_off[e], lane, 16);
    }
}

__global__ __launch_bounds__(256) void bam_enc_read_bytes_kernel(BamEncDev D, int64_t *out) {
    for (int32_t i = blockIdx.x * 256 + threadIdx.x; i < D.lr_count; i += gridDim.x * 256)
        out[i] = D.e_off[D.aln_off[D.lr_first + i + 1] - D.g0] - D.e_off[D.aln_off[D.lr_first + i] - D.g0];
}

unsigned grid_for(int64_t items) {
    int64_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}   // namespace

size_t bam_enc_temp_bytes(int64_t n) {
    size_t tb = 0;
    (void)rocprim::exclusive_scan(nullptr, tb, (int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)(n + 1),
                                  rocprim::plus<int64_t>());
    return tb + 256;
}

int bam_enc_flag_pass(const BamEncDev &D, void *stream) {
    if (D.n_sam <= 0) return 0;
    hipLaunchKernelGGL(bam_enc_flag_kernel, dim3(grid_for(D.n_sam)), dim3(256), 0, (hipStream_t)stream, D);
    return (int)hipGetLastError();
}

int bam_enc_size_pass(const BamEncDev &D, int64_t *off_out, void *temp, size_t temp_bytes, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bam_enc_size_kernel, dim3(grid_for(D.n + 1)), dim3(256), 0, s, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    size_t tb = temp_bytes;
    return (int)rocprim::exclusive_scan(temp, tb, D.e_size, off_out, (int64_t)0, (size_t)(D.n + 1), rocprim::plus<int64_t>(), s);
}

int bam_enc_read_bytes(const BamEncDev &D, int64_t *out, void *stream) {
    if (D.lr_count <= 0) return 0;
    hipLaunchKernelGGL(bam_enc_read_bytes_kernel, dim3(grid_for(D.lr_count)), dim3(256), 0, (hipStream_t)stream, D, out);
    return (int)hipGetLastError();
}

int bam_enc_write_pass(const BamEncDev &D, void *stream) {
    if (D.n <= 0) return 0;
    hipLaunchKernelGGL(bam_enc_write_kernel, dim3(grid_for(D.n * 16)), dim3(256), 0, (hipStream_t)stream, D);
    return (int)hipGetLastError();
}

}   // namespace prgpu

// BAM records -> the consensus stage's alignment columns, on the device (bam_core.h states
// the record layout and the unpack rules; bam_api.cpp drives the passes).
//
//   bam_field_kernel    one lane per record, file order: the aux walk for the last AS tag
//                       (score, PR_ALN_* flags), the long read of the record's reference id and
//                       whether the record is kept, a histogram of the kept records over the
//                       reference ids (one atomic per wave when the wave's records share a
//                       reference, as they mostly do in a coordinate-sorted stream).
//   (scan)              kept flags -> the kept records' file-order index.
//   bam_place_kernel    one lane per record: a kept record's column is its kept index moved by
//                       its reference's delta (the reads of the batch may be ordered differently
//                       from the BAM header's references; inside a read the file order stays).
//                       The stream is coordinate-sorted iff every kept index lies inside its
//                       reference's block of the histogram's scan, which is checked here.
//   (scans)             l_seq, n_cigar of the columns -> offsets into the pools.
//   bam_unpack_kernel   one 16-lane group per column, four columns per wave: SEQ, QUAL and the
//                       CIGAR ops into the pools, each lane writing aligned 16-byte chunks; the
//                       inserted bases of a long read's CIGARs are summed for the output bound.
// The passes are bandwidth-bound streaming; records are read bytewise (unaligned fields).
//
// With PR_BAM_RESTORE_SEQ (bam_core.h states the rule) three more kernels run, and the unpack
// kernel above is replaced by its twin; without it none of them is launched:
//   bam_donor_kernel    one lane per record of the whole stream: a record that may lend its SEQ
//                       goes into the donor table (open addressing in HBM, bam_table_insert).
//   bam_lookup_kernel   after the placement, one lane per column: a column without SEQ probes
//                       the table by its record's key, checks the lengths against its CIGAR and
//                       writes a_seq_src / a_hl / a_rc and a_lseq = q before the seq_off scan.  A
//                       missing donor or a length mismatch sets an error bit and leaves the lowest
//                       such record index (atomicMin) for the host's message.
//   bam_unpack_restore_kernel   bam_unpack_kernel with SEQ / QUAL read through a_seq_src.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "bam_core.h"
#include "bam_dev.h"

namespace prgpu {
namespace {

using namespace bam;

__global__ __launch_bounds__(256) void bam_field_kernel(BamDev D) {
    for (int64_t base = (int64_t)blockIdx.x * 256; base < D.n; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < D.n;
        int32_t rid = -1;
        bool keep = false;
        if (valid) {
            const uint8_t *rec = D.recs + D.off[i];
            const Fixed f = bam_fixed(rec);
            double score = 0.0;
            uint32_t fl = 0;
            int32_t text = 0;
            if (bam_aux_walk(bam_aux_at(rec, f), bam_end_of(rec, f), &score, &fl, &text) != BAM_OK) {
                atomicOr(D.err, BAM_E_AUX);
            } else if (fl & BAM_AS_TEXT) {
                D.text_list[atomicAdd(D.err + 1, 1)] = (int32_t)i;
            }
            fl |= bam_seq_flags(rec, f);
            rid = f.rid;
            if (!D.ref_to_lr) {
                keep = true;
            } else if (rid < -1 || rid >= D.n_ref) {
                atomicOr(D.err, BAM_E_RID);
            } else {
                keep = rid >= 0 && D.ref_to_lr[rid] >= 0;
            }
            D.f_score[i] = score;
            D.f_flags[i] = (uint8_t)fl;
            D.f_keep[i] = keep ? 1 : 0;
        }
        if (D.ref_to_lr) {
            // the wave's kept records of the first lane's reference: one add
            const bool k = valid && keep;
            const int32_t lead = __builtin_amdgcn_readfirstlane(rid);
            const unsigned long long same = __ballot(k && rid == lead);
            if (k && rid != lead) atomicAdd(D.cnt_ref + rid, 1ull);
            if (same && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)same) - 1)) atomicAdd(D.cnt_ref + lead, (unsigned long long)__popcll(same));
        }
    }
}

__global__ __launch_bounds__(256) void bam_place_kernel(BamDev D) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < D.n; i += (int64_t)gridDim.x * 256) {
        if (!D.f_keep[i]) continue;
        const uint8_t *rec = D.recs + D.off[i];
        const Fixed f = bam_fixed(rec);
        int64_t d = D.kidx[i];
        if (D.ref_to_lr) {
            if (d < D.ref_start[f.rid] || d >= D.ref_start[f.rid + 1]) {   // a record outside its reference's block
                atomicOr(D.err, BAM_E_ORDER);
                continue;
            }
            if (D.delta) d += D.delta[f.rid];
            if (D.f_flags[i] & PR_ALN_NO_SEQ) atomicOr(D.err, BAM_E_NOSEQ);
        }
        if (d < 0 || d >= D.n_kept) {
            atomicOr(D.err, BAM_E_ORDER);
            continue;
        }
        if (D.a_rid) D.a_rid[d] = f.rid;
        D.a_pos[d] = f.pos + 1;
        D.a_score[d] = D.f_score[i];
        D.a_flags[d] = D.f_flags[i] & (uint8_t)~BAM_AS_TEXT;
        D.a_lseq[d] = f.l_seq;
        D.a_ncig[d] = f.n_cigar;
        D.a_src[d] = i;
    }
}

__global__ __launch_bounds__(256) void bam_unpack_kernel(BamDev D) {
    const int lane = threadIdx.x & 15;
    for (int64_t d = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; d < D.n_kept; d += (int64_t)gridDim.x * 16) {
        const uint8_t *rec = D.recs + D.off[D.a_src[d]];
        const Fixed f = bam_fixed(rec);
        const int64_t so = D.seq_off[d];
        bam_unpack_seq(bam_seq_at(rec, f), f.l_seq, D.seq + so, lane, 16);
        if (D.qual) {
            const uint8_t *qb = bam_qual_at(rec, f);
            bam_unpack_qual(qb, f.l_seq, f.l_seq > 0 && qb[0] == 0xFF, D.qual + so, lane, 16);
        }
        long long ins = bam_copy_cigar(bam_cigar_at(rec, f), f.n_cigar, D.cig + D.cig_off[d], lane, 16);
        if (D.ins) {
            for (int m = 8; m; m >>= 1) ins += __shfl_xor(ins, m, 16);
            if (lane == 0 && ins) atomicAdd(D.ins + D.ref_to_lr[f.rid], (unsigned long long)ins);
        }
    }
}

__global__ __launch_bounds__(256) void bam_donor_kernel(BamDev D) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < D.n; i += (int64_t)gridDim.x * 256) {
        const uint8_t *rec = D.recs + D.off[i];
        const Fixed f = bam_fixed(rec);
        if (bam_is_donor(rec, f)) bam_table_insert(D.tab, D.tab_mask, D.recs, D.off, i, rec, f);
    }
}

__global__ __launch_bounds__(256) void bam_lookup_kernel(BamDev D) {
    for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < D.n_kept; d += (int64_t)gridDim.x * 256) {
        const int64_t i = D.a_src[d];
        int64_t src = i;
        int32_t hl = 0;
        uint8_t rc = 0;
        bool restored = false;
        if (D.a_flags[d] & PR_ALN_NO_SEQ) {
            const uint8_t *rec = D.recs + D.off[i];
            const Fixed f = bam_fixed(rec);
            const int64_t dn = bam_table_find(D.tab, D.tab_mask, D.recs, D.off, rec, f);
            if (dn < 0) {
                atomicOr(D.err, BAM_E_NODONOR);
                atomicMin(D.rst + 0, (unsigned long long)i);
            } else {
                const uint8_t *drec = D.recs + D.off[dn];
                const Fixed df = bam_fixed(drec);
                const CigarSpan sp = bam_cigar_span(rec, f);
                if (sp.hl + sp.q + sp.ht != (int64_t)df.l_seq) {
                    atomicOr(D.err, BAM_E_DONORLEN);
                    atomicMin(D.rst + 1, (unsigned long long)i);
                } else {
                    src = dn;
                    hl = (int32_t)sp.hl;
                    rc = ((bam_flag(rec) ^ bam_flag(drec)) & BAM_REVERSE) ? 1 : 0;
                    D.a_lseq[d] = (int32_t)sp.q;
                    D.a_flags[d] = (uint8_t)((D.a_flags[d] & ~PR_ALN_NO_SEQ) | bam_seq_flags(drec, df));
                    restored = true;
                }
            }
        }
        D.a_seq_src[d] = src;
        D.a_hl[d] = hl;
        D.a_rc[d] = rc;
        // the wave's restored columns: one add
        const unsigned long long m = __ballot(restored);
        if (restored && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(D.rst + 2, (unsigned long long)__popcll(m));
    }
}

__global__ __launch_bounds__(256) void bam_unpack_restore_kernel(BamDev D) {
    const int lane = threadIdx.x & 15;
    for (int64_t d = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; d < D.n_kept; d += (int64_t)gridDim.x * 16) {
        const int64_t i = D.a_src[d], si = D.a_seq_src[d];
        const uint8_t *rec = D.recs + D.off[i];
        const Fixed f = bam_fixed(rec);
        const int64_t so = D.seq_off[d];
        if (si == i) {
            bam_unpack_seq(bam_seq_at(rec, f), f.l_seq, D.seq + so, lane, 16);
            if (D.qual) {
                const uint8_t *qb = bam_qual_at(rec, f);
                bam_unpack_qual(qb, f.l_seq, f.l_seq > 0 && qb[0] == 0xFF, D.qual + so, lane, 16);
            }
        } else {
            const uint8_t *drec = D.recs + D.off[si];
            const Fixed df = bam_fixed(drec);
            const int32_t q = D.a_lseq[d], hl = D.a_hl[d];
            const bool rc = D.a_rc[d] != 0;
            bam_unpack_seq_from(bam_seq_at(drec, df), df.l_seq, hl, q, rc, D.seq + so, lane, 16);
            if (D.qual) {
                const uint8_t *qb = bam_qual_at(drec, df);
                bam_unpack_qual_from(qb, df.l_seq, hl, q, rc, qb[0] == 0xFF, D.qual + so, lane, 16);
            }
        }
        long long ins = bam_copy_cigar(bam_cigar_at(rec, f), f.n_cigar, D.cig + D.cig_off[d], lane, 16);
        if (D.ins) {
            for (int m = 8; m; m >>= 1) ins += __shfl_xor(ins, m, 16);
            if (lane == 0 && ins) atomicAdd(D.ins + D.ref_to_lr[f.rid], (unsigned long long)ins);
        }
    }
}

unsigned grid_for(int64_t items) {
    int64_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}   // namespace

size_t bam_scan_temp_bytes(int64_t n) {
    size_t tb = 0;
    (void)rocprim::exclusive_scan(nullptr, tb, (int32_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)(n + 1),
                                  rocprim::plus<int64_t>());
    return tb + 256;
}

int bam_field_pass(const BamDev &D, int64_t *kidx_out, void *temp, size_t temp_bytes, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bam_field_kernel, dim3(grid_for(D.n)), dim3(256), 0, s, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    size_t tb = temp_bytes;
    return (int)rocprim::exclusive_scan(temp, tb, D.f_keep, kidx_out, (int64_t)0, (size_t)(D.n + 1), rocprim::plus<int64_t>(), s);
}

int bam_place_pass(const BamDev &D, int64_t *seq_off_out, int64_t *cig_off_out, void *temp, size_t temp_bytes, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bam_place_kernel, dim3(grid_for(D.n)), dim3(256), 0, s, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    size_t tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, D.a_lseq, seq_off_out, (int64_t)0, (size_t)(D.n_kept + 1),
                                     rocprim::plus<int64_t>(), s)) != hipSuccess)
        return (int)e;
    tb = temp_bytes;
    return (int)rocprim::exclusive_scan(temp, tb, D.a_ncig, cig_off_out, (int64_t)0, (size_t)(D.n_kept + 1),
                                        rocprim::plus<int64_t>(), s);
}

int bam_donor_pass(const BamDev &D, void *stream) {
    if (D.n <= 0) return 0;
    hipLaunchKernelGGL(bam_donor_kernel, dim3(grid_for(D.n)), dim3(256), 0, (hipStream_t)stream, D);
    return (int)hipGetLastError();
}

int bam_place_restore_pass(const BamDev &D, int64_t *seq_off_out, int64_t *cig_off_out, void *temp, size_t temp_bytes, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bam_place_kernel, dim3(grid_for(D.n)), dim3(256), 0, s, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (D.n_kept > 0) {
        hipLaunchKernelGGL(bam_lookup_kernel, dim3(grid_for(D.n_kept)), dim3(256), 0, s, D);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    size_t tb = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, tb, D.a_lseq, seq_off_out, (int64_t)0, (size_t)(D.n_kept + 1),
                                     rocprim::plus<int64_t>(), s)) != hipSuccess)
        return (int)e;
    tb = temp_bytes;
    return (int)rocprim::exclusive_scan(temp, tb, D.a_ncig, cig_off_out, (int64_t)0, (size_t)(D.n_kept + 1),
                                        rocprim::plus<int64_t>(), s);
}

int bam_unpack_restore_pass(const BamDev &D, void *stream) {
    if (D.n_kept <= 0) return 0;
    hipLaunchKernelGGL(bam_unpack_restore_kernel, dim3(grid_for(D.n_kept * 16)), dim3(256), 0, (hipStream_t)stream, D);
    return (int)hipGetLastError();
}

int bam_unpack_pass(const BamDev &D, void *stream) {
    if (D.n_kept <= 0) return 0;
    hipLaunchKernelGGL(bam_unpack_kernel, dim3(grid_for(D.n_kept * 16)), dim3(256), 0, (hipStream_t)stream, D);
    return (int)hipGetLastError();
}

}   // namespace prgpu

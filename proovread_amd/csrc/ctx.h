// The library's one internal header: the private context (struct pr_ctx) and what the host files
// that share it need: the error string, HIPCHK, device buffers and their ids, host <-> device
// copies, and every function one host file calls in another, declared once with the file that
// defines it (those of the HIP-free files in err.h and bam_codec.h, which those files include
// too).  Included by every *_api.cpp and comm.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/prgpu.h"
#include "bam_codec.h"
#include "cns_plan.h"
#include "err.h"
#include "handoff_plan.h"
#include "sw_dev.h"
#include "seed_dev.h"

using namespace prgpu;

#define HIPCHK(x)                                                                        \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess)                                                            \
            return set_error(PR_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_));    \
    } while (0)

// device memory accounting behind pr_mem_stats, and the error of a failed hipMalloc (prgpu_api.cpp)
void prgpu_mem_note(const char *grp, int id, int64_t delta);
int prgpu_oom(const char *grp, int id, size_t want);

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    const char *grp = "buf";
    int id = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap && p) return 0;
        release();
        size_t want = bytes + 64;   // slack: kernels read whole dwords at the end of byte pools
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            return prgpu_oom(grp, id, want);
        }
        cap = want;
        prgpu_mem_note(grp, id, (int64_t)want);
        return 0;
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            prgpu_mem_note(grp, id, -(int64_t)cap);
        }
        p = nullptr;
        cap = 0;
    }
    // grow to `bytes` keeping the first `used` bytes (stream-ordered copy, then synchronised)
    int grow_keep(size_t bytes, size_t used, hipStream_t s) {
        if (bytes <= cap && p) return 0;
        void *np = nullptr;
        const size_t want = bytes + bytes / 4 + 64;
        if (hipMalloc(&np, want) != hipSuccess) return prgpu_oom(grp, id, want);
        if (p && used) {
            if (hipMemcpyAsync(np, p, used, hipMemcpyDeviceToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
                (void)hipFree(np);
                return set_error(PR_ERR_HIP, "device copy failed (%s[%d] growth)", grp, id);
            }
        }
        release();
        p = np;
        cap = want;
        prgpu_mem_note(grp, id, (int64_t)want);
        return 0;
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

// (the consensus buffers, CnsBufId: cns_plan.h)

// masking buffers (pr_mask_run inputs / outputs, pr_iter_mask output and run lists)
enum MaskBufId { MB_OFF, MB_SEQ, MB_QUAL, MB_OUT, MB_RUN_OFF, MB_RUNS, MB_TMP, MB_NRUNS, MB_ERR, MB_STATS, MB_COUNT };
// device seeding: the index copy (SI_*) and per-call buffers (SB_*)
enum SeedBufId {
    SI_TEXT, SI_CSTART, SI_CBLK, SI_LROFF, SI_KOFF, SI_KPOS, SI_KEXT, SI_CNT0,
    SB_SEQ = SI_CNT0 + 11, SB_OFF, SB_SCRATCH, SB_OUT, SB_NOUT, SB_STATUS, SB_NEXT, SB_PRE, SB_DENSE,
    SX_LRSEQ, SX_KEY0, SX_KEY1, SX_VAL0, SX_KC, SX_CNTPTR, SX_TEMP, SI_KSPLIT, SX_VAL1, SX_KCC, SX_KOFFC, SX_KCUR,
    SB_DP, SI_TEXT4, SB_ORDER, SI_BLKFR, SB_OCC, SD_COUNT
};
// the resident long-read set: pools, the dense offsets of a commit, the commit's staging pools
// (LS_RSEQ / LS_RQUAL: pr_lrset_snapshot's raw reads; LS_SRSAMP: pr_srset_sample's task sample)
enum LrSetBufId {
    LS_SEQ, LS_QUAL, LS_MAP, LS_OFF, LS_TSEQ, LS_TQUAL, LS_TMAP, LS_SRSEQ, LS_GSEQ, LS_GQUAL, LS_GMAP, LS_RSEQ, LS_RQUAL,
    LS_SRSAMP, LS_COUNT
};
// the exact-parity layout's exchange (pr_aln_exchange, owned batches): bounds, sort keys and
// indices, counts, op prefix, send / receive records and CIGAR ops, grouped hand-off inputs,
// the task's short reads
enum XchgBufId {
    XB_BOUNDS, XB_KEY0, XB_KEY1, XB_IDX0, XB_IDX1, XB_CNT, XB_OPIN, XB_OPAT, XB_SREC, XB_SCIG, XB_TEMP,
    XB_RREC, XB_RCIG, XB_RCIGAT, XB_GCNT, XB_GCNT64, XB_TASKOFF, XB_ERR, XB_GSR, XB_GSTATUS, XB_GPOS, XB_GSCORE,
    XB_GNCIG, XB_GCIGAT, XB_GSTRAND, XB_GPASS, XB_SR, XB_SROFF, XB_COUNT
};

// the hand-off: the tasks' per-read offsets, counts and error flags, the -b/-l filter's keep flags
// and scratch (PipeDev: keep, fsorted, fbin, fnc, flen, flst, flsti), the hand-off order, and the
// HBM sort of the big reads: their list, key offsets, key buffers
enum PipeBufId {
    PB_TASK_OFF, PB_CNT, PB_ERR, PB_F_KEEP, PB_F_SORTED, PB_F_BIN, PB_F_NC, PB_F_LEN, PB_F_LST, PB_F_LSTI,
    PB_ORDER, PB_BIG_LR, PB_BIG_OFF, PB_KEY0, PB_KEY1, PB_COUNT
};
static_assert(PB_ORDER == 10, "pr_mem_stats and PRGPU_MEM_TRACE report the index");

// the BAM export (pr_iter_export_bam): the FLAG column by SW task, the call's uploads (names, their
// offsets, qualities), per exported alignment its long read, grouped index, record size and offset,
// the scan's scratch, the record stream, the bytes of each read's records
enum BamEncBufId { EB_FLAG, EB_NAMES, EB_NAME_OFF, EB_QUAL, EB_LR, EB_J, EB_SIZE, EB_OFF, EB_TEMP, EB_OUT, EB_READ_BYTES, EB_COUNT };

// the SW stage's buffers (sw_api.cpp); from SWB_CHAIN on: bwa mode (aln_kernels.hip)
enum SwBufId {
    SWB_SR, SWB_SR_OFF, SWB_LR, SWB_LR_OFF, SWB_T_SR, SWB_T_LR, SWB_T_STRAND, SWB_T_QBEG, SWB_T_RBEG, SWB_T_SLEN,
    SWB_QB, SWB_QE, SWB_RB, SWB_RE, SWB_SCORE, SWB_TRUESC, SWB_W, SWB_PASS, SWB_GSCORE, SWB_POS, SWB_NCIG, SWB_STATUS,
    SWB_CIG, SWB_Z,
    SWB_CELLS,     // DP cell and cycle counters, the dequeue counter, the spill counters (sw_api.cpp: CELLS_*)
    SWB_PERM, SWB_BUCKET, SWB_X, SWB_XTRY, SWB_LIST,
    SWB_CIGSLOT,   // int64 [n+1] prefix of the per-task CIGAR slots
    SWB_CIGAT,     // int64 [n] first op of each task's CIGAR
    SWB_EHG,       // HBM DP rows of the general CIGAR kernel (long queries)
    SWB_CIGOFF,    // pr_sw_download compaction: prefix of ncigar
    SWB_CIGOUT,    //                            compacted ops
    SWB_CHAIN, SWB_SEEDOFF, SWB_SEL, SWB_EXTF, SWB_DEC, SWB_RESUME, SWB_ACNT, SWB_AREG, SWB_AIX, SWB_PSCORE, SWB_NPK,
    SWB_FDONE, SWB_PREQ, SWB_NOUT, SWB_OLIST, SWB_OFLAG, SWB_ATEMP, SWB_AOFF, SWB_ALIST, SWB_AFLAG, SWB_PPOOL, SWB_GLIST,
    SWB_GKEY0, SWB_GKEY1, SWB_GCNT, SWB_GLROFF, SWB_GPIPE, SWB_GDOWN, SWB_SCANIN, SWB_TLIST, SWB_CNEXT, SWB_HPREV, SWB_ABOX,
    SWB_RSNAP, SWB_KEYC,
    SWB_COUNT
};
static_assert(SWB_CELLS == 24 && SWB_CIGOUT == 34 && SWB_CHAIN == 35 && SWB_COUNT == 70,
              "pr_mem_stats and PRGPU_MEM_TRACE report the index");

// the resident SW batch (sw_api.cpp)
struct SwResident {
    bool loaded = false;
    bool launched = false;      // a single-seed launch ran on the resident batch (SWB_XTRY holds its flags)
    int64_t gen = 0;            // counts uploads and launches: what was derived from a launch names the gen it saw
    int64_t n_task = 0, n_sr = 0, n_lr = 0;
    int qmax = 0;
    DevBuf buf[SWB_COUNT];
    // bwa mode (pr_sw_batch.t_chain): the tasks are seeds, the outputs reported alignments
    bool bwa = false;
    int64_t read_id0 = 0;
    int64_t n_aln = 0;          // reported alignments of the last launch
    int ext_rounds = 0;         // extension rounds of the last launch (mem_chain2aln resumes)
    int64_t n_ext = 0;          // seeds extended
    int64_t n_rank0 = 0;        // first seeds of the chains (the first round)
    bool cnext_ready = false;   // cnext written by the device-seed unpack (seed ranks)
    int64_t n_big = 0;          // bwa mode: reads of more than ALN_WAVE_SEEDS seeds (the lane kernels')
    std::vector<int32_t> gcnt_host;   // bwa mode: reported alignments per long read of the last regrouping
    void *side = nullptr;       // hipStream_t: the early final pass beside the later extension rounds
    void *side_ev[3] = {nullptr, nullptr, nullptr};   // hipEvent_t
    int64_t n_patch = 0;        // mem_patch_reg global scores computed
    // bwa mode's bookkeeping kernels of the last launch (timing events, created on first use):
    // [0, 1] each round's walk, [2, 3] each late final pass, [4, 5] the early final pass (side
    // stream), [6, 7] its complement on the main stream
    void *bt_ev[8] = {};
    float ms_walk = 0.f, ms_final = 0.f, ms_final_early = 0.f;
    int64_t cig_slots = 0;      // ops in the slots (= first spill op)
    int64_t n_overflow = 0;     // tasks of the last launch whose CIGAR went to the spill area
    float ms_ext = 0.f, ms_glob = 0.f;
    unsigned long long cells[3] = {0, 0, 0};
    float ms_glob_ring = 0.f;
    SwEvPool ext_ev;
};
void sw_release(SwResident &r);   // sw_api.cpp

struct pr_ctx {
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev[11] = {};   // 0-7: SW, consensus, pipeline; 8-10: seeding
    // consensus resident batch
    DevBuf cb[CB_COUNT];
    bool cns_loaded = false;
    int32_t n_lr = 0;
    int64_t n_aln = 0, total_cols = 0, n_bins = 0, seq_cap = 0, chim_cap = 0;
    int64_t seed_pass2 = 0;   // reads of the last pr_seed_gpu_map that needed the large slices
    // reads the last pr_seed_gpu_map handed to pass 1b by lane, to pass 1b by wave, to pass 2 and
    // to the grown slices of the later passes (counted per pass): pr_seed_gpu_pass_reads
    int64_t seed_pass_reads[4] = {};
    std::vector<int64_t> seed_pre;   // per-read prefix of the last pr_seed_gpu_map's seeds (SB_DENSE)
    int64_t alg_bytes = 0;
    int64_t k_need = 0;   // per-read bound of kept alignments (K pool slices)
    bool has_ref = false, has_qual = false, has_ign = false;
    std::vector<int64_t> out_off, chim_off, bin_off, lr_off_host;
    float last_ms = 0.f;
    std::vector<int64_t> aln_off_host;   // the resident batch's alignment offsets (pr_cns_upload / pr_cns_upload_bam)
    float ms_bam = 0.f;                  // decode kernels of the last pr_cns_upload_bam / pr_bam_decode_alns_gpu
    // the BAM export of the resident iteration (bam_api.cpp)
    DevBuf eb[EB_COUNT];
    float ms_bam_enc = 0.f;              // encoder kernels of the last pr_iter_export_bam / _bytes
    int64_t iter_gen = 0;                // counts iteration uploads and launches: the export's uploads belong to one
    int64_t eb_gen = -1;                 // the iter_gen EB_FLAG / EB_NAMES / EB_NAME_OFF / EB_QUAL were filled for
    const void *eb_names_key = nullptr, *eb_qual_key = nullptr;   // and the host pools they were filled from
    std::vector<int64_t> eb_sr_off;      // the SW batch's short-read offsets on the host, of sw.gen eb_sr_gen
    int64_t eb_sr_gen = -1;
    // SW -> consensus pipeline (pr_iter_*)
    bool pipe = false;
    bool pipe_ref_ascii = false;   // pr_iter_batch.ref_seq given: consensus reference in CB_REF_SEQ
    int pipe_sort_cap = 0;
    DevBuf pb[PB_COUNT];
    handp::Plan ho;              // the hand-off's sort plan (explicit tasks: at upload; bwa mode: at launch)
    bool ho_done = false;        // a hand-off ran on this batch (pr_iter_handoff_stats / _order)
    int64_t ho_sw_gen = -1;      // ... over the SW launch of this sw.gen (the BAM export reads both)
    std::vector<int32_t> own_cnt_host;   // owned batch: received alignments per long read
    float ms_pipe = 0.f, ms_cns = 0.f;
    // SW resident batch
    SwResident sw;
    // masking
    DevBuf mb[MB_COUNT];
    // seeding
    DevBuf sd[SD_COUNT];
    bool seed_loaded = false;
    seedc::IndexView seed_view{};
    float ms_seed = 0.f, ms_seed_pass2 = 0.f;
    float ms_index = 0.f;
    float ms_siam = 0.f;   // kernels of the last pr_siam_* call
    float ms_ccs = 0.f;    // kernels of the last pr_ccs_* call
    float ms_utg = 0.f;    // kernels of the last pr_utg_run
    float ms_utg_k[5] = {};   // ... by kernel: prep, coverage, contained filter, consensus, pack
    int64_t seed_n_text = 0, seed_n_hits = 0;
    int64_t seed_sr_bases = -1;   // bases of the short reads of the last pr_seed_gpu_map (SB_SEQ)
    bool iter_masked = false;
    bool cns_launched = false;   // a consensus launch filled the CB_O_* outputs
    bool cns_gathered = false;   // the hand-off's SEQ / CIGAR offsets point into CB_SEQ / CB_CIG
    // exact-parity layout: received alignments (pr_aln_exchange) and an owned batch
    DevBuf xb[XB_COUNT];
    bool x_ready = false;        // XB_RREC / XB_RCIG hold the last exchange's records
    bool x_pass = false;         // world 1: the exchange is the identity, the owned launch reads the SW output
    int64_t x_nrecv = 0, x_nrcig = 0;
    std::vector<int64_t> x_from;  // records of the last exchange by source rank
    // the resident long-read set (pr_lrset_*): reads, qualities, mapping reference (masked reads)
    DevBuf ls[LS_COUNT];
    std::vector<int64_t> ls_off;
    int32_t ls_n = -1;
    bool ls_map_is_reads = true;
    std::vector<int64_t> ss_off;   // the resident short reads (pr_srset_load): offsets on the host
    std::vector<int64_t> ss_samp_off;   // pr_srset_sample's task sample (LS_SRSAMP), empty: none
    std::vector<int64_t> ls_raw_off;    // pr_lrset_snapshot's offsets, empty: none
    bool own = false;            // the resident iteration batch is an owned batch (pr_iter_upload_owned)
    bool own_ref_nt4 = false;    // its consensus reference is the SW long-read pool's slice (nt4)
    bool own_sr_resident = false;   // its short reads are the resident ones (LS_SRSEQ)
    int32_t own_lr0 = 0;
};

template <class T>
static int upload(DevBuf &d, const T *h, size_t n, hipStream_t s) {
    int rc = d.ensure(n * sizeof(T));
    if (rc) return rc;
    if (n && h) HIPCHK(hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, s));
    return 0;
}

template <class T>
static int download(T *h, const DevBuf &d, size_t n, hipStream_t s, size_t first = 0) {   // elements [first, first + n)
    if (h && n) HIPCHK(hipMemcpyAsync(h, d.as<T>() + first, n * sizeof(T), hipMemcpyDeviceToHost, s));
    return 0;
}

// ---------------------------------------------------------------------------
// functions one host file calls in another, by the file that defines them
namespace prgpu {
struct XchgSend;
}

// cns_api.cpp: the two halves of pr_cns_upload that pr_cns_upload_bam shares: the long-read part
// of a batch, and the scratch / output buffers once the alignment columns and bounds are set;
// the buffers of the given cnsp::Group mask sized for the context's n_lr, n_aln, seq_cap, chim_cap
int cns_upload_long_reads(pr_ctx *c, const pr_cns_batch *b);
int cns_alloc_resident(pr_ctx *c);
int cns_ensure(pr_ctx *c, unsigned groups);

// iter_api.cpp: the iteration batch's upload; dev_*: device sources in place of the batch's host
// pools (the resident long-read set and the seeding's copies: pr_iter_upload_lrset)
int iter_upload(pr_ctx *c, const pr_iter_batch *b, bool gpu_seeds, const uint8_t *dev_sr = nullptr,
                const uint8_t *dev_lr = nullptr, const uint8_t *dev_ref = nullptr, const uint8_t *dev_qual = nullptr);

// xchg_api.cpp: an owned batch's received records regrouped by long read into the hand-off's
// inputs (pr_iter_launch)
int own_group(pr_ctx *c, SwPtrs *sp);

// mask_api.cpp: the masking's capacity flag (syncs)
int mask_check_err(pr_ctx *c);

// seed_api.cpp: the seed index built in HBM; lr_dev: lr_seq is a device pointer (pr_lrset_index)
int index_build(pr_ctx *c, const uint8_t *lr_seq, const int64_t *lr_off, int n_lr, bool lr_dev);

// sw_api.cpp: device pointers of the resident SW batch (regroup: bwa mode's alignments grouped by
// long read), the sender's view of its reported alignments, the SW upload with the device-resident
// seeds of pr_seed_gpu_map, the -b/-l survivors from grouped into SAM order
int sw_get_ptrs(pr_ctx *c, SwPtrs *p);
int sw_get_pipe_ptrs(pr_ctx *c, SwPtrs *p, bool regroup);
int sw_xchg_send(pr_ctx *c, XchgSend *X);
int sw_upload_device_seeds(pr_ctx *c, const pr_sw_batch *b, const pr_seed_task *dev_tasks, const int64_t *seed_off_h,
                           const uint8_t *dev_sr = nullptr, const uint8_t *dev_lr = nullptr);
int sw_keep_to_sam(pr_ctx *c, const uint8_t *keep_grouped, uint8_t *keep_sam);

// comm.cpp: the context a communicator was made on
pr_ctx *comm_ctx(pr_comm *c);

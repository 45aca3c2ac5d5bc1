"""The BAM export of a task's alignments timed against the host chain it replaces:
a tenth of configs[1]'s bwa-sr-1 sample (the data of tools/time_bam_decode.py) staged as GpuStages
stages the task, the iteration left resident.

  (a)  the host chain on the resident launch: pr_sw_binfilter + pr_sw_sam + pr_sam_encode +
       pr_bam_sort_records, 16 threads each
  (b)  pr_iter_export_bam, wall clock, the names and qualities uploaded by the call
  (b2) the same with the pools already resident (a task's second and later ranges)
  (b') its kernels alone (pr_bam_export_last_ms)

One warm-up, then the median of REPEATS runs each.  The kernels' share of the HBM bandwidth is
(bytes read + bytes written) / kernel time over 8 TB/s, with the byte count written out below.

    python tools/time_bam_export.py [out.json]
"""
import ctypes as C
import json
import statistics
import struct
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REPEATS = 7
THREADS = 16
HBM_BYTES_PER_S = 8.0e12


def median_ms(fn):
    fn()
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 3), [round(x, 3) for x in t]


def main():
    from proovread_amd import _abi, bamio, bwa_proovread as bp, cns, correct, iteration, synth
    from proovread_amd import tasks as T
    gl, n_lr = 460_000, 1_380
    d = synth.simulate_reads(20261015 + 2, gl, n_lr, 10_000, int(round(15.0 * gl / 150)), threads=THREADS)
    asc = np.frombuffer(b"ACGTN", np.uint8)
    n_sr = len(d.sr_off) - 1
    ids = [f"lr{i}" for i in range(n_lr)]
    lr_off = np.ascontiguousarray(d.lr_off, np.int64)
    stages = correct.GpuStages()
    stages.load(correct.LongReads(ids, pools=(asc[d.lr_seq], lr_off, np.full(len(d.lr_seq), ord("5"), np.uint8))))
    sr_pool, sr_off = np.ascontiguousarray(d.sr_seq, np.uint8), np.ascontiguousarray(d.sr_off, np.int64)
    stages.load_short_reads(correct.ShortReads.from_pool(sr_pool, sr_off))
    task = "bwa-sr-1"
    cov = T.sr_coverage(task)
    binf = (20, 20 * cov)
    stages.task(task, None, sr_off, cns.CnsParams(coverage=cov * 0.75, max_ins_length=0), binf, None, False,
                (T.hcr_mask(task), 150), sr_ranges=np.array([[0, n_sr]], np.int64), dry=True)
    it = stages.last_iteration
    ctx = stages.ctx
    L = _abi.lib()
    bamio._codec()
    names, name_off = bp._name_pool([f"sr{i}" for i in range(n_sr)])
    sr_text = np.append(asc[sr_pool], np.uint8(0))
    quals = [np.full(len(sr_text), ord("I"), np.uint8) for _ in range(2)]
    lrn, lrn_off = bp._name_pool(ids)
    ref_arr = (C.c_char_p * n_lr)(*[n.encode() for n in ids])
    L.pr_sw_binfilter.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_void_p]
    L.pr_sw_sam.argtypes = [C.c_void_p, C.POINTER(bp.SamIn), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pr_sam_encode.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_char_p), C.c_int32, C.c_int, C.POINTER(C.c_void_p),
                                C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pr_bam_sort_records.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64)]
    n_aln = C.c_int64()
    _abi.check(L.pr_sw_aln_count(ctx.h, C.byref(n_aln)), "pr_sw_aln_count")
    keep = np.zeros(max(1, n_aln.value), np.uint8)
    got = {}

    def host_chain():
        _abi.check(L.pr_sw_binfilter(ctx.h, binf[0], float(binf[1]), keep.ctypes.data), "pr_sw_binfilter")
        si = bp.SamIn(sr_off.ctypes.data, sr_text.ctypes.data, quals[0].ctypes.data, names.ctypes.data, name_off.ctypes.data,
                      lrn.ctypes.data, lrn_off.ctypes.data, keep.ctypes.data, THREADS)
        txt, tl, nr = C.c_void_p(), C.c_int64(), C.c_int64()
        _abi.check(L.pr_sw_sam(ctx.h, C.byref(si), C.byref(txt), C.byref(tl), C.byref(nr)), "pr_sw_sam")
        enc, el, er = C.c_void_p(), C.c_int64(), C.c_int64()
        rc = L.pr_sam_encode(txt, tl.value, ref_arr, n_lr, THREADS, C.byref(enc), C.byref(el), C.byref(er))
        L.pr_buffer_free(txt)
        _abi.check(rc, "pr_sam_encode")
        srt, sl, sn = C.c_void_p(), C.c_int64(), C.c_int64()
        rc = L.pr_bam_sort_records(enc, el.value, THREADS, C.byref(srt), C.byref(sl), C.byref(sn))
        L.pr_buffer_free(enc)
        _abi.check(rc, "pr_bam_sort_records")
        got["host"] = bytes(memoryview((C.c_ubyte * sl.value).from_address(srt.value)))
        L.pr_buffer_free(srt)
        got.update(sam_bytes=tl.value, records=sn.value)

    kernel_ms, turn = [], [0]

    def export_with_upload():
        turn[0] ^= 1   # another quality pool every call: the call uploads the pools again
        got["dev"] = it.export_bam(names, name_off, quals[turn[0]])
        kernel_ms.append(it.export_ms())

    def export_resident():
        got["dev"] = it.export_bam(names, name_off, quals[turn[0]])

    a_ms, a_all = median_ms(host_chain)
    b_ms, b_all = median_ms(export_with_upload)
    b2_ms, b2_all = median_ms(export_resident)
    assert got["dev"] == got["host"], "the export differs from the host chain"
    body = got["dev"]
    n, o, name_bytes, ops, bases = 0, 0, 0, 0, 0
    while o < len(body):
        bs, = struct.unpack_from("<i", body, o)
        name_bytes += body[o + 12] - 1
        ops += struct.unpack_from("<H", body, o + 16)[0]
        bases += struct.unpack_from("<i", body, o + 20)[0]
        o += 4 + bs
        n += 1
    k_ms = statistics.median(kernel_ms[1:])
    # FLAG scatter: 8 bytes in and 2 out per alignment of the final pass.  Size pass: a_task, t_sr, two name
    # offsets, n_cigar, l_seq, score in (44), long read, grouped index and size out (16).  Scan: 8 in, 8 out
    # and as much scratch (24).  Write pass: the record's descriptors (grouped index, long read, offset,
    # short read, two sr_off, two name offsets, POS, score, n_cigar, l_seq, task, FLAG, strand, CIGAR start:
    # 87), its name, CIGAR ops, bases and qualities in, the record out.
    moved = n_aln.value * 10 + n * (44 + 16 + 24 + 87) + name_bytes + 4 * ops + 2 * bases + len(body)
    rec = {"records": n, "reported_before_filter": int(n_aln.value), "long_reads": n_lr, "short_reads": n_sr,
           "bam_body_bytes": len(body), "sam_text_bytes": got["sam_bytes"],
           "names_and_quals_uploaded_bytes": int(name_off[-1]) + int(sr_off[-1]),
           "a_host_chain_ms": a_ms, "b_export_wall_with_upload_ms": b_ms, "b2_export_wall_pools_resident_ms": b2_ms,
           "b_export_kernels_ms": round(k_ms, 3), "kernel_bytes_moved": moved,
           "kernel_hbm_fraction": round(moved / (k_ms * 1e-3) / HBM_BYTES_PER_S, 4),
           "runs_ms": {"a": a_all, "b": b_all, "b2": b2_all, "b_kernels": [round(x, 3) for x in kernel_ms[1:]]}}
    print(json.dumps(rec, indent=1))
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""The sam / bam modes' decode step timed on one BAM of about a million records:
a tenth of configs[1]'s bwa-sr-1 sample mapped with the bwa-proovread drop-in (as
tools/time_mem_dropin.py builds the whole sample), its SAM encoded and coordinate-sorted.

  (a) the host path bam2cns takes: pr_bam_decode_alns at 16 threads + pack_bam_chunk + pr_cns_upload
  (b) pr_cns_upload_bam: wall clock, and the decode kernels alone (pr_bam_decode_last_ms)
  (c) the consensus launch on the resident batch

One warm-up, then the median of REPEATS runs each.  The kernels' share of the HBM bandwidth is
(bytes read + bytes written) / kernel time over 8 TB/s, with the byte count written out below.

    python tools/time_bam_decode.py [out.json]

--restore times PR_BAM_RESTORE_SEQ instead: every third secondary line of the
mapping loses its SEQ and QUAL (`*`), a third of all records.  (on) pr_cns_upload_bam_opts with
the option on that stream; (off) pr_cns_upload_bam on the mapping as it is, whose secondary lines
carry what the option restores.  Both decode kernel times are pr_bam_decode_last_ms.

    python tools/time_bam_decode.py --restore [out.json]
"""
import ctypes as C
import io
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REPEATS = 7
HBM_BYTES_PER_S = 8.0e12


def median_ms(fn):
    fn()
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 3), [round(x, 3) for x in t]


def strip_secondaries(sam_text: str):
    """(lines with `*` on every third secondary line, the lines as mapped).  The drop-in prints
    the read's SEQ / QUAL on its secondary lines, in the line's orientation and without hard
    clips: what the option restores from the primary line, so the mapping itself is the restored
    stream.  About twenty of twenty-one records of this mapping are secondary lines."""
    star, full = [], []
    k = 0
    rows = [ln.split("\t") for ln in sam_text.split("\n") if ln and not ln.startswith("@")]
    # (the drop-in's bin filter can drop a read's primary line and leave secondary ones: those keep their SEQ)
    donors = {(f[0], int(f[1]) & 0xC0) for f in rows if not int(f[1]) & 0x904 and f[9] != "*" and "H" not in f[5]}
    for f in rows:
        ln = "\t".join(f)
        full.append(ln)
        if int(f[1]) & 0x100 and not int(f[1]) & 0x4 and f[9] != "*" and (f[0], int(f[1]) & 0xC0) in donors:
            k += 1
            if k % 3 == 0:
                ln = "\t".join(f[:9] + ["*", "*"] + f[11:])
        star.append(ln)
    return star, full


def time_restore(argv, sam_text, names, reads, n_lr):
    from proovread_amd import _abi, bamio, cns
    star, full = strip_secondaries(sam_text)
    n_sec = sum(1 for ln in star if ln.split("\t")[9] == "*")
    bodies = {k: bamio._native_sort(bamio._native_encode("".join(x + "\n" for x in v), names))
              for k, v in (("on", star), ("off", full))}
    ctx = _abi.default_context()
    L = _abi.lib()
    dr = cns.pack_reads(reads)
    r2l = np.arange(n_lr, dtype=np.int32)
    cb = _abi.CnsBatch()
    cb.n_lr = n_lr
    cb.lr_off = _abi.ptr(dr["lr_off"], C.c_int64)
    cb.ref_seq = _abi.ptr(dr["ref_seq"], C.c_uint8)
    cb.ref_qual = _abi.ptr(dr["ref_qual"], C.c_uint8)
    kernel_ms = {"on": [], "off": []}
    info = {}

    def run(which):
        body = bodies[which]
        nk, nr = C.c_int64(), C.c_int64()
        if which == "on":
            _abi.check(L.pr_cns_upload_bam_opts(ctx.h, C.byref(cb), body, len(body), _abi.ptr(r2l, C.c_int32), n_lr,
                                                _abi.PR_BAM_RESTORE_SEQ, C.byref(nk), C.byref(nr)), "pr_cns_upload_bam_opts")
            info["restored"] = int(nr.value)
        else:
            _abi.check(L.pr_cns_upload_bam(ctx.h, C.byref(cb), body, len(body), _abi.ptr(r2l, C.c_int32), n_lr, C.byref(nk)),
                       "pr_cns_upload_bam")
        ms = C.c_double()
        _abi.check(L.pr_bam_decode_last_ms(ctx.h, C.byref(ms)), "pr_bam_decode_last_ms")
        kernel_ms[which].append(ms.value)
        info["kept_" + which] = int(nk.value)

    on_ms, on_all = median_ms(lambda: run("on"))
    off_ms, off_all = median_ms(lambda: run("off"))
    rec = {"records": len(star), "secondaries_without_seq": n_sec, "restored": info["restored"], "kept_on": info["kept_on"],
           "kept_off": info["kept_off"], "long_reads": n_lr, "bam_body_bytes_on": len(bodies["on"]),
           "bam_body_bytes_off": len(bodies["off"]),
           "decode_kernels_ms_restore_on": round(statistics.median(kernel_ms["on"][1:]), 3),
           "decode_kernels_ms_restore_off_restored_stream": round(statistics.median(kernel_ms["off"][1:]), 3),
           "upload_bam_wall_ms_restore_on": on_ms, "upload_bam_wall_ms_restore_off_restored_stream": off_ms,
           "runs_ms": {"on": on_all, "off": off_all, "on_kernels": [round(x, 3) for x in kernel_ms["on"][1:]],
                       "off_kernels": [round(x, 3) for x in kernel_ms["off"][1:]]}}
    print(json.dumps(rec, indent=1))
    if argv:
        Path(argv[0]).parent.mkdir(parents=True, exist_ok=True)
        Path(argv[0]).write_text(json.dumps(rec, indent=1) + "\n")


def main():
    from proovread_amd import _abi, bam2cns, bamio, bwa_proovread, cns, synth
    from proovread_amd import tasks as T
    argv = [a for a in sys.argv[1:] if a != "--restore"]
    restore = "--restore" in sys.argv[1:]
    gl, n_lr = 460_000, 1_380
    d = synth.simulate_reads(20261015 + 2, gl, n_lr, 10_000, int(round(15.0 * gl / 150)), threads=16)
    asc = np.frombuffer(b"ACGTN", np.uint8)
    lr = [asc[d.lr_seq[d.lr_off[i]:d.lr_off[i + 1]]].tobytes().decode() for i in range(n_lr)]
    names = [f"lr{i}" for i in range(n_lr)]
    with tempfile.TemporaryDirectory(prefix="bamdec_") as td:
        lr_fa, sr_fq = Path(td) / "lr.fa", Path(td) / "sr.fq"
        lr_fa.write_text("".join(f">{n}\n{s}\n" for n, s in zip(names, lr)))
        with open(sr_fq, "wb") as fh:
            for i in range(len(d.sr_off) - 1):
                s = asc[d.sr_seq[d.sr_off[i]:d.sr_off[i + 1]]].tobytes()
                fh.write(b"@sr%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
        out = io.StringIO()
        rc = bwa_proovread.mem(["-b", "20", "-l", "300"] + T.bwa_argv("bwa-sr-1") + ["-t", "16", str(lr_fa), str(sr_fq)],
                               out=out, log=io.StringIO())
        assert rc == 0
    reads = [cns.LongRead(n, s, "5" * len(s)) for n, s in zip(names, lr)]
    if restore:
        return time_restore(argv, out.getvalue(), names, reads, n_lr)
    body = bamio._native_sort(bamio._native_encode(out.getvalue(), names))
    del out
    ctx = _abi.default_context()
    L = _abi.lib()
    L.pr_bam_decode_alns.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.POINTER(bam2cns._BamAlns)]
    L.pr_bam_alns_free.argtypes = [C.POINTER(bam2cns._BamAlns)]
    L.pr_bam_alns_free.restype = None
    L.pr_ctx_sync.argtypes = [C.c_void_p]
    dr = cns.pack_reads(reads)
    info = {}

    def host_path():
        a = bam2cns._BamAlns()
        _abi.check(L.pr_bam_decode_alns(body, len(body), 16, C.byref(a)), "pr_bam_decode_alns")
        try:
            def take(p, ct, n):
                return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(max(n, 1),))[:n].copy()
            n = a.n
            cols = {"rid": take(a.rid, C.c_int32, n), "pos1": take(a.pos1, C.c_int32, n),
                    "score": take(a.score, C.c_double, n), "flags": take(a.flags, C.c_uint8, n),
                    "seq_off": take(a.seq_off, C.c_int64, n), "lseq": take(a.lseq, C.c_int32, n),
                    "cig_off": take(a.cig_off, C.c_int64, n), "ncig": take(a.ncig, C.c_int32, n),
                    "seq": take(a.seq, C.c_uint8, a.seq_len), "qual": take(a.qual, C.c_uint8, a.seq_len),
                    "cig": take(a.cig, C.c_uint32, a.cig_len)}
            info.update(records=int(n), seq_bytes=int(a.seq_len), cigar_ops=int(a.cig_len))
        finally:
            L.pr_bam_alns_free(C.byref(a))
        batch = bam2cns.pack_bam_chunk(reads, names, cols)
        cb = cns.make_c_batch(batch)
        _abi.check(L.pr_cns_upload(ctx.h, C.byref(cb)), "pr_cns_upload")

    r2l = np.arange(n_lr, dtype=np.int32)
    cb = _abi.CnsBatch()
    cb.n_lr = n_lr
    cb.lr_off = _abi.ptr(dr["lr_off"], C.c_int64)
    cb.ref_seq = _abi.ptr(dr["ref_seq"], C.c_uint8)
    cb.ref_qual = _abi.ptr(dr["ref_qual"], C.c_uint8)
    kernel_ms = []

    def device_path():
        nk = C.c_int64()
        _abi.check(L.pr_cns_upload_bam(ctx.h, C.byref(cb), body, len(body), _abi.ptr(r2l, C.c_int32), n_lr, C.byref(nk)),
                   "pr_cns_upload_bam")
        ms = C.c_double()
        _abi.check(L.pr_bam_decode_last_ms(ctx.h, C.byref(ms)), "pr_bam_decode_last_ms")
        kernel_ms.append(ms.value)
        info["kept"] = int(nk.value)

    params = cns.CnsParams(coverage=11.25, detect_chimera=False, max_ins_length=0).to_c()

    def consensus():
        _abi.check(L.pr_cns_launch(ctx.h, C.byref(params)), "pr_cns_launch")
        _abi.check(L.pr_ctx_sync(ctx.h), "pr_ctx_sync")

    a_ms, a_all = median_ms(host_path)
    b_ms, b_all = median_ms(device_path)
    c_ms, c_all = median_ms(consensus)
    k_ms = statistics.median(kernel_ms[1:])
    n = info["records"]
    # field pass: the records once, 13 bytes of columns and flags out; placement: 36 bytes of every
    # record, 41 bytes of columns both ways; unpack: the records again, SEQ + CIGAR pools out;
    # scans: 12 bytes per element, three of them
    moved = 2 * len(body) + n * (8 + 13 + 36 + 8 + 2 * 41 + 8 + 3 * 12) + info["seq_bytes"] + 4 * info["cigar_ops"]
    rec = {"records": n, "kept": info["kept"], "long_reads": n_lr, "bam_body_bytes": len(body),
           "a_host_decode_pack_upload_ms": a_ms, "b_upload_bam_wall_ms": b_ms, "b_decode_kernels_ms": round(k_ms, 3),
           "c_consensus_launch_ms": c_ms, "kernel_bytes_moved": moved,
           "kernel_hbm_fraction": round(moved / (k_ms * 1e-3) / HBM_BYTES_PER_S, 4),
           "runs_ms": {"a": a_all, "b": b_all, "b_kernels": [round(x, 3) for x in kernel_ms[1:]], "c": c_all}}
    print(json.dumps(rec, indent=1))
    if argv:
        Path(argv[0]).parent.mkdir(parents=True, exist_ok=True)
        Path(argv[0]).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

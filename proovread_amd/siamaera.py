"""`siamaera`: detect and trim reverse-complement self-chimeras (bin/siamaera).

proovread pipes the trimmed reads through siamaera before it writes PRE.trimmed.fq
(proovread.cfg:159, bin/proovread:923-933).  A siamaera is an unsplit PacBio subread
`--R-->--J--<--R.rc--`; the reference finds it with two `blastn -strand minus` calls of the
read against itself and cuts the read down to one arm (siamaera:250-474).

Here the self-alignments come from libprgpu.so (pr_siam_*, include/prgpu.h): exact seeds
extended by ksw_extend2 with identity counts, one wave per read on the GPU
(csrc/siam_kernels.hip) or threads on the host.  blastn's heuristics are not restated:
parity with the reference is unpinned; the decision from the alignments
(siamaera:277-448) and the record editing are restated line by line.

    siamaera [options] < in.fa/fq > out.fa/fq
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .seqfilter import Record, format_record

VERSION = "0.01"   # siamaera:108

KEEP, TRIM, DROP = 0, 1, 2
SEED_OVERFLOW, HSP_OVERFLOW, TOO_LONG = 1, 2, 4
MAX_SEEDS, MAX_HSPS, MAX_LEN = 1024, 64, 131072


class Aligner(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("a", "b", "o", "e", "w", "zdrop", "word")]


class Params(C.Structure):
    _fields_ = [("seq_min_len", C.c_int32), ("term_ignore_len", C.c_int32), ("trim", C.c_int32),
                ("filter_inconclusive", C.c_int32), ("aln_min_idy", C.c_double), ("pass1", Aligner), ("pass2", Aligner)]


class Hsp(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("read", "qas", "qae", "sas", "sae", "length", "matches", "score")]


class Decision(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("action", "frm", "to")]


HspTuple = Tuple[int, int, int, int, int, int, int]   # qas, qae, sas, sae, length, matches, score

_set = False


def _lib():
    global _set
    L = _abi.lib()
    if not _set:
        PH = C.POINTER(C.POINTER(Hsp))
        L.pr_siam_params_default.argtypes = [C.POINTER(Params)]
        L.pr_siam_params_default.restype = None
        L.pr_siam_hsps_host.argtypes = [C.POINTER(Aligner), C.c_double, _abi.PU8, _abi.P64, C.c_int32, C.c_int, PH,
                                        _abi.P64, _abi.P32]
        L.pr_siam_hsps_gpu.argtypes = [C.c_void_p, C.POINTER(Aligner), C.c_double, _abi.PU8, _abi.P64, C.c_int32, PH,
                                       _abi.P64, _abi.P32]
        L.pr_siam_decide.argtypes = [C.POINTER(Params), C.c_int32, C.POINTER(Hsp), C.c_int32, C.POINTER(Hsp), C.c_int32,
                                     C.POINTER(Decision), _abi.P32]
        L.pr_siam_run.argtypes = [C.c_void_p, C.POINTER(Params), _abi.PU8, _abi.P64, C.c_int32, C.c_int,
                                  C.POINTER(Decision), _abi.P32, _abi.P64]
        L.pr_siam_last_ms.argtypes = [C.c_void_p, _abi.PD]
        L.pr_siam_seeds_host.argtypes = [_abi.PU8, C.c_int32, C.c_int32, _abi.P32, C.c_int32, _abi.P32]
        L.pr_siam_extend_host.argtypes = [C.POINTER(Aligner), _abi.PU8, C.c_int32, _abi.PU8, C.c_int32, C.c_int32,
                                          _abi.P32]
        L.pr_siam_extend_gpu.argtypes = [C.c_void_p, C.POINTER(Aligner), _abi.PU8, _abi.P64, _abi.PU8, _abi.P64,
                                         _abi.P32, C.c_int32, _abi.P32]
        _set = True
    return L


def default_params(**over) -> Params:
    """siamaera:123-134 and the two blastn option sets (:503-516, :551-561)."""
    p = Params()
    _lib().pr_siam_params_default(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


_NT4 = np.full(256, 4, np.uint8)
for _k, _c in enumerate(b"ACGT"):
    _NT4[_c] = _NT4[_c + 32] = _k


def nt4(seq: bytes) -> np.ndarray:
    """ASCII bases -> nt4 codes (A C G T in either case 0..3, anything else 4)."""
    return _NT4[np.frombuffer(bytes(seq), np.uint8)]


def _batch(seqs: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(seqs) + 1, np.int64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs])
    pool = nt4(b"".join(bytes(s) for s in seqs)) if len(seqs) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(pool), off


def _ctx(device: bool, ctx):
    if not device:
        return None
    return ctx or _abi.default_context()


def hsps(seqs: Sequence[bytes], aligner: Optional[Aligner] = None, min_idy: Optional[float] = None,
         device: bool = True, ctx=None, threads: int = 0) -> Tuple[List[List[HspTuple]], np.ndarray]:
    """One blastn call per read (pass 1's options by default): per read the kept alignments
    (qas, qae, sas, sae, length, matches, score) in order of production, and the per-read
    status flags."""
    L = _lib()
    p = default_params()
    al = aligner or p.pass1
    idy = p.aln_min_idy if min_idy is None else min_idy
    pool, off = _batch(seqs)
    n = len(seqs)
    status = np.zeros(max(n, 1), np.int32)
    out, cnt = C.POINTER(Hsp)(), C.c_int64()
    c = _ctx(device, ctx)
    if c is None:
        rc = L.pr_siam_hsps_host(C.byref(al), idy, _abi.ptr(pool, C.c_uint8), _abi.ptr(off, C.c_int64), n, threads,
                                 C.byref(out), C.byref(cnt), _abi.ptr(status, C.c_int32))
    else:
        rc = L.pr_siam_hsps_gpu(c.h, C.byref(al), idy, _abi.ptr(pool, C.c_uint8), _abi.ptr(off, C.c_int64), n,
                                C.byref(out), C.byref(cnt), _abi.ptr(status, C.c_int32))
    _abi.check(rc, "pr_siam_hsps")
    res: List[List[HspTuple]] = [[] for _ in range(n)]
    for k in range(cnt.value):
        h = out[k]
        res[h.read].append((h.qas, h.qae, h.sas, h.sae, h.length, h.matches, h.score))
    return res, status[:n]


def run(seqs: Sequence[bytes], params: Optional[Params] = None, device: bool = True, ctx=None, threads: int = 0):
    """siamaera's per-read decision for a batch -> (decisions [n, 3] = action, from, to;
    status [n]; summary dict with scanned / trimmed / inconclusive / flagged and, on the
    device, kernel_ms)."""
    L = _lib()
    p = params or default_params()
    pool, off = _batch(seqs)
    n = len(seqs)
    dec = np.zeros((max(n, 1), 3), np.int32)
    status = np.zeros(max(n, 1), np.int32)
    summ = np.zeros(4, np.int64)
    c = _ctx(device, ctx)
    rc = L.pr_siam_run(c.h if c is not None else None, C.byref(p), _abi.ptr(pool, C.c_uint8), _abi.ptr(off, C.c_int64),
                       n, threads, dec.ctypes.data_as(C.POINTER(Decision)), _abi.ptr(status, C.c_int32),
                       _abi.ptr(summ, C.c_int64))
    _abi.check(rc, "pr_siam_run")
    summary = dict(zip(("scanned", "trimmed", "inconclusive", "flagged"), (int(x) for x in summ)))
    if c is not None:
        ms = C.c_double()
        _abi.check(L.pr_siam_last_ms(c.h, C.byref(ms)), "pr_siam_last_ms")
        summary["kernel_ms"] = ms.value
    return dec[:n], status[:n], summary


def _hsp_array(hs: Sequence[Sequence[int]]):
    arr = (Hsp * max(len(hs), 1))()
    for k, h in enumerate(hs):
        arr[k] = Hsp(0, *[int(x) for x in h[:4]], *([int(x) for x in h[4:7]] if len(h) >= 7 else [0, 0, 0]))
    return arr


def decide(length: int, pass1: Sequence[Sequence[int]], pass2: Sequence[Sequence[int]] = (),
           params: Optional[Params] = None) -> Tuple[int, int, int, bool]:
    """The decision of siamaera:277-448 from alignment lists (qas, qae, sas, sae[, ...]) ->
    (action, from, to, inconclusive)."""
    p = params or default_params()
    d, inc = Decision(), C.c_int32()
    _abi.check(_lib().pr_siam_decide(C.byref(p), length, _hsp_array(pass1), len(pass1), _hsp_array(pass2), len(pass2),
                                     C.byref(d), C.byref(inc)), "pr_siam_decide")
    return d.action, d.frm, d.to, bool(inc.value)


def seeds(seq: bytes, word: int = 28) -> List[Tuple[int, int, int]]:
    """Test hook: every seed (i, p, len) of a read in (len desc, i asc, p asc) order."""
    L = _lib()
    s = np.ascontiguousarray(nt4(seq))
    n = C.c_int32()
    _abi.check(L.pr_siam_seeds_host(_abi.ptr(s, C.c_uint8), len(s), word, None, 0, C.byref(n)), "pr_siam_seeds_host")
    out = np.zeros(3 * max(n.value, 1), np.int32)
    _abi.check(L.pr_siam_seeds_host(_abi.ptr(s, C.c_uint8), len(s), word, _abi.ptr(out, C.c_int32), n.value, C.byref(n)),
               "pr_siam_seeds_host")
    return [tuple(int(x) for x in out[3 * k:3 * k + 3]) for k in range(n.value)]


def extend(q: bytes, t: bytes, h0: int, aligner: Optional[Aligner] = None) -> Tuple[int, int, int, int, int]:
    """Test hook: one ksw_extend2 extension with counts -> (score, qle, tle, matches, cols)."""
    al = aligner or default_params().pass1
    qa, ta = np.ascontiguousarray(nt4(q)), np.ascontiguousarray(nt4(t))
    out = np.zeros(5, np.int32)
    _abi.check(_lib().pr_siam_extend_host(C.byref(al), _abi.ptr(qa, C.c_uint8), len(qa), _abi.ptr(ta, C.c_uint8), len(ta),
                                          h0, _abi.ptr(out, C.c_int32)), "pr_siam_extend_host")
    return tuple(int(x) for x in out)


def extend_gpu(pairs: Sequence[Tuple[bytes, bytes]], h0: Sequence[int], aligner: Optional[Aligner] = None, ctx=None):
    """Test hook: a batch of extensions on the device, one wave per pair -> [n, 5] array."""
    al = aligner or default_params().pass1
    q, qo = _batch([p[0] for p in pairs])
    t, to = _batch([p[1] for p in pairs])
    h = np.ascontiguousarray(h0, np.int32)
    out = np.zeros((max(len(pairs), 1), 5), np.int32)
    c = ctx or _abi.default_context()
    _abi.check(_lib().pr_siam_extend_gpu(c.h, C.byref(al), _abi.ptr(q, C.c_uint8), _abi.ptr(qo, C.c_int64),
                                         _abi.ptr(t, C.c_uint8), _abi.ptr(to, C.c_int64), _abi.ptr(h, C.c_int32),
                                         len(pairs), _abi.ptr(out, C.c_int32)), "pr_siam_extend_gpu")
    return out[:len(pairs)]


def edit_record(r: Record, frm: int, to: int) -> Record:
    """siamaera:373-374 / :389-390 (and :413-414, :431-432): keep [frm, to) of the read.  The
    tail form is substr_seq(j), the head form substr_seq(0, j); both append SIAMAERA:a,b."""
    rid, desc, seq, qual = r
    if frm > 0:
        tag = f"SUBSTR:{frm} SIAMAERA:{frm},{len(seq)}"
        seq, qual = seq[frm:], (qual[frm:] if qual is not None else None)
    else:
        tag = f"SUBSTR:0,{to} SIAMAERA:0,{to}"
        seq, qual = seq[:to], (qual[:to] if qual is not None else None)
    return rid, f"{desc} {tag}" if desc else tag, seq, qual


def filter_records(records: Sequence[Record], params: Optional[Params] = None, device: bool = True, ctx=None,
                   threads: int = 0) -> Tuple[List[Record], dict]:
    """siamaera's main loop over records: trimmed reads edited, inconclusive reads dropped
    (filter_inconclusive) or kept, everything else unchanged -> (records, summary)."""
    dec, _, summary = run([r[2] for r in records], params, device, ctx, threads)
    out: List[Record] = []
    for r, (action, frm, to) in zip(records, dec):
        if action == TRIM:
            out.append(edit_record(r, int(frm), int(to)))
        elif action == KEEP:
            out.append(r)
    return out, summary


def summary_text(s: dict, filter_inconclusive: bool) -> str:
    """siamaera:477-484."""
    n = s["scanned"]
    if not n:
        return "Summary:\n0 reads scanned"
    return (f"Summary:\n{n} reads scanned\n"
            f"{s['trimmed']} siamaeras trimmed ({s['trimmed'] / n * 100:0.2f}%)\n"
            f"{s['inconclusive']} potential siamaeras with multiple, unresolved HSPs "
            f"{'filtered' if filter_inconclusive else 'ignored'} ({s['inconclusive'] / n * 100:0.2f}%)")


def parse_args(argv: Sequence[str]):
    ap = argparse.ArgumentParser(prog="siamaera", description="detect and trim self-similar chimaeras")
    ap.add_argument("-s", "--seq-min-len", type=int, default=150)
    ap.add_argument("-y", "--aln-min-idy", type=float, default=97.5)
    ap.add_argument("--filter-inconclusive", dest="filter_inconclusive", action="store_true", default=True)
    ap.add_argument("--no-filter-inconclusive", "--nofilter-inconclusive", dest="filter_inconclusive",
                    action="store_false")
    ap.add_argument("--term-ignore-len", type=int, default=10)
    ap.add_argument("--trim", type=int, default=5)
    ap.add_argument("--blast-path", default="", help="accepted and ignored (no BLAST is run)")
    ap.add_argument("-c", "--config", nargs="*", default=[], help="accepted and ignored")
    ap.add_argument("-V", "--version", action="store_true")
    ap.add_argument("-D", "--debug", action="store_true")
    ap.add_argument("--host", action="store_true", help="self-alignments on the host instead of the GPU")
    ap.add_argument("--threads", type=int, default=0)
    return ap.parse_args(list(argv))


def main(argv: Optional[Sequence[str]] = None, stdout=None, stderr=None) -> int:
    from .seqfilter import read_records
    a = parse_args(sys.argv[1:] if argv is None else argv)
    stdout = stdout or sys.stdout.buffer
    stderr = stderr or sys.stderr
    if a.version:
        stdout.write((VERSION + "\n").encode())
        stdout.flush()
        return 0
    recs = read_records("-")
    p = default_params(seq_min_len=a.seq_min_len, aln_min_idy=a.aln_min_idy, term_ignore_len=a.term_ignore_len,
                       trim=a.trim, filter_inconclusive=int(a.filter_inconclusive))
    out, summary = filter_records(recs, p, device=not a.host, threads=a.threads)
    fasta = any(r[3] is None for r in recs)
    stdout.write(b"".join(format_record(r, fasta, 0) for r in out))
    stdout.flush()
    if a.debug:
        print(f"[siamaera] {summary}", file=stderr)
    print("[siamaera] " + summary_text(summary, a.filter_inconclusive), file=stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())

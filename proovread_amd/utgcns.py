"""The unitig consensus: `bam2cns --utg-mode` (bin/proovread:1536-1586), the consensus half of
the tasks blasr-utg / dazzler-utg / bwa-utg of the modes sr+utg, mr+utg and utg.

Unitigs mapped onto a long read are added without bins (bam2cns:349-351), filtered by
--min-ncscore (Seq.pm:919-927), by --rep-coverage (Seq.pm:949-999) and for contained hits
(Seq.pm:1001-1047); the runs of high coverage (bam2cns:398-422) join the MCR ranges as ignored
columns of Sam::Seq's consensus (Seq.pm:714-734).  The rules live in csrc/utg_core.h (DESIGN.md
§14) and run through pr_utg_run (include/prgpu.h): on the GPU (csrc/utg_kernels.hip) or with
threads on the host.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _abi, cns

TOO_LONG, TOO_MANY, BAD_ALN = 1, 2, 4
MAX_LEN, MAX_ALNS = 262144, 4096
STATUS_NAMES = {TOO_LONG: "PR_UTG_TOO_LONG", TOO_MANY: "PR_UTG_TOO_MANY", BAD_ALN: "PR_UTG_BAD_ALN"}


class Params(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("trim", "indel_taboo_length", "min_aln_length", "phred_offset", "ref_phred_offset",
                                         "max_ins_length", "fallback_phred", "qual_weighted", "use_ref_qual", "invert_scores",
                                         "has_min_ncscore", "has_rep_coverage", "rep_coverage", "reserved")] + \
               [("indel_taboo", C.c_double), ("min_ncscore", C.c_double)]


class Batch(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("reserved", C.c_int32), ("n_alns", C.c_int64), ("read_off", _abi.P64),
                ("ref_seq", _abi.PU8), ("ref_qual", _abi.PU8), ("aln_off", _abi.P64), ("pos", _abi.P32), ("score", _abi.PD),
                ("has_score", _abi.PU8), ("has_qual", _abi.PU8), ("seq_off", _abi.P64), ("seq", _abi.PU8), ("qual", _abi.PU8),
                ("cig_off", _abi.P64), ("cigar", _abi.PU32), ("ign_off", _abi.P64), ("ign", _abi.P32), ("out_off", _abi.P64),
                ("win_off", _abi.P64)]


class Out(C.Structure):
    _fields_ = [(k, _abi.P32) for k in ("status", "seq_len", "trace_len", "n_win")] + \
               [(k, _abi.PU8) for k in ("seq", "qual", "trace", "kept")] + [("win", _abi.P32)]


@dataclasses.dataclass
class UtgParams:
    """The Sam::Seq class settings and bam2cns options of a --utg-mode call (bam2cns:171-237)."""
    trim: int = 1                        # cfg sr-trim
    indel_taboo_length: int = 7          # cfg sr-indel-taboo-length
    indel_taboo: float = 0.1             # cfg sr-indel-taboo
    min_aln_length: int = 50             # StateMatrixMinAlnLength
    phred_offset: int = 33
    qv_offset: int = 33                  # --qv-offset
    max_ins_length: int = 0              # --max-ins-length
    fallback_phred: int = 1              # --fallback-phred
    qual_weighted: bool = False          # --qual-weighted
    use_ref_qual: bool = True            # --[no-]use-ref-qual
    invert_scores: bool = False          # --invert-scores
    min_ncscore: Optional[float] = None  # --min-ncscore
    rep_coverage: Optional[int] = None   # --rep-coverage

    def to_c(self) -> Params:
        return Params(int(self.trim), int(self.indel_taboo_length or 0), int(self.min_aln_length), int(self.phred_offset),
                      int(self.qv_offset), int(self.max_ins_length), int(self.fallback_phred), int(bool(self.qual_weighted)),
                      int(bool(self.use_ref_qual)), int(bool(self.invert_scores)), int(self.min_ncscore is not None),
                      int(self.rep_coverage is not None), int(self.rep_coverage or 0), 0, float(self.indel_taboo),
                      float(self.min_ncscore or 0.0))


@dataclasses.dataclass
class Result(cns.ReadResult):
    """cns.ReadResult (what bam2cns.write_outputs prints) with the overlap windows of
    bam2cns:398-422 as (offset, length); `kept` flags the read's alignments that survived."""
    windows: List[Tuple[int, int]] = dataclasses.field(default_factory=list)


_set = False
_NORM = bytes(c if chr(c) in "ACGTN" else (ord(chr(c).upper()) if chr(c).upper() in "ACGT" else ord("N")) for c in range(256))


def _lib():
    global _set
    L = _abi.lib()
    if not _set:
        L.pr_utg_run.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Batch), C.c_int, C.POINTER(Out)]
        L.pr_utg_last_ms.argtypes = [C.c_void_p, _abi.PD]
        L.pr_utg_last_split.argtypes = [C.c_void_p, _abi.PD]
        _set = True
    return L


def _offsets(lens) -> np.ndarray:
    off = np.zeros(len(lens) + 1, np.int64)
    if len(lens):
        off[1:] = np.cumsum(lens)
    return off


def _pool(parts: Sequence[bytes]) -> np.ndarray:
    return np.frombuffer(b"".join(parts) + b"\0", np.uint8).copy()


class Packed:
    """The ctypes view of a chunk of reads with their alignments, and the arrays that back it."""

    def __init__(self, reads: Sequence[cns.LongRead], alns: Sequence[Sequence[cns.SamRecord]]):
        if len(reads) != len(alns):
            raise ValueError("utg: one alignment list per read")
        if any(r.seq is None for r in reads):
            raise ValueError("utg: needs the reads' sequences (--ref)")
        fasta = [r.qual is None for r in reads]
        if any(fasta) and not all(fasta):
            raise ValueError("utg: reads with and without qualities in one chunk")
        flat = [a for al in alns for a in al]
        for a in flat:
            if a.qual != "*" and len(a.qual) != len(a.seq):
                raise ValueError("utg: QUAL length != SEQ length")
        self.n_reads, self.n_alns = len(reads), len(flat)
        self.read_off = _offsets([len(r.seq) for r in reads])
        self.ref_seq = _pool([r.seq.encode("latin-1") for r in reads])
        self.ref_qual = None if (not reads or fasta[0]) else _pool([r.qual.encode("latin-1") for r in reads])
        self.aln_off = _offsets([len(al) for al in alns])
        self.pos = np.array([a.pos for a in flat] or [0], np.int32)
        self.score = np.array([a.score if a.score is not None else 0.0 for a in flat] or [0.0], np.float64)
        self.has_score = np.array([a.score is not None for a in flat] or [0], np.uint8)
        self.has_qual = np.array([a.qual != "*" for a in flat] or [0], np.uint8)
        self.seq_off = _offsets([len(a.seq) for a in flat])
        self.seq = _pool([a.seq.encode("latin-1").translate(_NORM) for a in flat])
        self.qual = _pool([(a.qual if a.qual != "*" else "!" * len(a.seq)).encode("latin-1") for a in flat])
        self.cig_off = _offsets([len(a.cigar) for a in flat])
        self.cigar = np.array([op for a in flat for op in a.cigar] + [0], np.uint32)
        ign = [r.mcr_ranges() for r in reads]
        self.ign_off = _offsets([len(x) for x in ign])
        self.ign = np.array([v for x in ign for pr in x for v in pr] + [0], np.int64).clip(-2**31, 2**31 - 1).astype(np.int32)
        self.out_off = _offsets([len(r.seq) + sum(len(a.seq) for a in al) for r, al in zip(reads, alns)])
        self.win_off = _offsets([max(len(al), 1) for al in alns])
        P = _abi.ptr
        self.batch = Batch(self.n_reads, 0, self.n_alns, P(self.read_off, C.c_int64), P(self.ref_seq, C.c_uint8),
                           P(self.ref_qual, C.c_uint8) if self.ref_qual is not None else None, P(self.aln_off, C.c_int64),
                           P(self.pos, C.c_int32), P(self.score, C.c_double), P(self.has_score, C.c_uint8),
                           P(self.has_qual, C.c_uint8), P(self.seq_off, C.c_int64), P(self.seq, C.c_uint8), P(self.qual, C.c_uint8),
                           P(self.cig_off, C.c_int64), P(self.cigar, C.c_uint32), P(self.ign_off, C.c_int64), P(self.ign, C.c_int32),
                           P(self.out_off, C.c_int64), P(self.win_off, C.c_int64))
        n = max(self.n_reads, 1)
        self.status, self.seq_len, self.trace_len, self.n_win = (np.zeros(n, np.int32) for _ in range(4))
        self.oseq, self.oqual, self.otrace = (np.zeros(int(self.out_off[-1]) + 1, np.uint8) for _ in range(3))
        self.kept = np.zeros(self.n_alns + 1, np.uint8)
        self.win = np.zeros(2 * int(self.win_off[-1]) + 2, np.int32)
        self.out = Out(*[P(a, C.c_int32) for a in (self.status, self.seq_len, self.trace_len, self.n_win)],
                       *[P(a, C.c_uint8) for a in (self.oseq, self.oqual, self.otrace, self.kept)], P(self.win, C.c_int32))

    def results(self, reads: Sequence[cns.LongRead]) -> List[Result]:
        res = []
        for r, read in enumerate(reads):
            o, n, t = int(self.out_off[r]), int(self.seq_len[r]), int(self.trace_len[r])
            w = self.win[2 * int(self.win_off[r]):2 * (int(self.win_off[r]) + int(self.n_win[r]))]
            res.append(Result(read.id, int(self.status[r]), self.oseq[o:o + n].tobytes().decode("latin-1"),
                              self.oqual[o:o + n].tobytes().decode("latin-1"), self.otrace[o:o + t].tobytes().decode("latin-1"),
                              kept=self.kept[int(self.aln_off[r]):int(self.aln_off[r + 1])].astype(bool),
                              windows=[(int(w[2 * k]), int(w[2 * k + 1])) for k in range(len(w) // 2)]))
        return res


def status_name(status: int) -> str:
    return "|".join(n for b, n in STATUS_NAMES.items() if status & b) or str(status)


def run_packed(reads: Sequence[cns.LongRead], A: Packed, params: UtgParams, device: bool = True, ctx=None, threads: int = 0,
               timing: Optional[dict] = None) -> List[Result]:
    p = params.to_c()
    c = None if not device else (ctx or _abi.default_context())
    _abi.check(_lib().pr_utg_run(c.h if c is not None else None, C.byref(p), C.byref(A.batch), threads, C.byref(A.out)),
               "pr_utg_run")
    if timing is not None and c is not None:
        v, k = C.c_double(), (C.c_double * 5)()
        _abi.check(_lib().pr_utg_last_ms(c.h, C.byref(v)), "pr_utg_last_ms")
        _abi.check(_lib().pr_utg_last_split(c.h, k), "pr_utg_last_split")
        timing.update(kernel_ms=v.value, split_ms=dict(zip(("prep", "coverage", "contained", "consensus", "pack"), list(k))))
    return A.results(reads)


def run(reads: Sequence[cns.LongRead], alns: Sequence[Sequence[cns.SamRecord]], params: UtgParams, device: bool = True,
        ctx=None, threads: int = 0) -> List[Result]:
    """bam2cns:375-455 with --utg-mode for every read: `alns[i]` are read i's alignments in file
    order.  device False: the host path (no GPU needed)."""
    if not reads:
        return []
    return run_packed(reads, Packed(reads, alns), params, device, ctx, threads)

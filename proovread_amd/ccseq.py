"""`ccseq`: circular consensus of PacBio subreads (bin/ccseq), the task `ccs-1` of the modes
sr and mr (proovread.cfg:107-109, bin/proovread:871-895).

All subreads of one ZMW (`m.../zmw/start_end` ids, consecutive in the input) collapse into one
read: ccseq picks one subread as the reference (ccseq:356-363), maps the others onto it with
bwa-proovread and takes Sam::Seq's quality-weighted consensus (ccseq:267-270).  Grouping, output
and the consensus engine are restated line by line; the mapping comes from libprgpu.so's own
rules (pr_ccs_*, include/prgpu.h): exact seeds vote for an orientation and a
diagonal, one banded local alignment per subread follows, on the GPU (csrc/ccs_kernels.hip) or
with threads on the host.  Parity of the mapping with bwa-proovread is unpinned.

    ccseq [--reads FQ | < FQ] > out.fq
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .seqfilter import Record, format_record

SECONDARY, PRIMARY, SINGLE = 0, 1, 2
TOO_LONG, TOO_MANY, BAD_ALN = 1, 2, 4
MAX_LEN, MAX_SUBREADS, MAX_BAND = 16384, 64, 512
ID_NOT_SUBREAD, ID_NOT_UNIQUE = 1, 2
_OPS = "MIDNS"


class Params(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("k", "w", "a", "b", "o_del", "o_ins", "e_del", "e_ins", "trim", "min_aln_length",
                                         "phred_offset", "reserved")] + [("indel_taboo", C.c_double)]


class Batch(C.Structure):
    _fields_ = [("n_groups", C.c_int32), ("n_sub", C.c_int32), ("grp_off", _abi.P32), ("grp_ref", _abi.P32),
                ("off", _abi.P64), ("seq", _abi.PU8), ("qual", _abi.PU8), ("cig_off", _abi.P64), ("out_off", _abi.P64)]


class Alns(C.Structure):
    _fields_ = [(k, _abi.P32) for k in ("mapped", "strand", "pos", "score", "n_cigar")] + [("cigar", _abi.PU32)]


class Out(C.Structure):
    _fields_ = [(k, _abi.P32) for k in ("status", "seq_len", "trace_len")] + [(k, _abi.PU8) for k in ("seq", "qual", "trace")]


class SubreadIdError(ValueError):
    """ccseq:238-243: an id that is no PacBio subread id, or one seen before."""

    def __init__(self, kind: int, index: int, rid: str):
        self.kind, self.index, self.rid = kind, index, rid
        super().__init__(("Not a valid PacBio subread id: " if kind == ID_NOT_SUBREAD else "Non-unique ID: ") + rid)


# a group: the subreads of one ZMW in input order and the index of the reference among them
Group = Tuple[List[bytes], List[bytes], int]            # seqs, quals, ref
Alignment = Optional[Tuple[int, int, int, str]]         # strand, pos (0-based), score, CIGAR; None: unmapped

_set = False


def _lib():
    global _set
    L = _abi.lib()
    if not _set:
        L.pr_ccs_params_default.argtypes = [C.POINTER(Params)]
        L.pr_ccs_params_default.restype = None
        L.pr_ccs_group.argtypes = [C.c_int32, C.c_char_p, _abi.P64, _abi.P32, _abi.P32, _abi.P32, _abi.P32, _abi.P32, _abi.P32]
        L.pr_ccs_run.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Batch), C.c_int, C.POINTER(Alns), C.POINTER(Out)]
        L.pr_ccs_map.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Batch), C.c_int, C.POINTER(Alns)]
        L.pr_ccs_cns.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Batch), C.c_int, C.POINTER(Alns), C.POINTER(Out)]
        L.pr_ccs_last_ms.argtypes = [C.c_void_p, _abi.PD]
        _set = True
    return L


def default_params(**over) -> Params:
    """ccseq:97 (-k 9 -w 300 -A 5 -B 11 -O 2,1 -E 4,3) and ccseq:214-217."""
    p = Params()
    _lib().pr_ccs_params_default(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


_NORM = bytes(c if chr(c) in "ACGT" else (ord(chr(c).upper()) if chr(c).upper() in "ACGT" else ord("N")) for c in range(256))
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def normalise(seq: bytes) -> bytes:
    """The stage's alphabet: upper case, everything but A C G T becomes N."""
    return bytes(seq).translate(_NORM)


def revcomp(seq: bytes) -> bytes:
    return bytes(seq).translate(_COMP)[::-1]


def group(ids: Sequence[str], lens: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, int]:
    """ccseq:237-299 and :356-363 -> (role [n], group [n], number of groups); raises SubreadIdError."""
    L = _lib()
    n = len(ids)
    enc = [i.encode("latin-1") for i in ids]
    off = np.zeros(n + 1, np.int64)
    if n:
        off[1:] = np.cumsum([len(e) for e in enc])
    ln = np.ascontiguousarray(lens, np.int32) if n else np.zeros(1, np.int32)
    role, grp = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    ng, kind, idx = C.c_int32(), C.c_int32(), C.c_int32()
    _abi.check(L.pr_ccs_group(n, b"".join(enc), _abi.ptr(off, C.c_int64), _abi.ptr(ln, C.c_int32), _abi.ptr(role, C.c_int32),
                              _abi.ptr(grp, C.c_int32), C.byref(ng), C.byref(kind), C.byref(idx)), "pr_ccs_group")
    if kind.value:
        raise SubreadIdError(kind.value, idx.value, ids[idx.value])
    return role[:n], grp[:n], ng.value


class _Arrays:
    """The ctypes view of a list of groups, with the arrays that back it."""

    def __init__(self, groups: Sequence[Group]):
        seqs = [s for g in groups for s in g[0]]
        quals = [q for g in groups for q in g[1]]
        for s, q in zip(seqs, quals):
            if len(s) != len(q):
                raise ValueError("ccs: quality length != sequence length")
        self.n_sub, self.n_groups = len(seqs), len(groups)
        lens = np.array([len(s) for s in seqs], np.int64)
        self.off = np.zeros(self.n_sub + 1, np.int64)
        self.off[1:] = np.cumsum(lens)
        self.seq = np.frombuffer(b"".join(seqs) + b"\0", np.uint8).copy()
        self.qual = np.frombuffer(b"".join(quals) + b"\0", np.uint8).copy()
        self.grp_off = np.zeros(self.n_groups + 1, np.int32)
        self.grp_off[1:] = np.cumsum([len(g[0]) for g in groups])
        self.grp_ref = np.array([self.grp_off[k] + g[2] for k, g in enumerate(groups)] or [0], np.int32)
        cig_len, out_len = np.zeros(self.n_sub, np.int64), np.zeros(self.n_groups, np.int64)
        for k in range(self.n_groups):
            s0, s1 = int(self.grp_off[k]), int(self.grp_off[k + 1])
            cig_len[s0:s1] = lens[s0:s1] + lens[self.grp_ref[k]] + 2
            out_len[k] = lens[s0:s1].sum()
        self.cig_off = np.zeros(self.n_sub + 1, np.int64)
        self.cig_off[1:] = np.cumsum(cig_len)
        self.out_off = np.zeros(self.n_groups + 1, np.int64)
        self.out_off[1:] = np.cumsum(out_len)
        self.batch = Batch(self.n_groups, self.n_sub, _abi.ptr(self.grp_off, C.c_int32), _abi.ptr(self.grp_ref, C.c_int32),
                           _abi.ptr(self.off, C.c_int64), _abi.ptr(self.seq, C.c_uint8), _abi.ptr(self.qual, C.c_uint8),
                           _abi.ptr(self.cig_off, C.c_int64), _abi.ptr(self.out_off, C.c_int64))
        n = max(self.n_sub, 1)
        self.mapped, self.strand, self.pos, self.score, self.n_cigar = (np.zeros(n, np.int32) for _ in range(5))
        self.cigar = np.zeros(int(self.cig_off[-1]) + 1, np.uint32)
        self.alns = Alns(*[_abi.ptr(a, C.c_int32) for a in (self.mapped, self.strand, self.pos, self.score, self.n_cigar)],
                         _abi.ptr(self.cigar, C.c_uint32))
        ng = max(self.n_groups, 1)
        self.status, self.seq_len, self.trace_len = (np.zeros(ng, np.int32) for _ in range(3))
        self.oseq, self.oqual, self.otrace = (np.zeros(int(self.out_off[-1]) + 1, np.uint8) for _ in range(3))
        self.out = Out(*[_abi.ptr(a, C.c_int32) for a in (self.status, self.seq_len, self.trace_len)],
                       *[_abi.ptr(a, C.c_uint8) for a in (self.oseq, self.oqual, self.otrace)])

    def set_alignments(self, alns: Sequence[Sequence[Alignment]]):
        for k, ga in enumerate(alns):
            for t, a in enumerate(ga):
                s = int(self.grp_off[k]) + t
                if a is None:
                    continue
                ops = parse_cigar(a[3])
                if len(ops) > self.cig_off[s + 1] - self.cig_off[s]:
                    raise ValueError("ccs: CIGAR longer than its slot")
                self.mapped[s], self.strand[s], self.pos[s], self.score[s], self.n_cigar[s] = 1, a[0], a[1], a[2], len(ops)
                self.cigar[self.cig_off[s]:self.cig_off[s] + len(ops)] = ops

    def alignments(self) -> List[List[Alignment]]:
        res: List[List[Alignment]] = []
        for k in range(self.n_groups):
            ga: List[Alignment] = []
            for s in range(int(self.grp_off[k]), int(self.grp_off[k + 1])):
                if not self.mapped[s]:
                    ga.append(None)
                    continue
                ops = self.cigar[self.cig_off[s]:self.cig_off[s] + self.n_cigar[s]]
                ga.append((int(self.strand[s]), int(self.pos[s]), int(self.score[s]),
                           "".join(f"{int(x) >> 4}{_OPS[int(x) & 15]}" for x in ops)))
            res.append(ga)
        return res

    def results(self) -> List[Tuple[int, bytes, bytes, bytes]]:
        res = []
        for k in range(self.n_groups):
            o, n, t = int(self.out_off[k]), int(self.seq_len[k]), int(self.trace_len[k])
            res.append((int(self.status[k]), self.oseq[o:o + n].tobytes(), self.oqual[o:o + n].tobytes(),
                        self.otrace[o:o + t].tobytes()))
        return res


def parse_cigar(cigar: str) -> List[int]:
    ops, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            ops.append(int(num) << 4 | _OPS.index(ch))
            num = ""
    return ops


def _ctx(device: bool, ctx):
    if not device:
        return None
    return ctx or _abi.default_context()


def _handle(c):
    return c.h if c is not None else None


def map_groups(groups: Sequence[Group], params: Optional[Params] = None, device: bool = True, ctx=None,
               threads: int = 0) -> List[List[Alignment]]:
    """Test hook: every subread mapped to its group's reference -> per group, per subread, an
    alignment or None (the reference itself, no seed, a group over a capacity)."""
    p = params or default_params()
    A = _Arrays(groups)
    _abi.check(_lib().pr_ccs_map(_handle(_ctx(device, ctx)), C.byref(p), C.byref(A.batch), threads, C.byref(A.alns)), "pr_ccs_map")
    return A.alignments()


def consensus_groups(groups: Sequence[Group], alns: Sequence[Sequence[Alignment]], params: Optional[Params] = None,
                     device: bool = True, ctx=None, threads: int = 0) -> List[Tuple[int, bytes, bytes, bytes]]:
    """Test hook: the consensus of each group from the alignments given -> (status, seq, qual, trace)."""
    p = params or default_params()
    A = _Arrays(groups)
    A.set_alignments(alns)
    _abi.check(_lib().pr_ccs_cns(_handle(_ctx(device, ctx)), C.byref(p), C.byref(A.batch), threads, C.byref(A.alns),
                                 C.byref(A.out)), "pr_ccs_cns")
    return A.results()


def run_groups(groups: Sequence[Group], params: Optional[Params] = None, device: bool = True, ctx=None, threads: int = 0):
    """The stage on groups -> (results [(status, seq, qual, trace)], alignments, kernel_ms or None)."""
    p = params or default_params()
    A = _Arrays(groups)
    c = _ctx(device, ctx)
    _abi.check(_lib().pr_ccs_run(_handle(c), C.byref(p), C.byref(A.batch), threads, C.byref(A.alns), C.byref(A.out)),
               "pr_ccs_run")
    ms = None
    if c is not None:
        v = C.c_double()
        _abi.check(_lib().pr_ccs_last_ms(c.h, C.byref(v)), "pr_ccs_last_ms")
        ms = v.value
    return A.results(), A.alignments(), ms


def sam_lines(ids: Sequence[str], grp: Group, alns: Sequence[Alignment]) -> List[str]:
    """Test hook: a group's alignments as SAM lines in arrival order (SEQ / QUAL in the aligned
    orientation, AS the DP score)."""
    seqs, quals, ref = grp
    out = []
    for t, a in enumerate(alns):
        if a is None:
            continue
        strand, pos, score, cigar = a
        seq, qual = (revcomp(seqs[t]), bytes(quals[t])[::-1]) if strand else (bytes(seqs[t]), bytes(quals[t]))
        out.append("\t".join([ids[t], "16" if strand else "0", ids[ref], str(pos + 1), "60", cigar, "*", "0", "0",
                              seq.decode(), qual.decode("latin-1"), f"AS:i:{score}"]))
    return out


def split_groups(records: Sequence[Record]):
    """Records -> (role [n], the groups as (record indices, Group)); sequences normalised."""
    role, grp, ng = group([r[0] for r in records], [len(r[2]) for r in records])
    members: List[List[int]] = [[] for _ in range(ng)]
    for k, g in enumerate(grp):
        if g >= 0:
            members[g].append(k)
    groups = []
    for mem in members:
        ref = next(t for t, k in enumerate(mem) if role[k] == PRIMARY)
        groups.append((mem, ([normalise(records[k][2]) for k in mem], [bytes(records[k][3]) for k in mem], ref)))
    return role, groups


def ccs_records(records: Sequence[Record], params: Optional[Params] = None, device: bool = True, ctx=None,
                threads: int = 0) -> Tuple[List[Record], Dict[str, int]]:
    """ccseq's main loop over FASTQ records in input order (ccseq:237-329): a group's reference
    subread becomes its consensus `@id CCS:primary`, a subread alone in its ZMW passes unchanged,
    every other subread is dropped -> (records, {single, primary, secondary, flagged, kernel_ms})."""
    for r in records:
        if r[3] is None:
            raise ValueError("ccseq: FASTQ input with qualities is required")
    role, groups = split_groups(records)
    results, _, ms = run_groups([g for _, g in groups], params, device, ctx, threads) if groups else ([], [], None)
    cons = {mem[g[2]]: res for (mem, g), res in zip(groups, results)}
    out: List[Record] = []
    stats = {"single": 0, "primary": 0, "secondary": 0, "flagged": 0}
    for k, r in enumerate(records):
        if role[k] == PRIMARY:
            stats["primary"] += 1
            status, seq, qual, _ = cons[k]
            if status:
                stats["flagged"] += 1
                out.append(r)
            else:
                out.append((r[0], "CCS:primary", seq, qual))   # state_matrix_consensus builds '@'.id: the description is gone
        elif role[k] == SINGLE:
            stats["single"] += 1
            out.append(r)
        else:
            stats["secondary"] += 1
    if ms is not None:
        stats["kernel_ms"] = ms
    return out, stats


def summary_text(s: Dict[str, int]) -> List[str]:
    """ccseq:324-328."""
    src, rc = s["single"] + s["primary"] + s["secondary"], s["single"] + s["primary"]
    return [f"Processed {src} subreads from {rc} reads",
            f"  {s['primary']} consensus + {s['single']} bypassed single subreads"]


def parse_args(argv: Sequence[str]):
    ap = argparse.ArgumentParser(prog="ccseq", description="circular consensus of PacBio subreads")
    ap.add_argument("reads_pos", nargs="?", default=None)
    ap.add_argument("--reads", default=None)
    ap.add_argument("-p", "--pre", default=".", help="accepted and ignored (no temporary files)")
    ap.add_argument("--threads", type=int, default=1)
    ap.add_argument("--chunk_seqs", "--chunk-seqs", type=int, default=2000, help="accepted and ignored (DESIGN.md §13)")
    ap.add_argument("--bwa-path", "--bwa_path", default="", help="accepted and ignored (no bwa is run)")
    ap.add_argument("-c", "--config", nargs="*", default=[], help="accepted and ignored")
    ap.add_argument("-V", "--version", action="store_true")
    ap.add_argument("-D", "--debug", action="store_true")
    ap.add_argument("--host", action="store_true", help="run on the host instead of the GPU")
    return ap.parse_args(list(argv))


def _log(stderr, msg: str):
    print(f"[{time.strftime('%y-%m-%d %H:%M:%S')}] [ccseq] {msg}", file=stderr)


def main(argv: Optional[Sequence[str]] = None, stdout=None, stderr=None) -> int:
    from .seqfilter import read_records
    a = parse_args(sys.argv[1:] if argv is None else argv)
    stdout = stdout or sys.stdout.buffer
    stderr = stderr or sys.stderr
    if a.version:
        stdout.write(b"0.01\n")
        stdout.flush()
        return 0
    src = a.reads or a.reads_pos
    if not src:
        _log(stderr, "Reading STDIN")
    recs = read_records(src or "-")
    try:
        out, stats = ccs_records(recs, device=not a.host, threads=a.threads)
    except SubreadIdError as e:
        _log(stderr, str(e))
        return 255
    stdout.write(b"".join(format_record(r, False, 0) for r in out))
    stdout.flush()
    if a.debug:
        _log(stderr, str(stats))
    for line in summary_text(stats):
        _log(stderr, line)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The unitig consensus (bam2cns --utg-mode) restated in plain Python from DESIGN.md §14:
a state matrix of per-column dictionaries, the three filters, the overlap windows and the
majority vote, with ties in length broken by arrival.  Slow and simple on purpose: it is the
arbiter for the random cases (tied lengths included) and must itself equal the golden records
of the reference's Perl engine (tests/golden/utg_expected.txt).
"""
from __future__ import annotations

import dataclasses
import math
import re
from typing import Dict, List, Optional, Sequence, Tuple

BAD_ALN = 4
FIXED = ["A", "T", "G", "C", "-", "N"]


class BadAlignment(Exception):
    """What the reference dies on."""


@dataclasses.dataclass
class Aln:
    name: str
    pos: int                        # 1-based POS
    ops: List[Tuple[int, str]]
    seq: str
    qual: str                       # '*' for none
    score: Optional[float]

    @classmethod
    def from_sam(cls, line: str) -> "Aln":
        f = line.rstrip("\n").split("\t")
        score = None
        for t in f[11:]:
            if t.startswith("AS:"):
                score = float(t[5:])
        seq = "".join(c if c in "ACGTN" else (c.upper() if c.upper() in "ACGT" else "N") for c in f[9])
        return cls(f[0], int(f[3]), [(int(n), op) for n, op in re.findall(r"(\d+)(\D)", f[5])], seq, f[10], score)

    def length(self) -> int:
        if self.ops and (self.ops[0][1] == "S" or self.ops[-1][1] == "S"):
            return sum(n for n, op in self.ops if op in "MD")
        return len(self.seq)


@dataclasses.dataclass
class Params:
    trim: int = 1
    indel_taboo_length: int = 7
    indel_taboo: float = 0.1
    min_aln_length: int = 50
    phred_offset: int = 33
    qv_offset: int = 33
    max_ins_length: int = 0
    fallback_phred: int = 1
    qual_weighted: bool = False
    use_ref_qual: bool = True
    invert_scores: bool = False
    min_ncscore: Optional[float] = None
    rep_coverage: Optional[int] = None


def phred2freq(p: int) -> float:
    return int(((p * p / 120.0) * 100) + 0.5) / 100


def freq2phred(f: float) -> int:
    return min(40, int(math.sqrt(f * 120.0) + 0.5))


def in_ranges(c: int, ranges: Sequence[Tuple[int, int]]) -> bool:
    return any(o <= c < o + n for o, n in ranges)


def range_in_ranges(pos: int, length: int, ranges: Sequence[Sequence[int]]) -> bool:
    c1, c2 = pos, pos + length - 1
    return any(o <= c1 < o + n and o <= c2 < o + n for o, n in ranges)


def states_of(a: Aln, p: Params, L: int):
    """The states of one alignment and their qualities from the first column rpos on, or None
    when the alignment is passed over."""
    if not len(a.seq) > p.min_aln_length:
        return None
    seq, qua = a.seq, a.qual if a.qual != "*" else chr(p.fallback_phred + p.phred_offset) * len(a.seq)
    ops = list(a.ops)
    if any(n <= 0 for n, _ in ops):
        raise BadAlignment("zero-length op")
    if ops and ops[0][1] == "S":
        seq, qua = seq[ops[0][0]:], qua[ops[0][0]:]
        ops.pop(0)
    if ops and ops[-1][1] == "S":
        seq, qua = seq[:len(seq) - ops[-1][0]], qua[:len(qua) - ops[-1][0]]
        ops.pop()
    if ops and ops[0][1] == "H":
        ops.pop(0)
    if ops and ops[-1][1] == "H":
        ops.pop()
    if not ops:
        raise BadAlignment("empty CIGAR")
    if any(op not in "MID" for _, op in ops):
        raise BadAlignment("unknown CIGAR op")
    if sum(n for n, op in ops if op in "MI") != len(seq):
        raise BadAlignment("CIGAR and SEQ differ in length")
    orig = len(a.seq)
    rpos = a.pos - 1
    if p.trim:
        taboo = p.indel_taboo_length if p.indel_taboo_length else int(orig * p.indel_taboo + 0.5)
        mc = dc = ic = 0
        for i, (n, op) in enumerate(ops):
            if op == "M":
                if mc + ic + n > taboo:
                    if i:
                        ops = ops[i:]
                        rpos += mc + dc
                        seq, qua = seq[mc + ic:], qua[mc + ic:]
                    break
                mc += n
            elif op == "D":
                dc += n
            else:
                ic += n
        if len(seq) < 50 or len(seq) / orig < 0.7:
            return None
        tail = 0
        for i in range(len(ops) - 1, 0, -1):
            n, op = ops[i]
            if op == "M":
                tail += n
                if tail > taboo:
                    if i < len(ops) - 1:
                        cut = tail - n
                        ops = ops[:i + 1]
                        seq, qua = seq[:len(seq) - cut], qua[:len(qua) - cut]
                    break
            elif op == "I":
                tail += n
        if len(seq) < p.min_aln_length or len(seq) / orig < 0.7:
            return None
    states: List[str] = []
    squals: List[str] = []
    q = 0
    for i, (n, op) in enumerate(ops):
        if op == "M":
            states += list(seq[q:q + n])
            squals += list(qua[q:q + n])
            q += n
        elif op == "D":
            states += ["-"] * n
            qb = qua[q - 1] if q > 1 else qua[q:q + 1]
            qa = qua[q] if q < len(qua) else qua[q - 1:q]
            squals += [min(qb, qa)] * n
        else:
            if i:
                if states[-1] == "-":
                    states[-1], squals[-1] = seq[q:q + n], qua[q:q + n]
                else:
                    states[-1] += seq[q:q + n]
                    squals[-1] += qua[q:q + n]
            else:
                states.append(seq[q:q + n])
                squals.append(qua[q:q + n])
            q += n
    if q != len(seq) or rpos < 0 or rpos + len(states) > L:
        raise BadAlignment("columns beyond the read")
    return rpos, states, squals


def state_matrix(alns: Sequence[Aln], p: Params, L: int, ref: Optional[Tuple[str, Optional[str]]], known: Dict[str, int],
                 ignore: Sequence[Tuple[int, int]] = (), qual_weighted: bool = False, use_ref_qual: bool = False):
    S: List[Dict[int, float]] = [dict() for _ in range(L)]
    known = dict(known)
    if use_ref_qual and ref and ref[1] is not None:
        for i, (b, q) in enumerate(zip(*ref)):
            f = phred2freq(ord(q) - p.qv_offset)
            if f:
                k = known.get(b, 5)
                S[i][k] = S[i].get(k, 0) + f
    for a in alns:
        st = states_of(a, p, L)
        if st is None:
            continue
        rpos, states, squals = st
        for s, sq in zip(states, squals):
            if ignore and in_ranges(rpos, ignore):
                rpos += 1
                continue
            if len(s) > 1 and s not in known:
                known[s] = len(known)
            k = known.get(s, 5)
            if qual_weighted:
                w = min(phred2freq(ord(c) - p.phred_offset) for c in sq) if sq else 0.0
            else:
                w = 1
            S[rpos][k] = S[rpos].get(k, 0) + w
            rpos += 1
    return S, known


def runs(cov: Sequence[float], cmax) -> List[List[int]]:
    out, start = [], None
    for i, c in enumerate(list(cov) + [None]):
        hi = c is not None and not c < cmax
        if hi and start is None:
            start = i
        elif not hi and start is not None:
            out.append([start, i - start])
            start = None
    return out


def consensus(ref_seq: str, ref_qual: Optional[str], mcrs: Sequence[Tuple[int, int]], alns: Sequence[Aln], p: Params):
    """-> (status, seq, qual, trace, kept [bool per alignment], windows)."""
    L = len(ref_seq)
    known = {s: i for i, s in enumerate(FIXED)}
    alive = list(range(len(alns)))

    def score(a: Aln):
        return None if a.score is None else (a.score * -1 if p.invert_scores else a.score)

    try:
        if p.min_ncscore is not None:                                   # step 1
            keep = []
            for i in alive:
                sc, ln = score(alns[i]), alns[i].length()
                if sc is None:
                    continue
                if ln == 0:
                    raise BadAlignment("length 0")
                if not (sc / ln) * (ln / (40 + ln)) < p.min_ncscore:
                    keep.append(i)
            alive = keep
        cov = []
        if p.rep_coverage is not None:                                   # step 2
            S, known = state_matrix([alns[i] for i in alive], p, L, None, known)
            cov = [sum(c.values()) for c in S]
            rwin = runs(cov, p.rep_coverage)
            if rwin:
                for w in rwin:
                    w[0] -= 150
                    w[1] += 300
                if rwin[0][0] < 0:
                    rwin[0][1] += rwin[0][0]
                    rwin[0][0] = 0
                rwin[-1][1] -= 1 if L - (rwin[-1][0] + rwin[-1][1]) < 0 else 0
                alive = [i for i in alive if not range_in_ranges(alns[i].pos, alns[i].length(), rwin)]
        # step 3: longest first, ties in arrival order; popped from the short end
        order = sorted(alive, key=lambda i: -alns[i].length())
        ids = list(order)
        coords = [[alns[i].pos, alns[i].length()] for i in order]
        scores = [score(alns[i]) or 0 for i in order]
        gone = set()
        while len(ids) > 1:
            iid, coo = ids.pop(), coords.pop()
            if coo[1] < 21:
                coo = [coo[0] + coo[1] // 2, 1]
            else:
                ad = int(coo[1] * 0.1)
                coo = [coo[0] + ad, coo[1] - 2 * ad]
            if range_in_ranges(coo[0], coo[1], coords):
                if coo[1] > coords[-1][1] - 40:
                    i = len(coords)
                    if scores[i] > scores[i - 1]:
                        iid, restore = ids.pop(), iid
                        coords.pop()
                        ids.append(restore)
                        coords.append(coo)
                gone.add(iid)
        alive = [i for i in alive if i not in gone]
        owin = [tuple(w) for w in runs(cov, p.rep_coverage)] if cov else []   # step 4: step 2's matrix or none
        S, known = state_matrix([alns[i] for i in alive], p, L, (ref_seq, ref_qual), known, ignore=list(mcrs) + owin,
                                qual_weighted=p.qual_weighted, use_ref_qual=p.use_ref_qual)
    except BadAlignment:
        return BAD_ALN, "", "", "", [False] * len(alns), []
    names = {i: s for s, i in known.items()}
    seq, freqs, trace = [], [], []
    for c, col in enumerate(S):
        best, idx = 0, None
        for k in sorted(col):
            f = col[k]
            if f > best:
                if p.max_ins_length and k > 4 and len(names[k]) > p.max_ins_length:
                    continue
                best, idx = f, k
        if not best:
            seq.append(ref_seq[c]), freqs.append(0), trace.append("M")
        elif idx == 4:
            trace.append("I")
        else:
            s = names[idx]
            seq.append(s), freqs.extend([best] * len(s)), trace.append("M" + "D" * (len(s) - 1))
    qual = "".join(chr(freq2phred(f) + p.phred_offset) for f in freqs)
    kept = [i in set(alive) for i in range(len(alns))]
    return 0, "".join(seq), qual, "".join(trace), kept, owin

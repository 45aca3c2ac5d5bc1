"""Plain-Python restatement of the ccs-1 rules of DESIGN.md §13 — TEST INFRASTRUCTURE.

Written from the text, not from the library: the grouping of ccseq:237-299 / :356-363 and the
mapping rules (seeds, orientation and band centre, banded local alignment).  Slow on purpose.
Also the simulator of ZMWs the ccs tests share.
"""
from __future__ import annotations

import random
import re
from typing import Dict, List, Optional, Sequence, Tuple

SUBREAD = re.compile(r"^(m[^/]+/\d+)/(\d+_\d+)")
NEG = -0x40000000
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


class BadId(Exception):
    def __init__(self, kind, index):
        self.kind, self.index = kind, index
        super().__init__(f"{kind} at {index}")


def group_ref(ids: Sequence[str], lens: Sequence[int]):
    """-> (roles, groups): roles 'primary' / 'single' / 'secondary' per record, groups as lists of
    record indices.  Raises BadId('not_subread' | 'not_unique', index)."""
    roles = ["secondary"] * len(ids)
    groups: List[List[int]] = []
    seen = set()
    cache: List[int] = []
    cid = None
    for k, rid in enumerate(ids):
        m = SUBREAD.match(rid)
        if not m:
            raise BadId("not_subread", k)
        if rid in seen:
            raise BadId("not_unique", k)
        seen.add(rid)
        if cid is not None and m.group(1) == cid:
            cache.append(k)
        else:
            if len(cache) > 1:
                groups.append(cache)
            elif len(cache) == 1:
                roles[cache[0]] = "single"
            cid = m.group(1)
            cache = [k]
    if len(cache) > 1:      # no elsif: a lone last record is never 'single'
        groups.append(cache)
    for g in groups:
        if len(g) == 2:
            ref = g[0] if lens[g[0]] > lens[g[1]] else g[1]
        else:
            ref = g[1]
        roles[ref] = "primary"
    return roles, groups


def revcomp(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def seeds(R: str, Q: str, k: int):
    """Every maximal run of matching cells (i + t, j + t), length >= k -> (i, j, len); N never matches."""
    out = []
    for d in range(-(len(Q) - 1), len(R)):
        i = max(0, d)
        j = i - d
        run = 0
        while i < len(R) and j < len(Q):
            if R[i] == Q[j] and R[i] in "ACGT":
                run += 1
            else:
                if run >= k:
                    out.append((i - run, j - run, run))
                run = 0
            i += 1
            j += 1
        if run >= k:
            out.append((i - run, j - run, run))
    return out


def centre(R: str, Q: str, k: int, w: int):
    """-> (rev, d0) or None.  Buckets of w diagonals, counted from the lowest diagonal -(|Q| - 1)."""
    if not R or not Q:
        return None
    per = []
    for rev in (0, 1):
        sd = seeds(R, revcomp(Q) if rev else Q, k)
        sums: Dict[int, int] = {}
        for i, j, ln in sd:
            b = (i - j + len(Q) - 1) // w
            sums[b] = sums.get(b, 0) + ln
        per.append((sd, sums))
    nb = (len(R) + len(Q) - 2) // w + 1
    best = None
    for rev in (0, 1):
        sums = per[rev][1]
        for b in range(nb):
            s = sums.get(b, 0) + sums.get(b + 1, 0)
            if s > 0 and (best is None or s > best[0]):   # ties: forward first, then the lower bucket
                best = (s, rev, b)
    if best is None:
        return None
    _, rev, b = best
    inside = [x for x in per[rev][0] if (x[0] - x[1] + len(Q) - 1) // w in (b, b + 1)]
    i, j, ln = min(inside, key=lambda x: (-x[2], x[0], x[0] - x[1]))   # longest, smallest i, lowest diagonal
    return rev, i - j


def score(p, r: str, q: str) -> int:
    if r not in "ACGT" or q not in "ACGT":
        return -1
    return p["a"] if r == q else -p["b"]


def align(R: str, Q: str, d0: int, p, stats: Optional[dict] = None) -> Optional[Tuple[int, int, str]]:
    """Banded local alignment around diagonal d0 -> (pos 0-based, score, CIGAR) or None.
    stats, if given, receives n_best: the number of cells that hold the best score."""
    w = p["w"]
    H: Dict[Tuple[int, int], int] = {}
    E: Dict[Tuple[int, int], int] = {}   # E[(i, j)]: the deletion state arriving at (i, j)
    D: Dict[Tuple[int, int], Tuple[int, bool, bool, bool]] = {}
    best, end, n_best = 0, None, 0
    for i in range(len(R)):
        f = NEG
        for j in range(max(0, i - d0 - w), min(len(Q), i - d0 + w + 1)):
            mm = H.get((i - 1, j - 1), 0) + score(p, R[i], Q[j])
            e = E.get((i, j), NEG)
            src, h = (0, mm) if mm >= e else (1, e)
            if not h >= f:
                src, h = 2, f
            stop = h <= 0
            H[(i, j)] = 0 if stop else h
            t = mm - p["o_del"] - p["e_del"]
            eext = e - p["e_del"] > t
            E[(i + 1, j)] = max(e - p["e_del"], t)
            t = mm - p["o_ins"] - p["e_ins"]
            fext = f - p["e_ins"] > t
            f = max(f - p["e_ins"], t)
            D[(i, j)] = (src, eext, fext, stop)
            if H[(i, j)] > best:
                best, end, n_best = H[(i, j)], (i, j), 0
            n_best += H[(i, j)] == best
    if stats is not None:
        stats["n_best"] = n_best if end is not None else 0
    if end is None:
        return None
    i, j = end
    ops: List[str] = []
    state = 0
    while (i, j) in D:
        src, eext, fext, stop = D[(i, j)]
        if state == 0:
            if stop:
                break
            state = src
        elif state == 1:
            state = 1 if eext else 0
        else:
            state = 2 if fext else 0
        ops.append("MDI"[state])
        if state != 2:
            i -= 1
        if state != 1:
            j -= 1
    ops.reverse()
    cigar = ""
    if j + 1 > 0:
        cigar += f"{j + 1}S"
    k = 0
    while k < len(ops):
        n = k
        while n < len(ops) and ops[n] == ops[k]:
            n += 1
        cigar += f"{n - k}{ops[k]}"
        k = n
    if len(Q) - 1 - end[1] > 0:
        cigar += f"{len(Q) - 1 - end[1]}S"
    return i + 1, best, cigar


def map_ref(R: str, Q: str, p) -> Optional[Tuple[int, int, int, str]]:
    """-> (strand, pos, score, CIGAR) or None, as proovread_amd.ccseq reports alignments."""
    c = centre(R, Q, p["k"], p["w"])
    if c is None:
        return None
    rev, d0 = c
    a = align(R, revcomp(Q) if rev else Q, d0, p)
    if a is None:
        return None
    return rev, a[0], a[1], a[2]


PARAMS = dict(k=9, w=300, a=5, b=11, o_del=2, o_ins=1, e_del=4, e_ins=3)


# ---------------------------------------------------------------------------
# simulated ZMWs (SURVEY.md §8d's CLR error model)

def noisy(rng: random.Random, s: str, ins=0.09, dele=0.045, sub=0.015) -> str:
    out = []
    for c in s:
        while rng.random() < ins:
            out.append(rng.choice("ACGT"))
        x = rng.random()
        if x < dele:
            continue
        out.append(rng.choice([b for b in "ACGT" if b != c]) if x < dele + sub else c)
    return "".join(out)


def sim_zmw(rng: random.Random, movie: str, hole: int, insert_len: int, passes: int, partial=True, rates=None,
            qual_range=(5, 20)):
    """-> (insert, [(id, seq, qual)]): alternating-strand passes of one insert; with `partial` the
    first and the last pass are cut to a random part of theirs."""
    insert = "".join(rng.choice("ACGT") for _ in range(insert_len))
    recs = []
    at = 0
    for k in range(passes):
        s = insert if k % 2 == 0 else revcomp(insert)
        if partial and passes > 2 and k == 0:
            s = s[rng.randrange(len(s) // 4, len(s) // 2):]
        if partial and passes > 2 and k == passes - 1:
            s = s[:rng.randrange(len(s) // 2, 3 * len(s) // 4)]
        s = noisy(rng, s, *(rates or ()))
        q = "".join(chr(33 + rng.randint(*qual_range)) for _ in s)
        recs.append((f"{movie}/{hole}/{at}_{at + len(s)}", s, q))
        at += len(s) + 40
    return insert, recs


def edit_distance(a: str, b: str) -> int:
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        ca = a[i - 1]
        for j in range(1, len(b) + 1):
            x = prev[j - 1] + (ca != b[j - 1])
            y = prev[j] + 1
            z = cur[j - 1] + 1
            cur[j] = x if x < y and x < z else (y if y < z else z)
        prev = cur
    return prev[-1]

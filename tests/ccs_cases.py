"""Groups and alignments the ccs consensus tests share — TEST INFRASTRUCTURE.

A case is a reference subread plus alignments given as (SEQ, QUAL, pos0, CIGAR) in arrival
order: hand-made ones that reach the corners of Sam::Seq's State_matrix under ccseq's settings,
and helpers that turn a case into the library's hook input and into a casefmt.Case for the
oracle and the Perl goldens.
"""
from __future__ import annotations

import random
import re
from typing import List, Tuple

import casefmt

Aln = Tuple[str, str, int, str]   # SEQ, QUAL (aligned orientation), 0-based POS, CIGAR


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def query_of(ref: str, pos: int, cigar: str, rng, ins=None) -> str:
    """The query a CIGAR spells against ref from pos: M copies, I inserts (`ins` strings in
    order, else random bases), S clips random bases."""
    out, r = [], pos
    ins = list(ins or [])
    for n, op in re.findall(r"(\d+)([MIDS])", cigar):
        n = int(n)
        if op == "M":
            out.append(ref[r:r + n])
            r += n
        elif op == "D":
            r += n
        elif op == "I":
            out.append(ins.pop(0) if ins else rand_seq(rng, n))
        else:
            out.append(rand_seq(rng, n))
    return "".join(out)


def q(n, c="?"):
    return c * n


def hand_cases():
    """name -> (ref seq, ref qual, [Aln]); the reference's qualities are low ('#': weight 0.03)
    unless a case needs otherwise."""
    rng = random.Random(77)
    cases = {}

    # an equal-weight tie between two insertion states at column 50: in the column AGG (first
    # alignment) precedes ATT (second), but ATT was seen first in the read (column 10)
    ref = list(rand_seq(rng, 120))
    ref[10] = ref[50] = "A"
    ref[11] = ref[51] = "C"
    ref = "".join(ref)
    a1 = query_of(ref, 0, "11M2I40M2I69M", rng, ["TT", "GG"])
    a2 = query_of(ref, 0, "51M2I69M", rng, ["TT"])
    cases["ins_tie_rank"] = (ref, q(120, "#"), [(a1, q(len(a1)), 0, "11M2I40M2I69M"), (a2, q(len(a2)), 0, "51M2I69M")])

    # Seq.pm:277: SEQ of 50 bases is not longer than StateMatrixMinAlnLength
    ref = rand_seq(rng, 150)
    short = ref[20:70]
    full = query_of(ref, 5, "140M", rng)
    cases["skip_277"] = (ref, q(150, "#"), [(short, q(50, "I"), 20, "50M"), (full, q(140), 5, "140M")])

    # Seq.pm:354: the clips leave 60 of 100 bases (< 70 %)
    c = "25S60M15S"
    s = query_of(ref, 40, c, rng)
    cases["skip_354"] = (ref, q(150, "#"), [(s, q(100, "I"), 40, c), (full, q(140), 5, "140M")])

    # Seq.pm:384: 701 of 1000 bases pass the head check; the taboo is 1, so the tail trim cuts
    # the last 1M and the 1I before it at the second M (the loop never looks at the first op):
    # 699 bases are left (< 70 %)
    ref2 = rand_seq(rng, 800)
    c = "299S350M1D349M1I1M"
    s = query_of(ref2, 30, c, rng, ["G"])
    full2 = query_of(ref2, 0, "800M", rng)
    cases["skip_384"] = (ref2, q(800, "#"), [(s, q(1000, "I"), 30, c), (full2, q(800), 0, "800M")])

    # a D+I pair becomes one replaced state with the insertion's qualities; a 1D1I is a mismatch
    ref = rand_seq(rng, 130)
    c = "40M2D3I30M1D1I57M"
    s = query_of(ref, 0, c, rng, ["TGA", "A" if ref[72] != "A" else "C"])
    ql = q(40, "5") + "I+I" + q(30, "5") + "I" + q(57, "5")
    cases["del_ins_pair"] = (ref, q(130, "#"), [(s, ql, 0, c)])

    # a leading insertion (and a leading deletion): the head trim removes both (Trim 1)
    c = "3I20M2D90M"
    s = query_of(ref, 4, c, rng, ["GGG"])
    c2 = "2M1D100M4I20M"
    s2 = query_of(ref, 2, c2, rng, ["ACAC"])
    cases["leading_ins"] = (ref, q(130, "#"), [(s, q(len(s)), 4, c), (s2, q(len(s2), "8"), 2, c2)])

    # deletions: the lesser neighbouring quality, the $qpos > 1 quirk at window position 1
    c = "1M2D60M3D1M1I59M"
    s = query_of(ref, 3, c, rng, ["T"])
    ql = "".join(chr(33 + (7 * k) % 41) for k in range(len(s)))
    cases["del_quals"] = (ref, "".join(chr(33 + (3 * k) % 30) for k in range(130)), [(s, ql, 3, c), (s, ql[::-1], 3, c)])

    # the reference alone: no alignment is usable; columns of weight 0 (quality '!') are uncovered
    rq = "".join("!" if k % 7 == 0 else "5" for k in range(130))
    cases["ref_alone"] = (ref, rq, [(short, q(50, "I"), 20, "50M")])
    return cases


def to_case(name: str, ref: str, rq: str, alns: List[Aln]) -> casefmt.Case:
    rid = f"m1/{len(name)}/0_{len(ref)}"
    sam = ["\t".join([f"q{k}", "0", rid, str(pos + 1), "60", cig, "*", "0", "0", s, ql, "AS:i:100"])
           for k, (s, ql, pos, cig) in enumerate(alns)]
    return casefmt.Case(name, {"qual_weighted": "1", "use_ref_qual": "1"}, ["@" + rid, ref, "+", rq], sam)


def case_alns(case: casefmt.Case) -> List[Aln]:
    out = []
    for ln in case.sam:
        f = ln.split("\t")
        out.append((f[9], f[10], int(f[3]) - 1, f[5]))
    return out


def to_group(ref: str, rq: str, alns: List[Aln]):
    """-> (Group, alignments) for ccseq.consensus_groups: the reference is subread 0, every
    alignment a forward subread."""
    grp = ([ref.encode()] + [a[0].encode() for a in alns], [rq.encode("latin-1")] + [a[1].encode("latin-1") for a in alns], 0)
    return grp, [None] + [(0, a[2], 100, a[3]) for a in alns]


ORACLE_OVER = dict(max_coverage=1e9, indel_taboo_length=0, indel_taboo=0.001, qual_weighted=1)

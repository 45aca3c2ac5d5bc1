"""Groups and alignments the ccs consensus tests share — TEST INFRASTRUCTURE.

A case is a reference subread plus alignments given as (SEQ, QUAL, pos0, CIGAR) in arrival
order, SEQ and QUAL in the aligned orientation; a fifth element 1 marks a subread sequenced from
the other strand: hand-made ones that reach the corners of Sam::Seq's State_matrix under ccseq's settings,
and helpers that turn a case into the library's hook input and into a casefmt.Case for the
oracle and the Perl goldens.

Further down, the cases built for the device kernels' edges, which the host tests and the
device tests share: pairs for the mapping (the band's scan over lanes, ties among seeds and
among cells), consensus groups on the edges of the kernel's tiles, and a batch of more groups
than one launch takes.  tests/test_ccs_host.py asserts that each reaches its edge.
"""
from __future__ import annotations

import functools
import itertools
import random
import re
from typing import List, NamedTuple, Tuple

import numpy as np

import casefmt
import ccs_ref

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


HAND_NAMES = ["ins_tie_rank", "skip_277", "skip_354", "skip_384", "del_ins_pair", "leading_ins", "del_quals", "ref_alone",
              "rev_ins_wins"]


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

    # column 40 holds two insertion states of three bases: the first alignment, from the reverse
    # strand (phred 33-47: weight >= 9.08), and the second (2-16: <= 2.13) carry one, the third
    # (17-31: 2.41 to 8.01) the other.  The second alone loses to the third; with the first it
    # wins, so the winning state is compared and written through the reverse strand's subread
    ref = rand_seq(rng, 80)
    ramp = lambda n, lo: "".join(chr(33 + lo + (7 * k) % 15) for k in range(n))   # noqa: E731
    r1 = query_of(ref, 1, "40M2I37M", rng, ["GT"])
    f2 = query_of(ref, 0, "41M2I35M", rng, ["GT"])
    f3 = query_of(ref, 3, "38M2I39M", rng, ["CC"])
    cases["rev_ins_wins"] = (ref, q(80, "#"), [(r1, ramp(len(r1), 33), 1, "40M2I37M", 1), (f2, ramp(len(f2), 2), 0, "41M2I35M"),
                                               (f3, ramp(len(f3), 17), 3, "38M2I39M")])
    return cases


def to_case(name: str, ref: str, rq: str, alns: List[Aln]) -> casefmt.Case:
    rid = f"m1/{len(name)}/0_{len(ref)}"
    sam = ["\t".join([f"q{k}", "16" if a[4:] == (1,) else "0", rid, str(a[2] + 1), "60", a[3], "*", "0", "0", a[0], a[1], "AS:i:100"])
           for k, a in enumerate(alns)]
    return casefmt.Case(name, {"qual_weighted": "1", "use_ref_qual": "1"}, ["@" + rid, ref, "+", rq], sam)


def case_alns(case: casefmt.Case) -> List[Aln]:
    out = []
    for ln in case.sam:
        f = ln.split("\t")
        out.append((f[9], f[10], int(f[3]) - 1, f[5]))
    return out


def to_group(ref: str, rq: str, alns: List[Aln]):
    """-> (Group, alignments) for ccseq.consensus_groups: the reference is subread 0, every
    alignment a subread, stored as sequenced."""
    sub = [(ccs_ref.revcomp(a[0]), a[1][::-1]) if a[4:] == (1,) else (a[0], a[1]) for a in alns]
    grp = ([ref.encode()] + [s.encode() for s, _ in sub], [rq.encode("latin-1")] + [ql.encode("latin-1") for _, ql in sub], 0)
    return grp, [None] + [(int(a[4:] == (1,)), a[2], 100, a[3]) for a in alns]


ORACLE_OVER = dict(max_coverage=1e9, indel_taboo_length=0, indel_taboo=0.001, qual_weighted=1)


# ---------------------------------------------------------------------------
# mapping cases: one subread against one reference, expected from ccs_ref.map_ref

class MapCase(NamedTuple):
    ref: str
    query: str
    over: dict   # the parameters that differ from ccs_ref.PARAMS


def ref_params(case: MapCase) -> dict:
    return dict(ccs_ref.PARAMS, **case.over)


def pair_group(case: MapCase):
    """-> the Group of the pair: the reference is subread 0, the query subread 1."""
    seqs = [case.ref.encode(), case.query.encode()]
    return seqs, [b"5" * len(s) for s in seqs], 0


_EXPECTED: dict = {}


def map_expected(case: MapCase):
    """ccs_ref.map_ref of the case, computed once per session (the wide bands take seconds)."""
    key = (case.ref, case.query, tuple(sorted(case.over.items())))
    if key not in _EXPECTED:
        _EXPECTED[key] = ccs_ref.map_ref(case.ref, case.query, ref_params(case))
    return _EXPECTED[key]


def cells_per_lane(w: int) -> int:
    """The run of band cells one lane of the alignment kernel holds: ceil((2 w + 2) / 64)."""
    return (2 * w + 2 + 63) // 64


def both_seeds(case: MapCase):
    """-> (forward seeds, reverse seeds) of the pair as ccs_ref.seeds lists them."""
    k = ref_params(case)["k"]
    return ccs_ref.seeds(case.ref, case.query, k), ccs_ref.seeds(case.ref, ccs_ref.revcomp(case.query), k)


def dshift(case: MapCase, seed) -> int:
    return seed[0] - seed[1] + len(case.query) - 1


def n_buckets(case: MapCase) -> int:
    return (len(case.ref) + len(case.query) - 2) // ref_params(case)["w"] + 1


def pair_sums(case: MapCase) -> dict:
    """(orientation, bucket) -> seed length sum of buckets b and b + 1, the positive ones."""
    w, out = ref_params(case)["w"], {}
    for rev, sd in enumerate(both_seeds(case)):
        sums: dict = {}
        for s in sd:
            sums[dshift(case, s) // w] = sums.get(dshift(case, s) // w, 0) + s[2]
        for b in range(n_buckets(case)):
            if sums.get(b, 0) + sums.get(b + 1, 0) > 0:
                out[(rev, b)] = sums.get(b, 0) + sums.get(b + 1, 0)
    return out


def _first(build, ok, start):
    """The case of the first random seed from `start` on that meets `ok`."""
    for seed in range(start, start + 500):
        case = build(random.Random(seed))
        if ok(case):
            return case
    raise AssertionError("no seed gives the case")


# A. the band: (w, length of the gap, length of each flank)
BANDS = [(31, 20, 120), (32, 20, 120), (63, 40, 120), (64, 40, 120), (300, 40, 120), (512, 150, 400)]
BAND_NAMES = [f"w{w}_{kind}" for w, _, _ in BANDS for kind in ("ins", "del", "rev")]


@functools.lru_cache(None)
def band_cases():
    """ref = rand(30) + A + B + rand(30) against A + gap + B (an insertion), the same with the
    gap in the reference (a deletion), and the insertion's reverse complement."""
    out = {}
    for w, n, fl in BANDS:
        rng = random.Random(1000 + w)
        a, b, gap, lf, rf = rand_seq(rng, fl), rand_seq(rng, fl), rand_seq(rng, n), rand_seq(rng, 30), rand_seq(rng, 30)
        out[f"w{w}_ins"] = MapCase(lf + a + b + rf, a + gap + b, {"w": w})
        out[f"w{w}_del"] = MapCase(lf + a + gap + b + rf, a + b, {"w": w})
        out[f"w{w}_rev"] = MapCase(lf + a + b + rf, ccs_ref.revcomp(a + gap + b), {"w": w})
    return out


def band_shape(name: str):
    """-> (w, gap length, the gap's CIGAR op, strand) of a band case."""
    w = int(name[1:name.index("_")])
    n = next(n for bw, n, _ in BANDS if bw == w)
    return w, n, "D" if name.endswith("_del") else "I", int(name.endswith("_rev"))


# (w, length of the flank before the gap); the gap is w long and the flank after it 20 longer.
# A gap of 300 bases in the reference loses to many short gaps through it, and so does every
# gap of 512: those are left out.
EDGE_BANDS = [(31, 100), (32, 100), (63, 100), (64, 100), (300, 200)]
EDGE_NAMES = [f"w{w}_{kind}" for w, _ in EDGE_BANDS for kind in (("ins", "del", "rev") if w < 300 else ("ins", "rev"))]


@functools.lru_cache(None)
def band_edge_cases():
    """As band_cases, but the gap is exactly w long and the flank after it is the longer one,
    so the band is centred on that flank's diagonal and the flank before the gap runs along the
    band's edge.  The insertion opens in the band's first cell, the start of lane 0's run, and
    its F crosses every run up to the centre; the deletion is entered from the band's last
    cell, whose E comes from the entry right of the band."""
    out = {}
    for w, fl in EDGE_BANDS:
        rng = random.Random(1500 + w)
        a, b, gap, lf, rf = rand_seq(rng, fl), rand_seq(rng, fl + 20), rand_seq(rng, w), rand_seq(rng, 30), rand_seq(rng, 30)
        out[f"w{w}_ins"] = MapCase(lf + a + b + rf, a + gap + b, {"w": w})
        if w < 300:
            out[f"w{w}_del"] = MapCase(lf + a + gap + b + rf, a + b, {"w": w})
        out[f"w{w}_rev"] = MapCase(lf + a + b + rf, ccs_ref.revcomp(a + gap + b), {"w": w})
    return out


OVERHANG_NAMES = [f"w{w}_{side}" for w in (31, 64) for side in ("end", "start")]


@functools.lru_cache(None)
def overhang_cases():
    """The match lies in the reference's last 60 bases and the query overhangs it by 40; the
    same at the reference's start."""
    rng = random.Random(2000)
    ref = rand_seq(rng, 200)
    end, start = ref[-60:] + rand_seq(rng, 40), rand_seq(rng, 40) + ref[:60]
    return {f"w{w}_{side}": MapCase(ref, q, {"w": w}) for w in (31, 64) for side, q in (("end", end), ("start", start))}


TIE_SCORES = dict(a=1, b=1, o_del=0, o_ins=0, e_del=1, e_ins=1, k=4, w=64)
TIE_NAMES = ["unrelated", "related"]


@functools.lru_cache(None)
def tie_cases():
    """A score set under which M, E and F tie all the time: two unrelated 150-mers, two related."""
    rng = random.Random(3000)
    x, y = rand_seq(rng, 150), rand_seq(rng, 150)
    z = (ccs_ref.noisy(rng, x, 0.05, 0.05, 0.05) + rand_seq(rng, 150))[:150]
    return {"unrelated": MapCase(x, y, dict(TIE_SCORES)), "related": MapCase(x, z, dict(TIE_SCORES))}


TANDEM_NAMES = ["w300", "w8"]


@functools.lru_cache(None)
def tandem_cases():
    """Three units of a six-unit tandem repeat: the best score is reached at four offsets."""
    rng = random.Random(4000)
    unit = rand_seq(rng, 50)
    ref = rand_seq(rng, 20) + unit * 6 + rand_seq(rng, 20)
    return {f"w{w}": MapCase(ref, unit * 3, {"w": w}) for w in (300, 8)}


# B. seeds
SEED_NAMES = ["orient_tie_w8", "orient_tie_w1", "key_tie_i", "key_tie_diag", "one_9mer", "one_8mer",
              "diag_255", "diag_256", "diag_257", "cand_254", "cand_256", "cand_258", "n_in_ref", "n_in_query"]
KEY_TIE_W = 8


def _beads(rng):
    """Three 8-mers joined by N: aligned to itself it scores 118, and no piece is a seed."""
    return "N".join(rand_seq(rng, 8) for _ in range(3))


def _key_tie(rng, by_i: bool):
    """Three seeds of 12 bases in one bucket of w = 8: (ACG)4 against (ACG)6 matches at three
    offsets.  by_i: the run of 18 is the reference's, so the seeds differ in i and the smallest
    wins; otherwise it is the query's, they share i, and the lowest diagonal wins.  Everything
    else is N, which seeds nothing, except a string of beads on a diagonal 10 from the winner's
    and within 8 of the losers': a band around a loser finds the beads (score 118), the band
    around the winner only the 12 bases (score 60)."""
    beads = _beads(rng)
    c, e, b = 7, 5, 6
    if by_i:   # seeds at (a, c), (a + 3, c), (a + 6, c): diagonals d, d + 3, d + 6; beads on d + 10
        q = "N" * c + "ACG" * 4 + "N" * 2 + beads + "N" * e
        low = lambda a: a - c                                     # noqa: E731
        ref = lambda a: "N" * a + "ACG" * 6 + "N" * 6 + beads + "N" * b   # noqa: E731
    else:      # seeds at (a, c), (a, c + 3), (a, c + 6): diagonals d, d - 3, d - 6; beads on d + 4
        q = "N" * c + "ACG" * 6 + "N" * 2 + beads + "N" * e
        low = lambda a: a - c - 6                                 # noqa: E731
        ref = lambda a: "N" * a + "ACG" * 4 + "N" * 12 + beads + "N" * b  # noqa: E731
    a = next(a for a in range(20, 40) if (low(a) + len(q) - 1) % KEY_TIE_W == 0)   # all three in one bucket
    return MapCase(ref(a), q, {"w": KEY_TIE_W})


def _kmer_case(rng, n):
    """The query shares ref[40:40 + n] with the reference, bounded by mismatches."""
    ref = rand_seq(rng, 80)
    lf, rf = rand_seq(rng, 30), rand_seq(rng, 30)
    lf = lf[:-1] + next(c for c in "ACGT" if c != ref[39])
    rf = next(c for c in "ACGT" if c != ref[40 + n]) + rf[1:]
    return MapCase(ref, lf + ref[40:40 + n] + rf, {"w": 8})


def _n_case(rng, in_ref: bool):
    """A 20-base match with an N at its 11th base, in the reference or in the query."""
    ref = rand_seq(rng, 120)
    lf, rf = rand_seq(rng, 30), rand_seq(rng, 30)
    lf = lf[:-1] + next(c for c in "ACGT" if c != ref[49])
    rf = next(c for c in "ACGT" if c != ref[70]) + rf[1:]
    q = lf + ref[50:70] + rf
    if in_ref:
        ref = ref[:60] + "N" + ref[61:]
    else:
        q = q[:40] + "N" + q[41:]
    return MapCase(ref, q, {"w": 8})


def _n_seeds(case):
    f, r = both_seeds(case)
    return len(f) + len(r)


@functools.lru_cache(None)
def seed_cases():
    out = {}
    rng = random.Random(5000)
    x = rand_seq(rng, 60)
    pal = x + ccs_ref.revcomp(x)   # its own reverse complement: both orientations vote alike
    ref = rand_seq(rng, 40) + pal + rand_seq(rng, 40)
    out["orient_tie_w8"] = MapCase(ref, pal, {"w": 8})
    out["orient_tie_w1"] = MapCase(ref, pal, {"w": 1})   # 2 * 319 candidates: each thread sees both orientations
    out["key_tie_i"] = _first(lambda r: _key_tie(r, True), lambda c: _n_seeds(c) == 5, 5100)
    out["key_tie_diag"] = _first(lambda r: _key_tie(r, False), lambda c: _n_seeds(c) == 5, 5200)
    out["one_9mer"] = _first(lambda r: _kmer_case(r, 9), lambda c: _n_seeds(c) == 1, 5300)
    out["one_8mer"] = _first(lambda r: _kmer_case(r, 8), lambda c: _n_seeds(c) == 0, 5400)
    # lr + lq - 1 diagonals at, under and over the seeds kernel's block of 256 threads
    base = rand_seq(rng, 130)
    sub = lambda s, at: s[:at] + next(c for c in "ACGT" if c != s[at]) + s[at + 1:]   # noqa: E731
    out["diag_255"] = MapCase(base[:128], sub(sub(base[:128], 40), 90), {"w": 8})
    out["diag_256"] = MapCase(base[:128], ccs_ref.revcomp(sub(base[:129], 64)), {"w": 8})
    out["diag_257"] = MapCase(base[:128], sub(base[:130], 30), {"w": 8})
    # 2 * n_buckets candidates around it: w = 1 makes a bucket of every diagonal
    short = rand_seq(rng, 70)
    out["cand_254"] = MapCase(short, short[5:63], {"w": 1})
    out["cand_256"] = MapCase(short, ccs_ref.revcomp(short[5:64]), {"w": 1})
    out["cand_258"] = MapCase(short, ccs_ref.revcomp(short[3:63]), {"w": 1})
    out["n_in_ref"] = _first(lambda r: _n_case(r, True), lambda c: _n_seeds(c) == 2, 5500)
    out["n_in_query"] = _first(lambda r: _n_case(r, False), lambda c: _n_seeds(c) == 2, 5600)
    return out


# ---------------------------------------------------------------------------
# C. consensus cases

# name -> (reference length, deleted columns, columns that carry a two-base insertion).  A block
# of the consensus kernel decides 256 columns at a time and carries the lengths written so far
# into the next 256; the last column of an alignment cannot hold either (the trim cuts it), nor
# can the last two from 500 bases on, where the taboo is one base.
TILES = {
    "L255_del250_ins252": (255, (250,), (252,)),
    "L256_del252_ins254": (256, (252,), (254,)),
    "L257_del255_ins252": (257, (255,), (252,)),
    "L257_del250_ins255": (257, (250,), (255,)),
    "L512_del255_ins509": (512, (255,), (509,)),
    "L512_del100_ins256": (512, (100,), (256,)),
    "L513_del255_ins510": (513, (255,), (510,)),
    "L260_del255_ins256": (260, (255,), (256,)),   # the last column of one tile, the first of the next
    "L516_del511_ins512": (516, (511,), (512,)),
}


def tile_case(name: str):
    """Three identical alignments of quality 'I' over the whole reference of quality '#': they
    decide a gap in the deleted columns and a three-base state (the base and two inserted ones)
    in the insertion columns."""
    L, dels, inss = TILES[name]
    rng = random.Random(6000 + L)
    ref = rand_seq(rng, L)
    ops, query = [], []
    for c in range(L):
        if c in dels:
            ops.append("D")
            continue
        ops.append("M")
        query.append(ref[c])
        if c in inss:
            ops += "II"
            query.append(rand_seq(rng, 2))
    cigar = "".join(f"{len(list(grp))}{op}" for op, grp in itertools.groupby(ops))
    query = "".join(query)
    return ref, q(L, "#"), [(query, q(len(query), "I"), 0, cigar)] * 3


def tile_trace(name: str) -> str:
    L, dels, inss = TILES[name]
    return "".join("I" if c in dels else "MDD" if c in inss else "M" for c in range(L))


MANY_OPS_CIGAR = "2M1I2M1D" * 150 + "20M"


def many_ops_case():
    """One alignment of 601 CIGAR ops next to a plain one over the whole reference."""
    rng = random.Random(6100)
    ref = rand_seq(rng, 1000)
    s = query_of(ref, 100, MANY_OPS_CIGAR, rng)
    return ref, q(1000, "#"), [(s, q(len(s)), 100, MANY_OPS_CIGAR), (ref, q(1000, "5"), 0, "1000M")]


def kept_ops(cigar: str, qlen: int, taboo_frac=0.001) -> int:
    """The CIGAR ops State_matrix keeps of an alignment (Seq.pm:316-385): the clips go, the head
    up to the first M that carries the bases past the taboo, the tail likewise."""
    ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDS])", cigar) if op != "S"]
    taboo = int(qlen * taboo_frac + 0.5)
    cb, ce, seen = 0, len(ops), 0
    for i, (n, op) in enumerate(ops):
        if op == "M" and seen + n > taboo:
            cb = i
            break
        seen += n if op != "D" else 0
    tail = 0
    for i in range(len(ops) - 1, cb, -1):
        n, op = ops[i]
        tail += n if op != "D" else 0
        if op == "M" and tail > taboo:
            ce = i + 1
            break
    return ce - cb


BAD_ALNS = ["139M", "140M6D", "70M3S67M", "150M", "140N", "over_slot"]


def malformed_batch(hand, bad: str):
    """-> (groups, alignments, over_slot): skip_277's group with its second alignment replaced
    by a malformed one, between the groups of del_ins_pair and leading_ins.  over_slot lists
    the (group, subread) whose CIGAR count is to pass its slot (consensus_raw)."""
    packed = [to_group(*hand[name]) for name in ("del_ins_pair", "skip_277", "leading_ins")]
    groups, alns = [g for g, _ in packed], [list(ga) for _, ga in packed]
    if bad == "over_slot":
        return groups, alns, ((1, 2),)
    alns[1][2] = (0, 20 if bad == "150M" else 5, 100, bad)
    return groups, alns, ()


def consensus_raw(groups, alns, over_slot=(), device=False, ctx=None):
    """ccseq.consensus_groups with the CIGAR counts of over_slot's subreads raised past their
    slots, which the hook itself refuses to pack."""
    import ctypes as C

    from proovread_amd import _abi, ccseq
    A = ccseq._Arrays(groups)
    A.set_alignments(alns)
    for g, t in over_slot:
        s = int(A.grp_off[g]) + t
        A.n_cigar[s] = A.cig_off[s + 1] - A.cig_off[s] + 1
    p = ccseq.default_params()
    c = ccseq._ctx(device, ctx)
    _abi.check(ccseq._lib().pr_ccs_cns(ccseq._handle(c), C.byref(p), C.byref(A.batch), 0, C.byref(A.alns), C.byref(A.out)),
               "pr_ccs_cns")
    return A.results()


def zmw_case(ids, grp, alns) -> casefmt.Case:
    """A mapped group as the oracle's case: its alignments as SAM lines in arrival order."""
    from proovread_amd import ccseq
    seqs, quals, ref = grp
    return casefmt.Case("zmw", {"qual_weighted": "1", "use_ref_qual": "1"},
                        ["@" + ids[ref], seqs[ref].decode(), "+", quals[ref].decode()], ccseq.sam_lines(ids, grp, alns))


def exact_len_zmw(rng, n, passes, zmw="m2/1"):
    """-> (ids, Group): `passes` alternating-strand subreads of exactly n bases each; the
    reference is the second (ccseq:356-363)."""
    insert = rand_seq(rng, n + n // 4 + 200)
    ids, seqs, quals, at = [], [], [], 0
    for k in range(passes):
        s = ccs_ref.noisy(rng, insert if k % 2 == 0 else ccs_ref.revcomp(insert), 0.02, 0.01, 0.005)
        s = s[:n] if k % 2 == 0 else s[-n:]
        assert len(s) == n
        ids.append(f"{zmw}/{at}_{at + n}")
        seqs.append(s.encode())
        quals.append("".join(chr(33 + rng.randint(5, 20)) for _ in s).encode())
        at += n + 40
    return ids, (seqs, quals, 1)


def full_house():
    """A group of MAX_SUBREADS subreads of 300 bases: 63 column maps of more than one tile each."""
    return exact_len_zmw(random.Random(6200), 300, 64)


# ---------------------------------------------------------------------------
# D. more groups and pairs than one launch takes

CHUNK_GROUPS, CHUNK_LEN = 65540, 60
_SUBST = bytes.maketrans(b"ACGT", b"CGTA")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@functools.lru_cache(None)
def chunk_groups():
    """65,540 groups of two 60-base subreads: the first a slice of one random string, the second
    (the reference) the first with one substitution, in every third group reverse-complemented."""
    n, ln = CHUNK_GROUPS, CHUNK_LEN
    big = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(7000).integers(0, 4, size=n * ln)].tobytes()
    qual = b"5" * ln
    groups = []
    for g in range(n):
        a = big[g * ln:(g + 1) * ln]
        at = 5 + g % (ln - 10)   # far enough from the ends that a clip never pays
        b = a[:at] + a[at:at + 1].translate(_SUBST) + a[at + 1:]
        if g % 3 == 2:
            b = b.translate(_COMP)[::-1]
        groups.append(([a, b], [qual, qual], 1))
    return groups


@functools.lru_cache(None)
def chunk_host():
    """-> (results, alignments) of the chunk batch on the host path, computed once per session."""
    from proovread_amd import ccseq
    results, alns, _ = ccseq.run_groups(chunk_groups(), ccseq.default_params(w=8), device=False, threads=8)
    return results, alns

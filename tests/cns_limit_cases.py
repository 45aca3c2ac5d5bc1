"""Inputs at the consensus kernel's per-read limits and with alignments that span
several pileup windows, for tests/test_cns_limits_gpu.py: seeded generators of casefmt.Case, and
a plain Python walk over SAM lines that counts insertion states, so that a case's state and pair
counts are known without asking the code under test."""
import itertools
import random

import casefmt

W = 1024   # columns of a pileup window


def rand_seq(rng, n):
    return "".join(rng.choices("ACGT", k=n))


def ops_with(span, events):
    """CIGAR ops of an alignment over `span` reference columns with indels at column offsets:
    (o, "I", string) inserts the string after the alignment's column o, (o, "D", k) deletes its
    columns o .. o + k - 1.  Returns (ops, inserted strings in order)."""
    ops, strings, at = [], [], 0
    for o, kind, v in sorted(events):
        m = (o + 1 if kind == "I" else o) - at
        assert m > 0, (o, kind, at)
        ops.append(("M", m))
        if kind == "I":
            ops.append(("I", len(v)))
            strings.append(v)
            at = o + 1
        else:
            ops.append(("D", v))
            at = o + v
    assert span > at
    ops.append(("M", span - at))
    return ops, strings


def sam_line(name, rid, ref, start0, ops, score, strings=(), rng=None):
    """A SAM line: M copies the reference, I takes the next of `strings`, S is random."""
    seq, r, it = [], start0, iter(strings)
    for op, n in ops:
        if op == "M":
            seq.append(ref[r:r + n])
            r += n
        elif op == "D":
            r += n
        elif op == "I":
            s = next(it)
            assert len(s) == n
            seq.append(s)
        else:
            seq.append(rand_seq(rng, n))
    assert r <= len(ref)
    sq = "".join(seq)
    cig = "".join(f"{n}{op}" for op, n in ops)
    return f"{name}\t0\t{rid}\t{start0 + 1}\t60\t{cig}\t*\t0\t0\t{sq}\t{'I' * len(sq)}\tAS:i:{score}"


def make(name, ref, placed, **params):
    """placed: (start0, SAM line) pairs; the case lists them in coordinate order (stable)."""
    sam = [l for _, l in sorted(placed, key=lambda t: t[0])]
    return casefmt.Case(name, {k: str(v) for k, v in params.items()}, [f"@{name}", ref, "+", "$" * len(ref)], sam)


# ------------------------------------------------------------------------------------------
# the Python walk
def fields(line):
    f = line.split("\t")
    ops = [(int(n), op) for n, op in casefmt_cigar(f[5])]
    return int(f[3]) - 1, ops, f[9]


def casefmt_cigar(cig):
    n = ""
    for ch in cig:
        if ch.isdigit():
            n += ch
        else:
            yield n, ch
            n = ""


def ins_states(line, margin=8):
    """(column, state string) of every insertion of a SAM line that lies at least `margin` read
    bases from either end of the aligned part of SEQ (the taboo trim cuts indels nearer than
    that; this only approximates it).  The state of an insertion after a matched base is that
    base plus the inserted ones; after a deletion it is the inserted bases alone."""
    start0, ops, seq = fields(line)
    q0 = ops[0][0] if ops[0][1] == "S" else 0
    q1 = len(seq) - (ops[-1][0] if ops[-1][1] == "S" else 0)
    col, q, prev = start0, 0, None
    for n, op in ops:
        if op == "M":
            col += n
            q += n
        elif op == "D":
            col += n
        elif op == "S":
            q += n
        elif op == "I":
            if q - q0 >= margin and q1 - (q + n) >= margin and prev in ("M", "D"):
                yield col - 1, (seq[q - 1:q + n] if prev == "M" else seq[q:q + n])
            q += n
        if op != "I":
            prev = op


def kept_lines(case, kept):
    return [l for l, k in zip(case.sam, kept) if k == "1"]


def n_states(lines):
    return len({s for l in lines for _, s in ins_states(l)})


def window_pairs(lines):
    """window -> number of distinct (column, state) pairs in it"""
    out = {}
    for c, s in {cs for l in lines for cs in ins_states(l)}:
        out[c // W] = out.get(c // W, 0) + 1
    return out


def center_bin(line, bin_size=20):
    """Sam::Seq's bin of an alignment: int((POS + length / 2) / bin size), its length being that
    of SEQ, or the M and D columns if it is soft-clipped."""
    start0, ops, seq = fields(line)
    clipped = ops[0][1] == "S" or ops[-1][1] == "S"
    n = sum(k for k, op in ops if op in "MD") if clipped else len(seq)
    return int((start0 + 1 + n / 2) / bin_size)


# ------------------------------------------------------------------------------------------
# the cases
def ordinary(rng, rid, ref, starts, tag="o", events=None):
    """150M alignments at `starts` (exact copies of the reference, AS 300 .. 499); events:
    start0 -> indel events for ops_with."""
    out = []
    for k, s in enumerate(starts):
        ops, strings = ops_with(150, events(s) if events else [])
        out.append((s, sam_line(f"{tag}{k}", rid, ref, s, ops, 300 + rng.randrange(200), strings)))
    return out


def spread_case(name, L, n, seed):
    """n 150 bp alignments spread over a read of L bases, the first and the last column covered;
    every fifth carries an insertion or a deletion."""
    rng = random.Random(seed)
    ref = rand_seq(rng, L)
    starts = [0, L - 150] + [rng.randrange(0, L - 150) for _ in range(n - 2)]
    ev = lambda s: [] if s % 5 else ([(70, "I", rand_seq(rng, 3))] if s % 2 else [(80, "D", 2)])
    return make(name, ref, ordinary(rng, name, ref, starts, events=ev))


def stack_case(n):
    """n identical 60M alignments (equal AS) on the same 60 columns of a 300 bp read; the
    coverage is set so high that the bin cap keeps all of them."""
    rng = random.Random(11)
    name = f"stack_{n}"
    ref = rand_seq(rng, 300)
    line = sam_line("s", name, ref, 100, [("M", 60)], 250)
    return casefmt.Case(name, {"coverage": "1e7"}, [f"@{name}", ref, "+", "$" * 300], [line] * n)


SPAN_RP = 1000


def span_case(ns):
    """A 6 kb read with one alignment of ns states from column 1000 on: 2000M 3D 2078M 4I and a
    last M of ns - 4081 (14 or more: past the taboo trim), so the insertion state has state index
    4080.  About 300 exact 150M alignments lie over it, none of them on the columns around the
    insertion, where the long alignment alone decides the consensus."""
    rng = random.Random(12)
    name = f"span_{ns}"
    L = 6000
    ref = rand_seq(rng, L)
    ops = [("M", 2000), ("D", 3), ("M", 2078), ("I", 4), ("M", ns - 4081)]
    icol = SPAN_RP + 4080
    lbin = int((SPAN_RP + 1 + 4096 / 2) / 20)   # the long alignment's bin stays its own (the bin cap)
    starts = []
    while len(starts) < 300:
        s = rng.randrange(0, L - 150)
        if (s + 150 <= icol - 20 or s >= icol + 20) and int((s + 1 + 75) / 20) != lbin:
            starts.append(s)
    placed = ordinary(rng, name, ref, starts)
    placed.append((SPAN_RP, sam_line("long", name, ref, SPAN_RP, ops, 20000, ["TGCA"])))
    return make(name, ref, placed, coverage=50)


def qoff_case():
    """An alignment whose soft clip of 65,536 bases puts its insertions at SEQ offsets beyond 16
    bits (three insertions of 60,000 bases keep 73 % of SEQ aligned, so the trim does not skip
    it), over a few ordinary alignments."""
    rng = random.Random(13)
    name = "qoff_over"
    ref = rand_seq(rng, 1000)
    ops = [("S", 65536), ("M", 100)] + [("I", 60000), ("M", 100)] * 3
    placed = ordinary(rng, name, ref, [rng.randrange(0, 850) for _ in range(20)])
    placed.append((200, sam_line("clip", name, ref, 200, ops, 2000, [rand_seq(rng, 60000) for _ in range(3)], rng)))
    return make(name, ref, placed, coverage=50)


def states_case(n):
    """Exactly n distinct insertion states: 150M alignments starting at multiples of 15 with an
    insertion after every 15th base (up to nine each), always after a reference 'A', every
    insertion a 6-mer of its own."""
    rng = random.Random(14)
    name = f"states_{n}"
    L = 3000
    ref = list(rand_seq(rng, L))
    for c in range(14, L, 15):
        ref[c] = "A"
    ref = "".join(ref)
    mers = ["".join(t) for t in itertools.product("ACGT", repeat=6)]
    rng.shuffle(mers)
    assert n <= len(mers)
    placed, left, k = [], n, 0
    while left:
        m = min(9, left)
        s = 15 * rng.randrange(0, (L - 150) // 15 + 1)
        ops, strings = ops_with(150, [(14 + 15 * j, "I", mers.pop()) for j in range(m)])
        placed.append((s, sam_line(f"i{k}", name, ref, s, ops, 300 + rng.randrange(200), strings)))
        left -= m
        k += 1
    return make(name, ref, placed, coverage=10000)


def pairs_case():
    """600 alignments over 1,150 columns, each with a random 3-base insertion after every second
    base: 256 possible states, tens of thousands of (column, state) pairs in window 0."""
    rng = random.Random(15)
    name = "pairs_over"
    ref = rand_seq(rng, 1500)
    placed = []
    for k in range(600):
        s = rng.randrange(0, 1000)
        ops, strings = ops_with(150, [(1 + 2 * j, "I", rand_seq(rng, 3)) for j in range(74)])
        placed.append((s, sam_line(f"p{k}", name, ref, s, ops, 300 + rng.randrange(200), strings)))
    return make(name, ref, placed, coverage=10000)


CHIM_LOW = (30, 31)           # the bins without alignments: the chimera candidate
CHIM_MF, CHIM_MT = 580, 659   # its compared columns, (30 - 1) * 20 .. (31 + 2) * 20 - 1
CHIM_LEFT = (26, 30)          # bins of the left side's alignments, (30 - 4) .. and of the right:
CHIM_RIGHT = (32, 36)


def chim_case(overflow):
    """A chimeric read in the style of make_cns_cases.make_case(chimera=True), laid out by hand:
    four 150M alignments centred in every bin but 30 and 31, the ones right of the gap carrying
    another haplotype on columns 625 .. 699.  Sixteen alignments (eight per side) carry an
    insertion after column 620, all different but one shared between the sides, five one after
    column 640.  overflow: the left side's alignments carry a 4-base insertion after every column
    of the compared window instead (and a soft-clipped base, so that their length, and with it
    their bin, is that of their 150 columns)."""
    rng = random.Random(16)
    name = "chim_over" if overflow else "chim_scan"
    L = 1400
    ref, src2 = rand_seq(rng, L), rand_seq(rng, L)
    hap = ref[:625] + src2[625:700] + ref[700:]
    tri = ["".join(t) for t in itertools.product("ACGT", repeat=3)]
    rng.shuffle(tri)
    tri.remove("GAT")
    tri.remove("TTC")
    placed, at640 = [], 0
    for b in range(4, 66):
        if b in CHIM_LOW:
            continue
        for j, off in enumerate((1, 6, 11, 16)):
            s = 20 * b - 76 + off
            ev = []
            if overflow:
                if CHIM_LEFT[0] <= b <= CHIM_LEFT[1]:
                    ev = [(c - s, "I", rand_seq(rng, 4)) for c in range(CHIM_MF, CHIM_MT + 1) if 10 <= c - s < 140]
            else:
                if b in (28, 29, 32, 33):
                    shared = (b, j) in ((28, 0), (32, 0))
                    ev.append((620 - s, "I", "GAT" if shared else tri.pop()))
                if b in (29, 32) and j < 3 and at640 < 5:
                    ev.append((640 - s, "I", "TTC" if j == 0 else tri.pop()))
                    at640 += 1
            ops, strings = ops_with(150, ev)
            if overflow and ev:
                ops = [("S", 1)] + ops
            base = hap if b >= CHIM_RIGHT[0] else ref
            placed.append((s, sam_line(f"c{b}_{j}", name, base, s, ops, 400 + rng.randrange(300), strings, rng)))
    return make(name, ref, placed, coverage=25, detect_chimera=1, use_ref_qual=0)


SPANS = ((1100, ((2, 0), (3, -1), (4, 1))), (2100, ((3, 0), (5, -1), (7, 1))),
         (3100, ((4, 0), (6, -1), (8, 1))), (4095, ((6, 0), (7, -1), (8, 1))))
SPANS_GAPS = ((102,), (153, 154))   # bins left without alignments: chimera candidates at windows 1|2, 2|3


def spans_case(detect_chimera):
    """An 8.3 kb read under alignments of 1,100, 2,100, 3,100 and 4,095 columns that end exactly
    on, one before and one after a multiple of 1,024, ten of 161 .. 1,000 columns, and one 150M
    alignment per remaining bin.  Every alignment that covers a window boundary B by ten columns
    or more on both sides carries, at odd B / 1024, an insertion after column B - 1 and one after
    column B, at even B / 1024 a deletion of columns B - 2 .. B + 1."""
    rng = random.Random(17)
    name = "spans_chim" if detect_chimera else "spans"
    L = 8300
    ref = rand_seq(rng, L)
    ins = {k: (rand_seq(rng, 2 + k % 3), rand_seq(rng, 1 + k % 2)) for k in range(1, 9)}

    def events(s, span):
        ev = []
        for k in range(1, L // W + 1):
            B = k * W
            if B - 2 - s < 10 or s + span - (B + 2) < 10:
                continue
            if k % 2:
                ev += [(B - 1 - s, "I", ins[k][0]), (B - s, "I", ins[k][1])]
            else:
                ev.append((B - 2 - s, "D", 4))
        return ev

    placed, taken = [], set(b for g in SPANS_GAPS for b in g)
    longs = [(W * k + d - span, span) for span, ends in SPANS for k, d in ends]
    longs += [(None, span) for span in (161, 161, 200, 250, 400, 400, 700, 700, 1000, 1000)]
    for n, (s, span) in enumerate(longs):
        while True:   # a bin of its own: the bin cap keeps it
            s1 = rng.randrange(200, L - 1200) if s is None else s
            ops, strings = ops_with(span, events(s1, span))
            line = sam_line(f"w{n}", name, ref, s1, ops, 5 * span, strings)
            b = center_bin(line)
            if b not in taken:
                break
            assert s is None, (s, span, b)
        taken.add(b)
        placed.append((s1, line))
    for b in range(4, L // 20 - 4):
        if b in taken:
            continue
        s = 20 * b - 76 + rng.randrange(1, 20)
        ops, strings = ops_with(150, events(s, 150))
        # (an insertion shifts the centre by a base or two: keep it off the neighbours' bins)
        line = sam_line(f"o{b}", name, ref, s, ops, 300 + rng.randrange(200), strings)
        if center_bin(line) in taken:
            continue
        placed.append((s, line))
    return make(name, ref, placed, coverage=30, detect_chimera=int(detect_chimera), use_ref_qual=0)

"""Deterministic generator of the unitig consensus cases (tests/golden/utg_cases.txt.gz, written by regen_utg.sh): one read
each, a few hundred to a few thousand columns, built so that every two alignments of a read have
different Sam::Alignment lengths (the reference's result then cannot depend on Perl's hash order).

    python make_utg_cases.py out_cases.txt
"""
import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]
from utg_cases import Case, aln_length, noisy_ops, rand_qual, rand_seq, sam_line, write_cases  # noqa: E402

FULL = "--utg-mode --qual-weighted --fallback-phred 30 --coverage 1 --rep-coverage 7 --min-ncscore 3.3"


class Builder:
    def __init__(self, seed: int, name: str, L: int, desc: str = "", fasta: bool = False):
        self.rng = random.Random(seed)
        self.name, self.L = name, L
        self.rid = "lr_" + name
        self.ref = rand_seq(self.rng, L)
        self.head = self.rid + (" " + desc if desc else "")
        self.qual = None if fasta else rand_qual(self.rng, L, 2, 30)
        self.sam = []

    def add(self, start, span, score, indel=0.02, mism=0.03, qual=None, ops=None, ins=None):
        ops = ops or noisy_ops(self.rng, span, indel)
        self.sam.append(sam_line(self.rng, f"u{len(self.sam)}", self.rid, self.ref, start, ops, score, mism, qual, ins))

    def stack(self, at, n, span0=52, score=400):
        """n short hits over [at, at + span0 + n): spans span0, span0 + 1, ..."""
        for k in range(n):
            self.add(at + (k % 3), span0 + k, score + k, indel=0.0)

    def case(self, flags, cfg=""):
        lens = [aln_length(s) for s in self.sam]
        assert len(set(lens)) == len(lens), (self.name, sorted(lens))
        if "--qual-weighted" not in flags:          # the hits' qualities are never read: QUAL '*'
            self.sam = ["\t".join(f[:10] + ["*"] + f[11:]) for f in (x.split("\t") for x in self.sam)]
        ref = [">" + self.head, self.ref] if self.qual is None else ["@" + self.head, self.ref, "+", self.qual]
        return Case(self.name, flags, cfg, ref, self.sam)


def run_of(spans, L, cmax):
    """The first run of columns covered by at least cmax of the (start, span) hits."""
    cov = [0] * (L + 1)
    for st, sp in spans:
        for c in range(st, st + sp):
            cov[c] += 1
    s = next(c for c in range(L) if cov[c] >= cmax)
    e = next(c for c in range(s, L + 1) if cov[c] < cmax)
    return s, e


def main(out):
    cases = []
    # hits are staggered: none lies inside another once shortened by 10 % at both ends, unless
    # the contained filter is what the case is about

    b = Builder(1, "qual_weighted", 400)          # also: --utg-mode without --rep-coverage, step 4 without step 2
    b.add(0, 220, 1100), b.add(90, 230, 1200), b.add(190, 210, 1000)
    cases.append(b.case("--utg-mode --qual-weighted"))

    b = Builder(2, "rep_coverage", 700)           # step 4 with step 2: a stack in the middle, long hits over it
    b.add(0, 400, 2000), b.add(301, 399, 2100), b.stack(330, 5)
    cases.append(b.case("--utg-mode --rep-coverage 3"))

    b = Builder(3, "min_ncscore", 500)
    b.add(0, 250, 1250), b.add(150, 300, 600), b.add(50, 230, 740), b.add(100, 150, None), b.add(30, 60, 330)
    b.add(220, 280, 1400)
    cases.append(b.case("--utg-mode --min-ncscore 3.3"))

    b = Builder(4, "fallback_phred", 400)         # QUAL * and real QUAL mixed
    b.add(0, 220, 1100, qual="*"), b.add(90, 230, 1200), b.add(190, 210, 1000, qual="*")
    cases.append(b.case("--utg-mode --qual-weighted --fallback-phred 30"))

    b = Builder(5, "invert_scores", 450)          # blasr's negative AS
    b.add(0, 260, -1560), b.add(80, 240, -500), b.add(190, 259, -1350), b.add(150, 201, 1000)
    cases.append(b.case("--utg-mode --invert-scores --min-ncscore 3.3"))

    b = Builder(6, "full_set", 900)               # proovread's flags, blasr scores
    b.add(0, 550, -2700), b.add(350, 540, -2600), b.add(120, 300, -1450, qual="*"), b.add(450, 200, -150)
    b.stack(250, 8, score=-400), b.stack(700, 7, span0=70, score=-50)
    cases.append(b.case(FULL + " --invert-scores"))

    b = Builder(7, "fasta_ref", 500, desc="MCR0:50,100", fasta=True)
    b.add(0, 380, 1800), b.add(110, 370, 1900), b.stack(220, 4)
    cases.append(b.case("--utg-mode --qual-weighted --rep-coverage 4"))

    b = Builder(8, "mcr_plus_windows", 700, desc="SUBSTR:0,700 MCR0:60,40 MCR1:350,30")
    b.add(0, 450, 2000), b.add(180, 480, 2100), b.add(300, 230, 1000), b.stack(560, 3, span0=60)
    cases.append(b.case("--utg-mode --qual-weighted --rep-coverage 3"))

    b = Builder(9, "ignore_hcr", 400, desc="MCR0:50,40")
    b.add(0, 250, 1200), b.add(100, 260, 1300)
    cases.append(b.case("--utg-mode --qual-weighted --ignore-hcr"))

    # a window clamped at column 0 that swallows whole hits.  u6 ends one column before the
    # window does and goes; u7 ends on the window's last column counted from 0 and stays,
    # because POS is 1-based
    b = Builder(10, "rep_clamp_start", 700)
    b.stack(30, 6, span0=55)
    s, e = run_of([(30 + (k % 3), 55 + k) for k in range(6)], 700, 4)
    wend = e + 150                                # the window is [0, e + 150)
    b.add(wend - 1 - 62, 62, 300, indel=0.0), b.add(wend - 61, 61, 310, indel=0.0), b.add(230, 450, 2200)
    cases.append(b.case("--utg-mode --rep-coverage 4"))

    # a window over the read's end: shortened by 1, not by the overhang, so a hit that ends on the
    # last column (u7) is still swallowed
    b = Builder(11, "rep_clamp_end", 500)
    b.add(0, 380, 1800), b.stack(410, 6, span0=58), b.add(500 - 75, 75, 300, indel=0.0)
    cases.append(b.case("--utg-mode --rep-coverage 4"))

    # the contained filter: very short hits (< 21), hits of almost identical length with the swap
    # by score both ways, long hits
    b = Builder(12, "contained_classes", 900)
    b.add(0, 500, 2400, indel=0.0), b.add(380, 480, 2300, indel=0.0)
    b.add(150, 15, 60, indel=0.0), b.add(600, 18, 70, indel=0.0), b.add(880, 20, 80, indel=0.0)
    b.add(100, 300, 1400, indel=0.0), b.add(770, 121, 500, indel=0.0)
    b.add(600, 100, 500, indel=0.0), b.add(595, 112, 300, indel=0.0)
    b.add(200, 101, 200, indel=0.0), b.add(195, 113, 400, indel=0.0)
    b.add(400, 140, 900, indel=0.0), b.add(398, 150, 100, indel=0.0)
    cases.append(b.case("--utg-mode"))

    b = Builder(13, "d_plus_i", 400)              # 1D1I instead of a mismatch, D followed by two I
    b.add(0, 240, 1100, ops=[(60, "M"), (1, "D"), (1, "I"), (90, "M"), (2, "D"), (2, "I"), (1, "I"), (87, "M")])
    b.add(90, 241, 1000, ops=[(40, "M"), (1, "D"), (1, "I"), (199, "M")])
    b.add(180, 220, 900)
    cases.append(b.case("--utg-mode --qual-weighted"))

    b = Builder(14, "leading_ins_trim0", 400)     # a leading I is a column of its own without the trim
    b.add(10, 240, 1100, ops=[(3, "I"), (120, "M"), (2, "I"), (120, "M")])
    b.add(100, 230, 1000, ops=[(3, "I"), (230, "M")], ins={0: "ACG"})
    b.add(190, 205, 900)
    cases.append(b.case("--utg-mode --qual-weighted", "sr-trim=0"))

    b = Builder(15, "hard_clips", 450)
    b.add(0, 250, 1100, ops=[(5, "H"), (250, "M"), (7, "H")]), b.add(90, 270, 1200, ops=[(4, "S"), (270, "M"), (6, "H")])
    b.add(200, 245, 1000, ops=[(6, "S"), (120, "M"), (1, "I"), (125, "M"), (3, "S")])
    cases.append(b.case("--utg-mode --qual-weighted"))

    # two of three hits carry the same 5-base insertion: it wins, unless --max-ins-length turns it down
    for name, flags in (("ins_wins", "--utg-mode --no-use-ref-qual"), ("max_ins_length", "--utg-mode --no-use-ref-qual --max-ins-length 3")):
        b = Builder(16, name, 450)
        b.add(0, 260, 1200, ops=[(130, "M"), (5, "I"), (130, "M")], ins={1: "ACGTA"}, mism=0.0)
        b.add(60, 320, 1500, ops=[(70, "M"), (5, "I"), (250, "M")], ins={1: "ACGTA"}, mism=0.0)
        b.add(120, 321, 1400, ops=[(321, "M")], mism=0.0)
        cases.append(b.case(flags))

    # two insertion states of equal weight in column c; the one that ranks first was first seen in
    # u0, which the contained filter removes afterwards: with --rep-coverage the ranks come from
    # the matrix of step 2 (u0 included), without it from the consensus pass (u2 before u3)
    for name, flags in (("ins_tie_rank_step2", "--utg-mode --no-use-ref-qual --rep-coverage 50"), ("ins_tie_rank", "--utg-mode --no-use-ref-qual")):
        b = Builder(17, name, 600)
        c = 350
        b.ref = b.ref[:100] + b.ref[c] + b.ref[101:]
        b.add(60, 80, 300, ops=[(41, "M"), (2, "I"), (39, "M")], ins={1: "TT"}, mism=0.0)
        b.add(0, 200, 900, ops=[(200, "M")], mism=0.0)
        b.add(240, 210, 1000, ops=[(c - 240 + 1, "M"), (2, "I"), (210 - (c - 240) - 1, "M")], ins={1: "AA"}, mism=0.0)
        b.add(290, 230, 1100, ops=[(c - 290 + 1, "M"), (2, "I"), (230 - (c - 290) - 1, "M")], ins={1: "TT"}, mism=0.0)
        cases.append(b.case(flags))

    b = Builder(18, "no_survivor", 300)
    b.add(0, 200, 100), b.add(50, 220, 90)
    cases.append(b.case("--utg-mode --qual-weighted --min-ncscore 3.3"))

    b = Builder(20, "long_5000", 5100, fasta=True)
    b.add(50, 5000, 24000, qual="*")
    cases.append(b.case(FULL))

    b = Builder(21, "rep_coverage_zero", 300)     # every column is a window: everything is ignored
    b.add(0, 200, 900), b.add(50, 220, 1000)
    cases.append(b.case("--utg-mode --rep-coverage 0"))

    b = Builder(23, "bad_cigar_eq", 400)          # '=': Sam::Seq dies with "Unknown Cigar"
    b.add(0, 200, 900), b.add(100, 220, 1000, ops=[(70, "M"), (80, "="), (70, "M")])
    cases.append(b.case("--utg-mode --qual-weighted"))

    write_cases(out, cases)


if __name__ == "__main__":
    main(sys.argv[1])

"""Cases of the unitig consensus (bam2cns --utg-mode): the text format of
tests/golden/utg_cases.txt.gz / utg_expected.txt, the hand-made corner cases behind them, a seeded
generator of random reads, and the conversions to the library's input and to command lines.

A case file holds, per case::

    >>CASE name
    >>PARAM flags --qual-weighted --rep-coverage 7 ...      (bam2cns options)
    >>PARAM cfg sr-trim=0 ...                               (proovread.cfg overrides)
    >>REF
    @id [desc]\\nSEQ\\n+\\nQUAL      or      >id [desc]\\nSEQ
    >>SAM
    <SAM lines in arrival order>
    >>END

and an expected file::

    >>CASE name
    >>ERROR 1                      (only if the reference died)
    >>FASTQ
    @id\\nSEQ\\n+\\nQUAL
    >>TRACE
    MMDI...
    >>KEPT
    names of the alignments left after every filter, in arrival order
    >>WIN
    offset,length ...              (the overlap windows of bam2cns:398-422)
    >>END
"""
from __future__ import annotations

import dataclasses
import gzip
import random
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

GOLDEN = Path(__file__).resolve().parent / "golden"


@dataclasses.dataclass
class Case:
    name: str
    flags: str
    cfg: str
    ref: List[str]
    sam: List[str]

    @property
    def fasta(self) -> bool:
        return self.ref[0].startswith(">")


@dataclasses.dataclass
class Expected:
    name: str
    error: bool = False
    fastq: str = ""
    trace: str = ""
    kept: List[str] = dataclasses.field(default_factory=list)
    windows: List[Tuple[int, int]] = dataclasses.field(default_factory=list)


def write_cases(path, cases: Sequence[Case], header: str = "") -> None:
    with open(path, "w") as fh:
        fh.write(header)
        for c in cases:
            fh.write(f">>CASE {c.name}\n>>PARAM flags {c.flags}\n>>PARAM cfg {c.cfg}\n>>REF\n")
            fh.write("\n".join(c.ref) + "\n>>SAM\n" + "".join(s + "\n" for s in c.sam) + ">>END\n")


def read_cases(path=GOLDEN / "utg_cases.txt.gz") -> List[Case]:
    out, cur, sect = [], None, ""
    for line in (gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)):
        line = line.rstrip("\n")
        if line.startswith("#") and not sect:
            continue
        if line.startswith(">>CASE "):
            cur, sect = Case(line[7:], "", "", [], []), "head"
        elif line.startswith(">>PARAM flags"):
            cur.flags = line[14:]
        elif line.startswith(">>PARAM cfg"):
            cur.cfg = line[12:]
        elif line == ">>REF":
            sect = "ref"
        elif line == ">>SAM":
            sect = "sam"
        elif line == ">>END":
            out.append(cur)
            sect = ""
        elif sect == "ref":
            cur.ref.append(line)
        elif sect == "sam" and line:
            cur.sam.append(line)
    return out


def read_expected(path=GOLDEN / "utg_expected.txt") -> Dict[str, Expected]:
    out, cur, sect, fq = {}, None, "", []
    for line in open(path):
        line = line.rstrip("\n")
        if line.startswith("#") and not sect:
            continue
        if line.startswith(">>CASE "):
            cur, sect, fq = Expected(line[7:]), "head", []
        elif line.startswith(">>ERROR"):
            cur.error = True
        elif line in (">>FASTQ", ">>TRACE", ">>KEPT", ">>WIN"):
            sect = line[2:]
        elif line == ">>END":
            cur.fastq = "".join(x + "\n" for x in fq)
            out[cur.name] = cur
            sect = ""
        elif sect == "FASTQ":
            fq.append(line)
        elif sect == "TRACE":
            cur.trace = line
        elif sect == "KEPT":
            cur.kept = line.split()
        elif sect == "WIN":
            cur.windows = [tuple(int(v) for v in w.split(",")) for w in line.split()]
    return out


# ---------------------------------------------------------------------------
# building cases
def rand_seq(rng: random.Random, n: int) -> str:
    return "".join(rng.choice("ACGT") for _ in range(n))


def rand_qual(rng: random.Random, n: int, lo: int = 5, hi: int = 40) -> str:
    return "".join(chr(33 + rng.randrange(lo, hi + 1)) for _ in range(n))


def noisy_ops(rng: random.Random, span: int, indel: float) -> List[Tuple[int, str]]:
    """A CIGAR over `span` reference columns: M runs broken by short I / D."""
    ops: List[Tuple[int, str]] = []
    left = span
    while left > 0:
        m = min(left, 1 + int(rng.expovariate(indel)) if indel > 0 else left)
        ops.append((m, "M"))
        left -= m
        if left <= 0:
            break
        if rng.random() < 0.5:
            ops.append((rng.randrange(1, 4), "I"))
        else:
            d = min(left - 1, rng.randrange(1, 4))
            if d > 0:
                ops.append((d, "D"))
                left -= d
    if ops[-1][1] != "M":
        ops.pop()
    return ops


def sam_line(rng: random.Random, name: str, rid: str, ref: str, start: int, ops: Sequence[Tuple[int, str]],
             score: Optional[int], mism: float = 0.03, qual: Optional[str] = None, ins: Optional[Dict[int, str]] = None) -> str:
    """An alignment at 0-based `start` with the given ops; M copies the reference with mismatches,
    I takes random bases (or ins[op index]), S random bases; qual '*' for none."""
    seq, r = [], start
    for k, (n, op) in enumerate(ops):
        if op in "M=X":
            for t in range(n):
                b = ref[r + t]
                seq.append(rng.choice([x for x in "ACGT" if x != b]) if rng.random() < mism else b)
            r += n
        elif op == "D":
            r += n
        elif op in "IS":
            seq.append(ins[k] if ins and k in ins else rand_seq(rng, n))
    s = "".join(seq)
    q = qual if qual is not None else rand_qual(rng, len(s))
    cig = "".join(f"{n}{op}" for n, op in ops)
    tags = [] if score is None else [f"AS:i:{score}"]
    return "\t".join([name, "0", rid, str(start + 1), "60", cig, "*", "0", "0", s, q] + tags)


def aln_length(sam: str) -> int:
    """Alignment.pm:417-431."""
    import re
    f = sam.split("\t")
    cig = f[5]
    if re.search(r"^\d+S|S$", cig):
        return sum(int(n) for n, op in re.findall(r"(\d+)([MD])", cig))
    return len(f[9])


def random_case(rng: random.Random, name: str, lo: int = 300, hi: int = 3000, max_alns: int = 80) -> Case:
    """A seeded random read with 0..max_alns alignments, tied lengths included."""
    L = rng.randrange(lo, hi + 1)
    ref = rand_seq(rng, L)
    rid = f"lr_{name}"
    fasta = rng.random() < 0.15
    desc = ""
    if rng.random() < 0.4:
        k = rng.randrange(1, 3)
        desc = " " + " ".join(f"MCR{i}:{rng.randrange(0, L)},{rng.randrange(1, 120)}" for i in range(k))
    n = rng.choice([0, 1, 2, 3, 5, 8, 13, 30, max_alns]) if rng.random() < 0.5 else rng.randrange(0, max_alns + 1)
    sam = []
    stack_at = rng.randrange(0, L)
    for i in range(n):
        kind = rng.random()
        if kind < 0.45:      # a stack of short hits
            span = rng.choice([15, 20, 30, 55, 60, 60, 61, 80, 120])
            start = max(0, min(L - span, stack_at + rng.randrange(-40, 41)))
        elif kind < 0.9:
            span = rng.randrange(51, max(52, min(L, 1500)))
            start = rng.randrange(0, L - span + 1)
        else:
            span = rng.randrange(max(51, L // 2), L + 1)
            start = rng.randrange(0, L - span + 1)
        span = min(span, L - start)
        ops = noisy_ops(rng, span, rng.choice([0.0, 0.01, 0.03, 0.08]))
        if rng.random() < 0.15:
            ops = [(rng.randrange(1, 9), "S")] + ops
        if rng.random() < 0.15:
            ops = ops + [(rng.randrange(1, 9), "S")]
        if rng.random() < 0.05:
            ops = [(3, "H")] + ops if ops[0][1] != "S" else ops
        if rng.random() < 0.04 and ops[0][1] == "M":
            ops = [(2, "I")] + ops
        score = None if rng.random() < 0.05 else rng.randrange(-6, 7) * span + rng.randrange(-50, 50)
        qual = "*" if rng.random() < 0.3 else None
        sam.append(sam_line(rng, f"u{i}", rid, ref, start, ops, score, mism=rng.choice([0.0, 0.02, 0.1]), qual=qual))
    flags = ["--utg-mode"]
    if rng.random() < 0.7:
        flags.append("--qual-weighted")
    if rng.random() < 0.6:
        flags += ["--rep-coverage", str(rng.choice([0, 1, 2, 3, 5, 7]))]
    if rng.random() < 0.5:
        flags += ["--min-ncscore", rng.choice(["3.3", "0.5", "-1", "2"])]
    if rng.random() < 0.5:
        flags += ["--fallback-phred", str(rng.choice([0, 10, 30]))]
    if rng.random() < 0.4:
        flags.append("--invert-scores")
    if rng.random() < 0.3:
        flags += ["--max-ins-length", str(rng.choice([1, 2, 3]))]
    if rng.random() < 0.2:
        flags.append("--no-use-ref-qual")
    if rng.random() < 0.1:
        flags.append("--ignore-hcr")
    cfg = rng.choice(["", "", "sr-trim=0", "sr-indel-taboo-length=0 sr-indel-taboo=0.05", "sr-indel-taboo-length=3"])
    refl = [f">{rid}{desc}", ref] if fasta else [f"@{rid}{desc}", ref, "+", rand_qual(rng, L, 0, 40)]
    return Case(name, " ".join(flags), cfg, refl, sam)


def random_cases(seed: int, n: int, **kw) -> List[Case]:
    rng = random.Random(seed)
    return [random_case(rng, f"r{seed}_{i}", **kw) for i in range(n)]


# ---------------------------------------------------------------------------
# conversions
def parse_flags(flags: str, cfg: str = "") -> dict:
    """The options of a case as keyword arguments of proovread_amd.utgcns.UtgParams, plus
    ignore_hcr."""
    f = flags.split()
    o: dict = {}
    i = 0
    while i < len(f):
        k = f[i]
        if k == "--qual-weighted":
            o["qual_weighted"] = True
        elif k == "--no-use-ref-qual":
            o["use_ref_qual"] = False
        elif k == "--invert-scores":
            o["invert_scores"] = True
        elif k == "--ignore-hcr":
            o["ignore_hcr"] = True
        elif k == "--rep-coverage":
            i += 1
            o["rep_coverage"] = int(f[i])
        elif k == "--min-ncscore":
            i += 1
            o["min_ncscore"] = float(f[i])
        elif k == "--fallback-phred":
            i += 1
            o["fallback_phred"] = int(f[i])
        elif k == "--max-ins-length":
            i += 1
            o["max_ins_length"] = int(f[i])
        elif k == "--coverage":
            i += 1
        elif k != "--utg-mode":
            raise ValueError(k)
        i += 1
    for kv in cfg.split():
        k, v = kv.split("=")
        o[{"sr-trim": "trim", "sr-indel-taboo-length": "indel_taboo_length", "sr-indel-taboo": "indel_taboo"}[k]] = \
            float(v) if k == "sr-indel-taboo" else int(v)
    return o


def to_inputs(case: Case):
    """(LongRead, [SamRecord], UtgParams) of a case, as bam2cns prepares them."""
    from proovread_amd import cns, utgcns
    o = parse_flags(case.flags, case.cfg)
    ignore = o.pop("ignore_hcr", False)
    head = case.ref[0][1:].split(None, 1)
    desc = head[1] if len(head) > 1 else ""
    if case.fasta:
        read = cns.LongRead(head[0], case.ref[1], None, "")
        o["use_ref_qual"] = False
    else:
        read = cns.LongRead(head[0], case.ref[1], case.ref[3], "" if ignore else desc)
    return read, [cns.SamRecord.from_line(s) for s in case.sam], utgcns.UtgParams(**o)


def write_files(case: Case, d: Path, bam: bool = False) -> List[str]:
    """The case as files and the bam2cns command line that runs it (without --host / --prefix)."""
    rid = case.ref[0][1:].split()[0]
    ref = d / (case.name + (".fa" if case.fasta else ".fq"))
    ref.write_text("\n".join(case.ref) + "\n")
    sam = d / (case.name + ".sam")
    sam.write_text(f"@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:{rid}\tLN:{len(case.ref[1])}\n" + "".join(s + "\n" for s in case.sam))
    argv = ["--ref", str(ref), "--debug"] + case.flags.split()
    if case.cfg:
        cfg = d / (case.name + ".cfg")
        cfg.write_text("(\n" + "".join(f"  '{kv.split('=')[0]}' => {kv.split('=')[1]},\n" for kv in case.cfg.split()) + ");\n")
        argv += ["--cfg", str(cfg)]
    if bam:
        import bamio
        out = d / (case.name + ".bam")
        bamio.write_bam(str(out), [(rid, len(case.ref[1]))], case.sam)
        return ["--bam", str(out)] + argv
    return ["--sam", str(sam)] + argv

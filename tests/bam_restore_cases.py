"""PR_BAM_RESTORE_SEQ's rule (include/prgpu.h) restated in plain Python on SAM
lines, and the streams the restore tests share (tests/test_bam_restore_host.py on the host build
of bam_core.h, tests/test_bam_restore_gpu.py on the device).

The oracle rewrites lines; the project's encoder and the decode path that was there before the
option then run on the rewritten lines.  Nothing here calls the code under test."""
import random
import re

CIGAR_OP = re.compile(r"(\d+)([MIDNSHP=X])")
PR_ERR_SAM, PR_ERR_NOSEQ = -3, -4
_COMP = str.maketrans("ACGT", "TGCA")


class Refused(Exception):
    def __init__(self, code, index, qname):
        super().__init__(f"{code}: record {index} ({qname})")
        self.code, self.index, self.qname = code, index, qname


def span(cigar: str):
    """(q, hl, ht, has_h): the M I S = X lengths, the leading / trailing H, an H anywhere."""
    ops = [(int(n), o) for n, o in CIGAR_OP.findall(cigar)] if cigar != "*" else []
    q = sum(n for n, o in ops if o in "MIS=X")
    hl = ops[0][0] if ops and ops[0][1] == "H" else 0
    ht = ops[-1][0] if len(ops) > 1 and ops[-1][1] == "H" else 0
    return q, hl, ht, any(o == "H" for _, o in ops)


def restore(lines, kept=None):
    """SAM lines in record order -> (the lines with every kept `*` SEQ restored, donor_of):
    donor_of[i] is the record line i took its SEQ from.  kept: the reference names whose records
    are kept (None: all).  Raises Refused for the lowest record the rule refuses."""
    fields = [ln.split("\t") for ln in lines]
    donors = {}
    for i, f in enumerate(fields):
        flag = int(f[1])
        if f[9] != "*" and not flag & 0x904 and not span(f[5])[3]:
            donors.setdefault((f[0], flag & 0xC0), i)
    out, donor_of = [], {}
    for i, f in enumerate(fields):
        if f[9] != "*" or (kept is not None and f[2] not in kept):
            out.append(lines[i])
            continue
        flag = int(f[1])
        d = donors.get((f[0], flag & 0xC0))
        if d is None:
            raise Refused(PR_ERR_NOSEQ, i, f[0])
        df = fields[d]
        q, hl, ht, _ = span(f[5])
        if hl + q + ht != len(df[9]):
            raise Refused(PR_ERR_SAM, i, f[0])
        seq, qual = df[9], df[10]
        if (flag ^ int(df[1])) & 0x10:
            seq = seq[::-1].translate(_COMP)
            qual = qual if qual == "*" else qual[::-1]
        g = list(f)
        g[9] = seq[hl:hl + q]
        g[10] = qual if qual == "*" else qual[hl:hl + q]
        out.append("\t".join(g))
        donor_of[i] = d
    return out, donor_of


def sort_lines(lines, names):
    """Coordinate order as a stable sort by (reference, POS): what `samtools sort` leaves of lines
    that share both is their input order."""
    rid = {n: k for k, n in enumerate(names)}
    return sorted(lines, key=lambda ln: (rid[ln.split("\t")[2]], int(ln.split("\t")[3])))


# ---------------------------------------------------------------------------- the directed stream
NAMES = ["lr0", "lr_out", "lr1", "lr2"]     # the header's references; lr_out is in no batch
REPEAT = 150


def _rc(s):
    return s[::-1].translate(_COMP)


def _mutate(rng, s, n):
    s = list(s)
    for j in rng.sample(range(len(s)), min(n, len(s))):
        s[j] = rng.choice("ACGT")
    return "".join(s)


def directed(seed=5):
    """(long reads {id: sequence}, SAM lines sorted by coordinate).  Three long reads of about
    410 bp share a 150 bp repeat (lr2 carries its reverse complement), lr_out is the repeat alone.
    Short reads from the repeat have one primary line and `*` secondaries on the other copies,
    as `bwa mem -a` prints them; short reads from the unique parts have a primary line only."""
    rng = random.Random(seed)
    dna = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    rep = dna(REPEAT)
    at = {"lr0": 60, "lr1": 170, "lr2": 215, "lr_out": 0}
    lrs = {"lr0": dna(60) + rep + dna(200), "lr1": dna(170) + rep + dna(90), "lr2": dna(215) + _rc(rep) + dna(48)}
    fwd = {"lr0": True, "lr1": True, "lr2": False, "lr_out": True}
    lines = []

    def place(qname, flag, ref, a, L, seq, qual, hl=0, ht=0, extra=""):
        """A line for bases [a + hl, a + L - ht) of the repeat on `ref`; seq None: `*`."""
        strand = 0 if fwd[ref] else 16
        lo, hi = a + hl, a + L - ht
        pos = at[ref] + (lo if fwd[ref] else REPEAT - hi) + 1
        # in the orientation of the line's strand the clips swap sides on the reverse copy
        h5, h3 = (hl, ht) if fwd[ref] else (ht, hl)
        cig = (f"{h5}H" if h5 else "") + f"{hi - lo}M" + (f"{h3}H" if h3 else "")
        lines.append("\t".join([qname, str(flag | strand), ref, str(pos), "60" if not flag & 256 else "0", cig, "*", "0", "0",
                                seq or "*", qual or "*", f"AS:i:{hi - lo - 2}"]) + extra)

    def repeat_read(k, primary, others, clips, flag=0, qname=None, with_qual=True):
        L = rng.randrange(40, 71)
        a = rng.randrange(0, REPEAT - L)
        x = _mutate(rng, rep[a:a + L], 2)                        # the read, in the repeat's orientation
        qx = "".join(chr(33 + rng.randrange(20, 41)) for _ in range(L))
        qname = qname or f"rep{k}"
        sq = (x, qx) if fwd[primary] else (_rc(x), qx[::-1])
        place(qname, flag, primary, a, L, sq[0], sq[1] if with_qual else None)
        for ref, (hl, ht) in zip(others, clips):
            place(qname, flag | 256, ref, a, L, None, None, hl, ht)

    k = 0
    # both strands, every clip form (an odd leading clip among them), donors on every reference
    for primary, others in (("lr0", ("lr1", "lr2")), ("lr2", ("lr0", "lr1")), ("lr1", ("lr2", "lr0")),
                            ("lr_out", ("lr0", "lr2")), ("lr_out", ("lr1", "lr2"))):
        for clips in (((0, 0), (0, 0)), ((5, 0), (3, 0)), ((0, 7), (0, 4)), ((3, 4), (7, 6)), ((1, 0), (0, 1))):
            repeat_read(k, primary, others, clips)
            k += 1
    repeat_read(k, "lr0", ("lr1", "lr2"), ((0, 0), (5, 2)), with_qual=False)            # a donor without QUAL
    repeat_read(k + 1, "lr_out", ("lr2",), ((2, 0),), with_qual=False)
    repeat_read(k + 2, "lr1", ("lr0", "lr2"), ((0, 0), (0, 0)), flag=0x41, qname="pair")   # two mates of one QNAME
    repeat_read(k + 3, "lr2", ("lr0", "lr1"), ((0, 3), (0, 0)), flag=0x81, qname="pair")
    repeat_read(k + 4, "lr0", ("lr2",), ((0, 0),), qname="x")                             # names of 1 and 254 bytes
    repeat_read(k + 5, "lr2", ("lr1",), ((9, 0),), qname="n" * 254)
    # a secondary line that kept its own SEQ (bwa-proovread's form)
    L, a = 50, 20
    x = _mutate(rng, rep[a:a + L], 1)
    place("own", 0, "lr0", a, L, x, "5" * L)
    place("own", 256, "lr1", a, L, _mutate(rng, x, 1), "7" * L)
    # an insertion and soft clips under `*`
    x = rep[30:50] + "TT" + rep[50:80]
    lines.append("\t".join(["ins", "0", "lr0", str(at["lr0"] + 31), "60", "20M2I30M", "*", "0", "0", x, "I" * 52, "AS:i:40"]))
    lines.append("\t".join(["ins", "256", "lr1", str(at["lr1"] + 36), "0", "5S15M2I26M4S", "*", "0", "0", "*", "*", "AS:i:30"]))
    # the unique parts: plain primary lines
    for j in range(24):
        ref = ("lr0", "lr1", "lr2")[j % 3]
        s = lrs[ref]
        L = rng.randrange(40, 71)
        p = rng.choice([q for q in range(0, len(s) - L) if q + L <= at[ref] or q >= at[ref] + REPEAT])
        lines.append("\t".join([f"uniq{j}", str(16 * (j % 2)), ref, str(p + 1), "60", f"{L}M", "*", "0", "0",
                                _mutate(rng, s[p:p + L], 1), "I" * L, f"AS:i:{L - 1}"]))
    return lrs, sort_lines(lines, NAMES)


# ---------------------------------------------------------------------------- the table under load
def fnv_home_slot(qname: str, flag: int, mask: int) -> int:
    """bam_key_hash's home slot of a key: FNV-1a over the name, its NUL and the mate bits, mixed."""
    m64 = (1 << 64) - 1
    h = 0xcbf29ce484222325
    for b in qname.encode() + b"\0" + bytes([flag & 0xC0]):
        h = ((h ^ b) * 0x100000001b3) & m64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & m64
    h ^= h >> 33
    return h & mask


def probing(n=2000, seed=9):
    """n names one character apart, each with a `*` secondary line (first in the stream) and a
    primary line whose SEQ no other read has: the restored SEQ names the donor."""
    rng = random.Random(seed)
    seqs = set()
    while len(seqs) < n:
        seqs.add("".join(rng.choice("ACGT") for _ in range(24)))
    seqs = sorted(seqs)
    rng.shuffle(seqs)
    sec = [f"q{i:04d}\t{256 + 16 * (i % 2)}\tlr0\t{i + 1}\t0\t24M\t*\t0\t0\t*\t*" for i in range(n)]
    pri = [f"q{i:04d}\t0\tlr1\t{i + 1}\t60\t24M\t*\t0\t0\t{seqs[i]}\t{'I' * 24}" for i in range(n)]
    return sec + pri


# ---------------------------------------------------------------------------- refusals (reference lr0)
REFUSALS = {
    # name: (lines, code, the record that is named)
    "no_donor": (["a\t0\tlr0\t1\t60\t4M\t*\t0\t0\tACGT\tIIII", "b\t256\tlr0\t2\t0\t4M\t*\t0\t0\t*\t*",
                  "c\t256\tlr0\t3\t0\t4M\t*\t0\t0\t*\t*"], PR_ERR_NOSEQ, 1),
    "length_mismatch": (["a\t0\tlr0\t1\t60\t4M\t*\t0\t0\tACGT\tIIII", "a\t256\tlr0\t2\t0\t2H3M\t*\t0\t0\t*\t*"], PR_ERR_SAM, 1),
    "donor_with_h_only": (["a\t0\tlr0\t1\t60\t1H4M\t*\t0\t0\tACGT\tIIII", "a\t2048\tlr0\t2\t60\t4M1H\t*\t0\t0\tACGT\tIIII",
                           "a\t256\tlr0\t3\t0\t5M\t*\t0\t0\t*\t*"], PR_ERR_NOSEQ, 2),
}

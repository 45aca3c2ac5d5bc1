"""The directed batch of tests/test_bam_export_gpu.py: three random long reads and short reads cut
from them exactly, placed so that the exported records cover what the encoder can get wrong --
every AS width the scores of this batch reach, both strands, a secondary record, a soft clip, an
N, odd and even l_seq, the shortest and the longest name, and bins on three reg2bin levels."""
import numpy as np

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
R0_LEN, R1_LEN, R2_LEN = 16600, 1000, 131300


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def directed(seed: int = 11):
    """-> (long reads [(id, seq, qual)], short reads [(name, seq, qual)], what: name -> note)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    r0 = bytearray(bytes(rng.choice(acgt, R0_LEN)))
    r1 = bytes(rng.choice(acgt, R1_LEN))
    r2 = bytearray(bytes(rng.choice(acgt, R2_LEN)))
    r2[90000:90150] = r2[40000:40150]   # one 150-mer twice: a primary and a secondary record
    r0, r2 = bytes(r0), bytes(r2)
    srs, what = [], {}

    def add(name, seq, note):
        q = bytes(rng.integers(35, 74, len(seq)).astype(np.uint8))
        srs.append((name, seq, q))
        what[name] = note

    # R0: alignments ending at 16383 and at 16384, one straddling 16384
    add("end16383", r0[16233:16383], "R0 [16233, 16383)")
    add("end16384", r0[16234:16384], "R0 [16234, 16384)")
    add("over16384", r0[16300:16450], "R0 [16300, 16450)")
    # R2: inside one 16 kb window, and straddling 131072
    add("in16k", r2[20000:20150], "R2 [20000, 20150)")
    add("over131072", r2[131000:131150], "R2 [131000, 131150)")
    # 25, 26, 51, 52 bp: AS 125, 130, 255, 260 -> c, C, C, s; odd and even l_seq
    for l, at in ((25, 1000), (26, 2000), (51, 3000), (52, 4000)):
        add(f"len{l}", r0[at:at + l], f"R0 [{at}, {at + l}) AS {5 * l}")
    # 150 bp on both strands
    add("fw150", r0[5000:5150], "R0 forward")
    add("rc150", revcomp(r0[6000:6150]), "R0 reverse")
    add("rc150b", revcomp(r2[50000:50151]), "R2 reverse, odd l_seq")
    # an N inside
    s = bytearray(r0[7000:7150])
    s[70] = ord("N")
    add("withN", bytes(s), "R0 forward with N")
    s = bytearray(revcomp(r2[60000:60150]))
    s[31] = ord("N")
    add("withNrc", bytes(s), "R2 reverse with N")
    # a 20-base tail that mismatches the reference everywhere: a soft clip
    tail = r0[8130:8150].translate(bytes.maketrans(b"ACGT", b"CATG"))
    add("clip3", r0[8000:8130] + tail, "R0 130M20S")
    add("clip5rc", revcomp(r0[9000:9130] + r0[9130:9150].translate(bytes.maketrans(b"ACGT", b"CATG"))), "R0 reverse, clip")
    # the planted 150-mer
    add("twice", r2[40000:40150], "R2 at 40000 and 90000")
    # names of 1 and of 254 bytes
    add("x", r0[10000:10150], "1-byte name")
    add("n" * 254, r2[70000:70150], "254-byte name")
    lrs = [("R0", r0, b"$" * len(r0)), ("R1", r1, b"$" * len(r1)), ("R2", r2, b"$" * len(r2))]
    return lrs, srs, what

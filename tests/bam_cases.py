"""BAM record streams for the decoder tests (tests/test_bam_core_host.py on the host build of
bam_core.h, tests/test_bam_decode_gpu.py on the device): records of every shape the decoder
branches on, encoded by the project's own pr_sam_encode, and malformed ones patched from them."""
import ctypes as C
import random
import struct

import numpy as np

from proovread_amd import bamio, cns
from proovread_amd.bam2cns import _BamAlns

LSEQS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257)
NCIGS = (0, 1, 3, 40)
REFS = ("lr0", "lr1", "lr2")
# no AS, AS of every integer type (the encoder picks the smallest that fits), f and Z
AS_TAGS = (None, "AS:i:-7", "AS:i:200", "AS:i:-300", "AS:i:60000", "AS:i:-100000", "AS:i:3000000000", "AS:f:123.456",
           "AS:Z: 42.5abc", "AS:Z:", "AS:Z:-.5e1")
# every type the walk skips: A, the six integers, f, Z, an empty Z, H, B arrays of each subtype, an empty B
SKIP_TAGS = ("XA:A:x", "Xc:i:-5", "XC:i:201", "Xs:i:-301", "XS:i:60001", "Xi:i:-100001", "XI:i:3000000001", "Xf:f:3.25",
             "XZ:Z:hi there", "XE:Z:", "XH:H:1F", "Ba:B:c,-1,2,3", "Bb:B:C,1,2,250", "Bc:B:s,-300,2", "Bd:B:S,60000,2",
             "Be:B:i,-100000,7", "Bf:B:I,3000000000", "Bg:B:f,1.5,2.5", "Bh:B:i")
COLUMNS = ("rid", "pos1", "score", "flags", "seq_off", "lseq", "cig_off", "ncig", "seq", "qual", "cig")


def sam_lines(seed=7):
    """SAM lines covering l_seq x read-name length x n_cigar, QUAL present / absent, the AS forms
    (alone, after every skip type, twice), an unmapped record."""
    rng = random.Random(seed)
    lines = []
    k = 0
    for lseq in LSEQS:
        for name_len in range(1, 9):
            for ncig in NCIGS:
                qname = "qrstuvwx"[:name_len]
                cig = "".join(f"{rng.randint(1, 300)}{rng.choice('MIDNSHP=X')}" for _ in range(ncig)) or "*"
                seq = "".join(rng.choice("=ACMGRSVTWYHKDBN") for _ in range(lseq)) or "*"
                qual = "*" if (lseq == 0 or k % 3 == 1) else "".join(chr(33 + rng.randint(0, 93)) for _ in range(lseq))
                unmapped = k % 11 == 10
                tags = []
                if k % 2 == 0:
                    tags += SKIP_TAGS
                a = AS_TAGS[k % len(AS_TAGS)]
                if a:
                    tags.append(a)
                if k % 7 == 3:
                    tags.append(AS_TAGS[(k // 7) % (len(AS_TAGS) - 1) + 1])   # AS twice: the last wins
                f = [qname, "4" if unmapped else str(16 * (k % 2)), "*" if unmapped else REFS[k % 3],
                     "0" if unmapped else str(1 + 10 * k), "60", cig, "*", "0", "0", seq, qual] + tags
                lines.append("\t".join(f))
                k += 1
    return lines


def encode(lines, refs=REFS):
    """SAM lines -> a BAM record stream (pr_sam_encode)."""
    return bamio._native_encode("".join(x + "\n" for x in lines), list(refs))


def with_aux(rec: bytes, aux: bytes) -> bytes:
    """A record (block_size first) with its aux area replaced."""
    bs, = struct.unpack_from("<i", rec, 0)
    l_rn = rec[12]
    n_cig, = struct.unpack_from("<H", rec, 16)
    l_seq, = struct.unpack_from("<i", rec, 20)
    body = rec[4:4 + 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq] + aux
    assert len(body) <= bs + len(aux)
    return struct.pack("<i", len(body)) + body


def malformed_records():
    """Records whose aux area is cut inside a field or names an unknown type."""
    rec = encode(["q1\t0\tlr0\t5\t60\t4M\t*\t0\t0\tACGT\tIIII"])
    good = (b"XAAx", b"Xcc\x01", b"Xss\x01\x02", b"Xii\x01\x02\x03\x04", b"Xff\x00\x00\x80\x3f", b"XZZabc\x00",
            b"XBBs\x02\x00\x00\x00\x01\x02\x03\x04", b"ASi\x07\x00\x00\x00")
    out = []
    for g in good:
        for cut in range(1, len(g)):
            out.append(with_aux(rec, g[:cut]))
    out += [with_aux(rec, b"XXq\x01"), with_aux(rec, b"XXBq\x01\x00\x00\x00\x01"),
            with_aux(rec, b"XXBc\xff\xff\xff\xff"), with_aux(rec, b"ASi\x01\x00\x00\x00XZZabc")]
    return out


def take_alns(a: _BamAlns):
    """The columns and pools of a pr_bam_alns as numpy copies."""
    def take(p, ct, n):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(max(n, 1),))[:n].copy()
    n = a.n
    return {"rid": take(a.rid, C.c_int32, n), "pos1": take(a.pos1, C.c_int32, n), "score": take(a.score, C.c_double, n),
            "flags": take(a.flags, C.c_uint8, n), "seq_off": take(a.seq_off, C.c_int64, n), "lseq": take(a.lseq, C.c_int32, n),
            "cig_off": take(a.cig_off, C.c_int64, n), "ncig": take(a.ncig, C.c_int32, n),
            "seq": take(a.seq, C.c_uint8, a.seq_len), "qual": take(a.qual, C.c_uint8, a.seq_len),
            "cig": take(a.cig, C.c_uint32, a.cig_len)}


def host_decode(body: bytes):
    """pr_bam_decode_alns (the host decoder) -> (rc, columns or None)."""
    L, _, _ = bamio._codec()
    L.pr_bam_decode_alns.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.POINTER(_BamAlns)]
    L.pr_bam_alns_free.argtypes = [C.POINTER(_BamAlns)]
    L.pr_bam_alns_free.restype = None
    a = _BamAlns()
    rc = L.pr_bam_decode_alns(body, len(body), 1, C.byref(a))
    if rc:
        return rc, None
    try:
        return 0, take_alns(a)
    finally:
        L.pr_bam_alns_free(C.byref(a))


def assert_same(got, want):
    for k in COLUMNS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if k == "score":   # bit for bit (a NaN would compare unequal)
            assert (got[k].view(np.uint64) == want[k].view(np.uint64)).all(), k
        else:
            assert (got[k] == want[k]).all(), (k, np.nonzero(got[k] != want[k])[0][:5])


def perl_number(text: bytes) -> float:
    return cns.parse_perl_number(text.decode("latin-1"))

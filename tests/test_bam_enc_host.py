"""The device BAM encoder's shared core (proovread_amd/csrc/bam_enc_core.h: record size, record
bytes by one lane or spread over 16) built for the host (tests/native/bam_enc_host.cpp) against
pr_sam_encode of the equivalent SAM line, byte for byte, with guard bytes around every record;
the same file runs as a program under AddressSanitizer and UBSan.  Also the host pieces of
--keep-temporary-files: pr_fastq4_names against the record parser, and the flag itself."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bam_cases
from proovread_amd import correct

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "bam_enc_host.cpp"
CODEC = ROOT / "proovread_amd" / "csrc" / "bam_codec.cpp"

# the grid of tests/native/bam_enc_host.cpp
LSEQS = (1, 2, 15, 16, 17, 25, 26, 150, 151, 1000)
NAMES = (1, 2, 3, 4, 5, 254)
SCORES = (-129, -128, 0, 127, 128, 255, 256, 32767, 32768, 65535, 65536)
CIG_KINDS, POS_KINDS = 4, 7   # n_cigar 1, 2, 2 (span 0), 7; ends at 16383/4/5, straddles of 1 << 17, 20, 23, 26


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    out = tmp_path_factory.mktemp("bam_enc") / "libbam_enc_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", str(out), str(SRC),
                    str(CODEC), "-lz", "-pthread"], check=True)
    L = C.CDLL(str(out))
    L.bam_enc_grid.argtypes = [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.bam_enc_grid.restype = C.c_int64
    L.bam_enc_record.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.c_void_p, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    L.bam_enc_record.restype = C.c_int64
    L.bam_enc_last_error.restype = C.c_char_p
    return L


@pytest.mark.parametrize("nlanes", [1, 16])
def test_grid_equals_sam_encode(core, nlanes):
    """Every combination of l_seq, name length, CIGAR shape, strand, QUAL present / absent, AS and
    POS window, each record written at the line offset it has in the stream."""
    cases, guards = C.c_int64(), C.c_int64()
    bad = core.bam_enc_grid(nlanes, C.byref(cases), C.byref(guards))
    assert bad == 0, core.bam_enc_last_error().decode()
    assert guards.value == 0
    assert cases.value == len(LSEQS) * len(NAMES) * CIG_KINDS * 2 * 2 * len(SCORES) * POS_KINDS


def _encode(core, rid, pos, flag, score, name, ops, nt4, qual, rev, nl, align):
    cig = np.array(ops, np.uint32)
    seq = np.array(nt4, np.uint8)
    q = None if qual is None else np.frombuffer(qual, np.uint8)
    out = np.zeros(8192, np.uint8)
    n = core.bam_enc_record(rid, pos, flag, score, name, len(name), cig.ctypes.data, len(cig), seq.ctypes.data,
                            None if q is None else q.ctypes.data, len(seq), rev, nl, align, out.ctypes.data, len(out))
    assert n > 0, n
    return out[:n].tobytes()


def test_records_against_the_library_encoder(core):
    """A few records against libprgpu's own pr_sam_encode (the grid uses the copy compiled into
    the test library), at every offset of a 16-byte line; a wrong byte is seen."""
    rng = np.random.default_rng(5)
    for l in (1, 16, 17, 51, 150):
        nt4 = rng.integers(0, 5, l).astype(np.uint8)
        qual = bytes(rng.integers(33, 75, l).astype(np.uint8))
        ops = [(3 << 4) | 4, (l << 4) | 0, (2 << 4) | 2, (1 << 4) | 1]
        for rev in (0, 1):
            seq = "".join("ACGTN"[b] for b in nt4) if not rev else "".join("TGCAN"[b] for b in nt4[::-1])
            for q in (qual, None):
                qs = "*" if q is None else (q[::-1] if rev else q).decode()
                for score, flag in ((l * 5, 16 * rev), (-300, 16 * rev | 0x100)):
                    line = f"read{l}\t{flag}\tlr1\t{16380 - l + 1}\t{0 if flag & 0x100 else 60}\t3S{l}M2D1I\t*\t0\t0\t{seq}\t{qs}\tAS:i:{score}"
                    want = bam_cases.encode([line])
                    for align in range(16):
                        got = _encode(core, 1, 16380 - l, flag, score, f"read{l}".encode(), ops, nt4, q, rev, 16, align)
                        assert got == want, (l, rev, q is None, score, align)
    assert _encode(core, 1, 5, 0, 7, b"x", [(4 << 4)], [0, 1, 2, 3], None, 0, 1, 0) != \
        bam_cases.encode(["x\t0\tlr1\t6\t60\t4M\t*\t0\t0\tACGA\t*\tAS:i:7"])


def test_program_under_sanitizers(tmp_path):
    """The stand-alone program (the same grid, 1 and 16 lanes) built with AddressSanitizer and UBSan."""
    exe = tmp_path / "bam_enc_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DBAM_ENC_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(SRC), str(CODEC), "-lz", "-pthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout


# ---------------------------------------------------------------------------- short-read names
def _parser_names(data: bytes):
    from proovread_amd import seqchunker
    names, quals = [], []
    for a, b in seqchunker.records(data):
        lines = data[a:b].split(b"\n")
        names.append(lines[0][1:].split()[0])
        quals.append(lines[3].strip() if data[a:a + 1] == b"@" else None)
    return names, quals


def _fastq(n, descriptions, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        l = int(rng.integers(1, 90))
        s = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), l))
        q = bytes(rng.integers(33, 74, l).astype(np.uint8)).replace(b"@", b"A")
        d = (b" 1:N:0:%d" % i if i % 2 else b"\tlen=%d extra" % l) if descriptions else b""
        out.append(b"@r%d/%d" % (i * 7919, i % 2 + 1) + d + b"\n" + s + b"\n+\n" + q + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("descriptions", [False, True])
def test_fastq4_names_equals_the_record_parser(descriptions):
    data = _fastq(300, descriptions)
    srs = correct.ShortReads(data, chunk_number=10)
    names, quals = _parser_names(data)
    assert len(names) == 300 and (not descriptions or any(b" " in data[a:data.index(b"\n", a)] for a in srs.starts[:4]))
    for rg in (np.array([[0, 300]]), np.array([[250, 300], [3, 4], [10, 120]]), np.zeros((0, 2), np.int64)):
        idx = [i for a, b in rg for i in range(a, b)]
        got = correct._fastq4_names_native(data, srs.starts[idx], srs.lengths[idx])
        assert got is not None and srs.fastq4
        pool, off, qual = srs.names_of(rg)
        assert np.array_equal(off, got[1]) and bytes(pool[:off[-1]]) == bytes(got[0][:off[-1]])
        assert [bytes(pool[off[k]:off[k + 1]]) for k in range(len(idx))] == [names[i] for i in idx]
        assert bytes(qual[:int(srs.lengths[idx].sum())]) == b"".join(quals[i] for i in idx)


def test_fastq4_names_declines_fasta_and_the_parser_takes_over():
    rng = np.random.default_rng(9)
    recs = [(b"f%d" % i, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 70 + i))) for i in range(40)]
    data = b"".join(b">" + n + b" desc\n" + s[:60] + b"\n" + s[60:] + b"\n" for n, s in recs)
    srs = correct.ShortReads(data, chunk_number=4)
    assert not srs.fastq4 and correct._fastq4_names_native(data, srs.starts, srs.lengths) is None
    pool, off, qual = srs.names_of(np.array([[5, 40], [0, 2]]))
    idx = list(range(5, 40)) + [0, 1]
    assert qual is None
    assert [bytes(pool[off[k]:off[k + 1]]) for k in range(len(idx))] == [recs[i][0] for i in idx]
    # a start that is no record start is declined too
    fq = _fastq(5, False)
    assert correct._fastq4_names_native(fq, np.array([1], np.int64), np.array([0], np.int64)) is None


@pytest.mark.parametrize("eol, pad", [(b"\r\n", b""), (b"\n", b"  "), (b"\n", b"\t")], ids=["crlf", "blanks", "tab"])
def test_fastq4_names_declines_what_the_scan_declines(eol, pad):
    """CR LF line ends: the scan declines the stream and the record parser strips the CR, so the
    reads are shorter than their lines; the native pass must decline too, whatever lengths it is
    given, and names_of must not try it.  Blanks behind SEQ and QUAL pass the scan, which keeps
    them as bases: the native pass takes the records with those lengths and declines them with
    the stripped ones.  In no case does it write more than the given lengths add up to."""
    recs = [(b"a", b"ACGT", b"IIII"), (b"bb", b"ACGTACGTAC", b"ABCDEFGHIJ"), (b"c", b"A", b"#")]
    data = b"".join(b"@" + n + b" d" + eol + s + pad + eol + b"+" + eol + q + pad + eol for n, s, q in recs)
    srs = correct.ShortReads(data, chunk_number=2)
    stripped = np.array([len(s) for _, s, _ in recs], np.int64)
    line_len = stripped + len(pad) + (1 if eol == b"\r\n" else 0)
    if eol == b"\r\n":
        assert not srs.fastq4 and np.array_equal(srs.lengths, stripped)
        for lens in (stripped, line_len):
            assert correct._fastq4_names_native(data, srs.starts, lens) is None
        pool, off, qual = srs.names_of(np.array([[0, 3]]))
        assert [bytes(pool[off[k]:off[k + 1]]) for k in range(3)] == [n for n, _, _ in recs]
        assert bytes(qual[:int(stripped.sum())]) == b"".join(q for _, _, q in recs)
    else:
        assert srs.fastq4 and np.array_equal(srs.lengths, line_len)
        assert correct._fastq4_names_native(data, srs.starts, stripped) is None
        pool, off, qual = srs.names_of(np.array([[0, 3]]))
        assert [bytes(pool[off[k]:off[k + 1]]) for k in range(3)] == [n for n, _, _ in recs]
        assert bytes(qual[:int(line_len.sum())]) == b"".join(q + pad for _, _, q in recs)
    # a plain record whose length differs from the one the caller holds is declined as well
    plain = b"@x\nACGT\n+\nIIII\n"
    assert correct._fastq4_names_native(plain, np.array([0], np.int64), np.array([3], np.int64)) is None
    assert correct._fastq4_names_native(plain, np.array([0], np.int64), np.array([4], np.int64)) is not None


def test_from_pool_names():
    srs = correct.ShortReads.from_pool(np.zeros(30, np.uint8), np.array([0, 10, 20, 30], np.int64), chunk_number=3)
    pool, off, qual = srs.names_of(np.array([[1, 3]]))
    assert bytes(pool[:off[-1]]) == b"sr1sr2" and list(off) == [0, 3, 6] and qual is None


# ---------------------------------------------------------------------------- the flag
def test_parse_args_takes_the_flag(tmp_path, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = correct.parse_args(["-l", "lr.fq", "-s", "sr.fq", "-p", str(tmp_path / "o"), "--keep-temporary-files"])
    assert a.keep_temporary_files is True
    assert correct.parse_args(["-l", "lr.fq", "-s", "sr.fq", "-p", "o"]).keep_temporary_files is False


def test_the_flag_is_refused_with_ranks(monkeypatch, capsys):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        correct.parse_args(["-l", "lr.fq", "-s", "sr.fq", "-p", "o", "--keep-temporary-files"])
    assert "one GPU" in capsys.readouterr().err
    assert correct.parse_args(["-l", "lr.fq", "-s", "sr.fq", "-p", "o"]).keep_temporary_files is False
    # the loop refuses it too, before it touches a device: ranks, and the exact-parity layout
    comm = type("Comm", (), {"world": 2, "rank": 0})()
    with pytest.raises(ValueError, match="one GPU"):
        correct.run([], b"", correct.LoopConfig(keep_temporary="x"), stages=object(), comm=comm)
    with pytest.raises(ValueError, match="one GPU"):
        correct.run([], b"", correct.LoopConfig(keep_temporary="x", exact_layout=True), stages=object())

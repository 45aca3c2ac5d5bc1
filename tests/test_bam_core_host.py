"""The device BAM decoder's shared core (proovread_amd/csrc/bam_core.h: fixed fields, aux walk,
SEQ / QUAL / CIGAR unpack) built for the host (tests/native/bam_core_host.cpp) against the host
decoder pr_bam_decode_alns, on records made with pr_sam_encode; malformed aux areas are refused
without a read past the record (every record is decoded from a heap copy of exactly its size, and
the same file runs as a program under AddressSanitizer and UBSan)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import bam_cases
from proovread_amd.bam2cns import _BamAlns

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "bam_core_host.cpp"
PR_ERR_ARG, PR_ERR_SAM = -1, -3


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    out = tmp_path_factory.mktemp("bam_core") / "libbam_core_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", str(out), str(SRC)], check=True)
    L = C.CDLL(str(out))
    L.bam_core_decode.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.POINTER(_BamAlns), C.POINTER(C.POINTER(C.c_int64))]
    L.bam_core_free.argtypes = [C.POINTER(_BamAlns), C.POINTER(C.c_int64)]
    L.bam_core_free.restype = None
    L.bam_core_last_error.restype = C.c_char_p
    return L


def core_decode(L, body: bytes, nlanes: int):
    a = _BamAlns()
    text_at = C.POINTER(C.c_int64)()
    rc = L.bam_core_decode(body, len(body), nlanes, C.byref(a), C.byref(text_at))
    if rc:
        return rc, None
    try:
        cols = bam_cases.take_alns(a)
        for i in range(a.n):   # the host's share of the device path: Perl's number of an AS:Z text
            if text_at[i] >= 0:
                cols["score"][i] = bam_cases.perl_number(body[text_at[i]:body.index(b"\0", text_at[i])])
        return 0, cols
    finally:
        L.bam_core_free(C.byref(a), text_at)


@pytest.fixture(scope="module")
def stream():
    return bam_cases.encode(bam_cases.sam_lines())


@pytest.mark.parametrize("nlanes", [1, 16])
def test_core_equals_host_decoder(core, stream, nlanes):
    rc, want = bam_cases.host_decode(stream)
    assert rc == 0
    rc, got = core_decode(core, stream, nlanes)
    assert rc == 0
    n = len(bam_cases.LSEQS) * 8 * len(bam_cases.NCIGS)
    assert len(want["rid"]) == n and (want["rid"] == -1).any()
    assert set(want["lseq"]) == set(bam_cases.LSEQS) and set(want["ncig"]) == set(bam_cases.NCIGS)
    assert {0, 1, 2, 3, 4} <= set(int(x) for x in want["flags"])   # no AS / AS, QUAL absent, SEQ absent
    bam_cases.assert_same(got, want)


def test_single_records_at_every_pool_offset(core):
    """Records decoded one by one and in pairs: the first pool byte of the second record falls on
    every offset of a 16-byte line."""
    for l in range(0, 36):
        lines = [f"a\t0\tlr0\t1\t60\t{max(l, 1)}M\t*\t0\t0\t{'ACGTN'[l % 5] * l or '*'}\t{'I' * l or '*'}\tAS:i:{l}",
                 "bb\t16\tlr1\t2\t60\t3M1I2M\t*\t0\t0\t" + "ACGTRYKM" * 5 + "\t*"]
        body = bam_cases.encode(lines)
        rc, want = bam_cases.host_decode(body)
        rc2, got = core_decode(core, body, 16)
        assert rc == 0 and rc2 == 0
        bam_cases.assert_same(got, want)


def test_malformed_aux_is_refused(core):
    recs = bam_cases.malformed_records()
    assert len(recs) > 30
    for r in recs:
        assert bam_cases.host_decode(r)[0] == PR_ERR_SAM
        assert core_decode(core, r, 16)[0] == PR_ERR_SAM
        assert core.bam_core_last_error() == b"bad BAM aux field"


def test_size_errors_have_the_host_decoder_texts(core):
    from proovread_amd import _abi
    rec = bam_cases.encode(["q1\t0\tlr0\t5\t60\t4M\t*\t0\t0\tACGT\tIIII"])
    bad_lseq = bytearray(rec)
    bad_lseq[20] = 200
    for body, text in ((rec[:3], "truncated BAM record"), (rec[:-1], "bad BAM record size"),
                       (bytes(bad_lseq), "BAM record fields exceed its size")):
        assert bam_cases.host_decode(body)[0] == PR_ERR_ARG
        assert _abi.lib().pr_last_error().decode() == text
        assert core_decode(core, body, 1)[0] == PR_ERR_ARG
        assert core.bam_core_last_error().decode() == text


def test_program_under_sanitizers(tmp_path):
    """The stand-alone program (its own records, a plain decoder, every truncation of an aux
    area) built with AddressSanitizer and UBSan."""
    exe = tmp_path / "bam_core_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout

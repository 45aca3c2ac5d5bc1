"""PR_BAM_RESTORE_SEQ on the host: the restoring part of proovread_amd/csrc/bam_core.h (key hash and
compare, donor table, CIGAR walk, bam_unpack_seq_from / bam_unpack_qual_from) built for the host
(tests/native/bam_restore_host.cpp) against the rule restated in Python (bam_restore_cases.restore)
followed by the host decoder pr_bam_decode_alns; the same source as a program under
AddressSanitizer and UBSan; and the samfilter drop-in against fixtures made with the reference's
Sam::Parser, Sam::Alignment and Fasta::Seq (tests/golden/gen_samfilter_golden.pl)."""
import ctypes as C
import io
import subprocess
import sys
from pathlib import Path

import pytest

import bam_cases
import bam_restore_cases as rc
from proovread_amd.bam2cns import _BamAlns

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "bam_restore_host.cpp"
GOLD = ROOT / "tests" / "golden"
PR_ERR_SAM, PR_ERR_NOSEQ = -3, -4


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    out = tmp_path_factory.mktemp("bam_restore") / "libbam_restore_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", str(out), str(SRC)], check=True)
    L = C.CDLL(str(out))
    L.bam_restore_decode.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.POINTER(_BamAlns), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), C.POINTER(C.POINTER(C.c_int64))]
    L.bam_restore_free.argtypes = [C.POINTER(_BamAlns), C.POINTER(C.c_int64)]
    L.bam_restore_free.restype = None
    L.bam_restore_last_error.restype = C.c_char_p
    return L


def core_decode(L, body: bytes, nlanes: int = 16):
    """(rc, columns, restored count, {record: donor}) or (rc, None, None, lowest refused record)."""
    a = _BamAlns()
    nr, bad = C.c_int64(), C.c_int64()
    donor_of = C.POINTER(C.c_int64)()
    code = L.bam_restore_decode(body, len(body), nlanes, C.byref(a), C.byref(nr), C.byref(bad), C.byref(donor_of))
    if code:
        return code, None, None, bad.value
    try:
        return 0, bam_cases.take_alns(a), nr.value, {i: donor_of[i] for i in range(a.n) if donor_of[i] >= 0}
    finally:
        L.bam_restore_free(C.byref(a), donor_of)


def check_stream(L, lines, names):
    want_lines, donor_of = rc.restore(lines)
    code, want = bam_cases.host_decode(bam_cases.encode(want_lines, names))
    assert code == 0
    body = bam_cases.encode(lines, names)
    for nlanes in (1, 16):
        code, got, nr, donors = core_decode(L, body, nlanes)
        assert code == 0, L.bam_restore_last_error()
        assert nr == len(donor_of) and donors == donor_of
        bam_cases.assert_same(got, want)
    return want_lines, donor_of


def test_directed_stream_holds_what_it_is_for():
    """The oracle's own output has every case the device test relies on."""
    _, lines = rc.directed()
    out, donor_of = rc.restore(lines)
    f, g = [ln.split("\t") for ln in lines], [ln.split("\t") for ln in out]
    took = sorted(donor_of)
    assert len({x[0] for x in f}) >= 55 and len(took) >= 50
    assert {int(f[i][1]) & 16 for i in took} == {0, 16}                                   # both strands
    assert {(int(f[i][1]) ^ int(f[donor_of[i]][1])) & 16 for i in took} == {0, 16}        # same and other orientation
    forms = {(rc.span(f[i][5])[1] > 0, rc.span(f[i][5])[2] > 0) for i in took}
    assert forms == {(False, False), (True, False), (False, True), (True, True)}          # H at the head, the tail, both
    assert any(rc.span(f[i][5])[1] % 2 == 1 for i in took)                                # an odd leading clip
    assert any(f[donor_of[i]][2] == "lr_out" for i in took)                               # a donor that is not kept
    assert any(f[donor_of[i]][10] == "*" and g[i][10] == "*" for i in took)               # a donor without QUAL
    mates = {int(f[i][1]) & 0xC0 for i in took if f[i][0] == "pair"}
    assert mates == {0x40, 0x80}
    assert all(int(f[donor_of[i]][1]) & 0xC0 == int(f[i][1]) & 0xC0 for i in took)
    assert {len(f[i][0]) for i in took} >= {1, 254}
    assert any(int(x[1]) & 256 and x[9] != "*" for x in f)                                # a record that keeps its own SEQ
    assert any("I" in f[i][5] and "S" in f[i][5] for i in took)
    assert all(x[9] != "*" and len(x[9]) == rc.span(x[5])[0] for x in g)
    assert any(donor_of[i] > i for i in took) and any(donor_of[i] < i for i in took)      # donors on either side


def test_core_equals_oracle_on_the_directed_stream(core):
    _, lines = rc.directed()
    check_stream(core, lines, rc.NAMES)


def test_core_probes_past_collisions(core):
    lines = rc.probing()
    n = len(lines) // 2
    homes = [rc.fnv_home_slot(f"q{i:04d}", 0, 4095) for i in range(n)]
    assert n - len(set(homes)) >= 200                     # hundreds of donors that do not get their home slot
    _, donor_of = check_stream(core, lines, ["lr0", "lr1"])
    assert donor_of == {i: n + i for i in range(n)}


def test_core_lower_index_wins(core):
    lines = ["d\t0\tlr0\t9\t60\t4M\t*\t0\t0\tGGGG\tIIII", "d\t256\tlr0\t10\t0\t4M\t*\t0\t0\t*\t*",
             "d\t0\tlr0\t11\t60\t4M\t*\t0\t0\tACGT\t5555", "d\t1024\tlr1\t1\t60\t4M\t*\t0\t0\tTTTT\t*",
             "d\t272\tlr1\t2\t0\t1H3M\t*\t0\t0\t*\t*"]
    out, donor_of = check_stream(core, lines, ["lr0", "lr1"])
    assert donor_of == {1: 0, 4: 0} and out[4].split("\t")[9:11] == ["CCC", "III"]


@pytest.mark.parametrize("case", sorted(rc.REFUSALS))
def test_core_refuses_as_the_oracle(core, case):
    lines, code, index = rc.REFUSALS[case]
    with pytest.raises(rc.Refused) as e:
        rc.restore(lines)
    assert (e.value.code, e.value.index) == (code, index)
    got = core_decode(core, bam_cases.encode(lines, ["lr0"]))
    assert (got[0], got[3]) == (code, index)


def test_program_under_sanitizers(tmp_path):
    """The stand-alone program (donor lengths 1..70, 255, 256, 1000, every hard-clip split, both
    orientations, by 1 and 16 lanes, guard bytes around the pools) with AddressSanitizer and UBSan."""
    exe = tmp_path / "bam_restore_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all equal" in r.stdout


# ---------------------------------------------------------------------------- samfilter
def _cases(path):
    out, name = {}, None
    for ln in path.read_text().splitlines(keepends=True):
        if ln.startswith("#case "):
            name = ln.split()[1]
            out[name] = []
        else:
            out[name].append(ln)
    return out


def test_samfilter_equals_the_reference_modules():
    from proovread_amd import samfilter
    cases, expected = _cases(GOLD / "samfilter_cases.txt"), _cases(GOLD / "samfilter_expected.txt")
    assert sorted(cases) == sorted(expected) and len(cases) == 4
    assert sum(not ln.startswith("@") for c in cases.values() for ln in c) >= 12
    died = 0
    for name, lines in cases.items():
        if expected[name] == ["!die\n"]:
            with pytest.raises(samfilter.SamfilterError):
                list(samfilter.filter_lines(lines))
            died += 1
        else:
            assert list(samfilter.filter_lines(lines)) == expected[name], name
    assert died == 3


def test_samfilter_command_line():
    cases, expected = _cases(GOLD / "samfilter_cases.txt"), _cases(GOLD / "samfilter_expected.txt")
    for name, status in (("mixed", 0), ("other_name", 255)):
        r = subprocess.run([sys.executable, "-m", "proovread_amd.samfilter"], input="".join(cases[name]), capture_output=True,
                           text=True, cwd=ROOT)
        assert r.returncode == status, r.stderr
        if status == 0:
            assert r.stdout == "".join(expected[name])
        else:
            assert "without primary alignment" in r.stderr


def test_restore_option_needs_external_alignments(tmp_path, capsys):
    """--restore-secondary-seq is a usage error without --sam / --bam; LoopConfig carries it."""
    from proovread_amd import correct
    lr, sr, bam = tmp_path / "lr.fq", tmp_path / "sr.fq", tmp_path / "x.bam"
    for p in (lr, sr, bam):
        p.write_text("")
    with pytest.raises(SystemExit) as e:
        correct.parse_args(["-l", str(lr), "-s", str(sr), "-p", "o", "--restore-secondary-seq"])
    assert e.value.code == 2 and "--restore-secondary-seq needs --sam or --bam" in capsys.readouterr().err
    a = correct.parse_args(["-l", str(lr), "--bam", str(bam), "-p", "o", "--restore-secondary-seq"])
    assert a.restore_secondary_seq and a.mode == "bam"
    assert not correct.parse_args(["-l", str(lr), "--bam", str(bam), "-p", "o"]).restore_secondary_seq
    assert correct.LoopConfig().restore_seq is False

"""The unitig consensus (bam2cns --utg-mode) on the host: the library's host path against the
records of the reference's Perl engine (tests/golden/utg_expected.txt), against the plain-Python
restatement on seeded random reads, through the bam2cns command line, and csrc/utg_core.h alone
under AddressSanitizer and UBSan."""
import functools
import subprocess
from pathlib import Path

import pytest

import utg_cases
import utg_ref
from proovread_amd import bam2cns, utgcns

HERE = Path(__file__).resolve().parent
CASES = utg_cases.read_cases()
EXPECTED = utg_cases.read_expected()


def ref_result(case):
    o = utg_cases.parse_flags(case.flags, case.cfg)
    o.pop("ignore_hcr", None)
    read, _, _ = utg_cases.to_inputs(case)
    if case.fasta:
        o["use_ref_qual"] = False
    return utg_ref.consensus(read.seq, read.qual, read.mcr_ranges(), [utg_ref.Aln.from_sam(s) for s in case.sam], utg_ref.Params(**o))


def as_tuple(res):
    return res.status, res.seq, res.qual, res.trace, [bool(k) for k in res.kept], list(res.windows)


def golden_tuple(case):
    """The expected record as as_tuple gives it (a case the reference dies on: PR_UTG_BAD_ALN)."""
    e = EXPECTED[case.name]
    if e.error:
        return utgcns.BAD_ALN, "", "", "", [False] * len(case.sam), []
    _, seq, _, qual = e.fastq.rstrip("\n").split("\n")
    return 0, seq, qual, e.trace, [s.split("\t")[0] in e.kept for s in case.sam], e.windows


@functools.lru_cache(maxsize=None)
def random_set():
    return tuple(utg_cases.random_cases(7, 300))


def test_golden_cases_are_the_issue_s():
    names = {c.name for c in CASES}
    assert {"qual_weighted", "rep_coverage", "min_ncscore", "fallback_phred", "invert_scores", "full_set", "fasta_ref",
            "mcr_plus_windows", "rep_clamp_start", "rep_clamp_end", "contained_classes", "d_plus_i", "leading_ins_trim0",
            "hard_clips", "max_ins_length", "ins_tie_rank_step2", "ins_tie_rank", "no_survivor", "long_5000", "bad_cigar_eq"} <= names
    assert set(EXPECTED) == names
    for c in CASES:                      # no two alignments of a read of the same length: hash order cannot matter
        lens = [utg_cases.aln_length(s) for s in c.sam]
        assert len(set(lens)) == len(lens), c.name
    head = open(utg_cases.GOLDEN / "utg_expected.txt").read().split(">>CASE")[0]
    digests = [l.split()[-1] for l in head.splitlines() if "PERL_HASH_SEED" in l]
    assert len(digests) == 3 and len(set(digests)) == 1
    # what the cases are about shows in the records
    assert EXPECTED["ins_tie_rank_step2"].fastq != EXPECTED["ins_tie_rank"].fastq
    assert EXPECTED["ins_wins"].trace.count("D") == 5 and EXPECTED["max_ins_length"].trace.count("D") == 0
    assert "u7" in EXPECTED["rep_clamp_start"].kept and "u6" not in EXPECTED["rep_clamp_start"].kept
    assert "u7" not in EXPECTED["rep_clamp_end"].kept
    assert EXPECTED["qual_weighted"].windows == [] and EXPECTED["rep_coverage_zero"].windows == [(0, 300)]
    assert EXPECTED["bad_cigar_eq"].error and sum(e.error for e in EXPECTED.values()) == 1


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_python_restatement_equals_golden(case):
    st, seq, qual, trace, kept, win = ref_result(case)
    assert (st, seq, qual, trace, kept, [tuple(w) for w in win]) == golden_tuple(case)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_path_equals_golden(case):
    read, alns, p = utg_cases.to_inputs(case)
    (res,) = utgcns.run([read], [alns], p, device=False)
    assert as_tuple(res) == golden_tuple(case)
    if not EXPECTED[case.name].error:
        assert res.fastq == EXPECTED[case.name].fastq


def test_host_path_equals_python_restatement_on_random_reads():
    cases = random_set()
    assert any(len(set(map(utg_cases.aln_length, c.sam))) < len(c.sam) for c in cases)   # tied lengths
    n_filtered = n_win = 0
    for c in cases:
        read, alns, p = utg_cases.to_inputs(c)
        (res,) = utgcns.run([read], [alns], p, device=False)
        st, seq, qual, trace, kept, win = ref_result(c)
        assert as_tuple(res) == (st, seq, qual, trace, kept, [tuple(w) for w in win]), (c.name, c.flags, c.cfg)
        n_filtered += (not all(kept)) and st == 0
        n_win += bool(win)
    assert n_filtered > 50 and n_win > 20


def _run_cli(argv):
    try:
        return bam2cns.main(argv)
    except SystemExit as e:
        return e.code


@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
def test_cli_host_writes_the_golden_records(tmp_path, bam):
    for c in CASES:
        argv = utg_cases.write_files(c, tmp_path, bam=bam) + ["--host", "--prefix", str(tmp_path / c.name)]
        rc = _run_cli(argv)
        e = EXPECTED[c.name]
        if e.error:
            assert rc == 255, c.name
            continue
        assert rc == 0, c.name
        assert (tmp_path / (c.name + ".fq")).read_text() == e.fastq, c.name
        assert (tmp_path / (c.name + ".debug.trace")).read_text() == e.fastq + e.trace + "\n", c.name
        assert (tmp_path / (c.name + ".chim.tsv")).read_text() == ""


def test_cli_names_the_read_and_the_flag(tmp_path, capsys):
    c = next(c for c in CASES if c.name == "bad_cigar_eq")
    assert _run_cli(utg_cases.write_files(c, tmp_path) + ["--host", "--prefix", str(tmp_path / "o")]) == 255
    err = capsys.readouterr().err
    assert "lr_bad_cigar_eq" in err and "PR_UTG_BAD_ALN" in err


@pytest.mark.parametrize("extra", [["--qual-weighted"], ["--rep-coverage", "7"], ["--min-ncscore", "3.3"], ["--host"],
                                   ["--utg-mode", "--detect-chimera", "--host"], ["--utg-mode", "--haplo-coverage", "--host"]],
                         ids=lambda x: " ".join(x))
def test_refused_combinations_exit_255(tmp_path, extra):
    c = CASES[0]
    argv = [a for a in utg_cases.write_files(c, tmp_path) if a != "--utg-mode"]
    assert _run_cli(argv + extra + ["--prefix", str(tmp_path / "o")]) == 255


def test_star_seq_dies(tmp_path):
    c = CASES[0]
    argv = utg_cases.write_files(c, tmp_path)
    sam = Path(argv[1])
    f = c.sam[0].split("\t")
    f[9] = f[10] = "*"
    sam.write_text(sam.read_text() + "\t".join(f) + "\n")
    assert _run_cli(argv + ["--host", "--prefix", str(tmp_path / "o")]) == 255


def test_capacities_are_flagged_and_neighbours_exact():
    import random
    from proovread_amd import cns
    rng = random.Random(5)
    small, alns, p = utg_cases.to_inputs(CASES[0])
    long_seq = utg_cases.rand_seq(rng, utgcns.MAX_LEN + 1)
    too_long = cns.LongRead("too_long", long_seq, "5" * len(long_seq), "")
    many = [cns.SamRecord.from_line(utg_cases.sam_line(rng, f"m{i}", "too_many", small.seq, i % 100, [(60, "M")], 100))
            for i in range(utgcns.MAX_ALNS + 1)]
    too_many = cns.LongRead("too_many", small.seq, small.qual, "")
    res = utgcns.run([too_long, small, too_many, small], [[], alns, many, alns], p, device=False)
    assert [r.status for r in res] == [utgcns.TOO_LONG, 0, utgcns.TOO_MANY, 0]
    assert res[0].seq == "" and res[2].seq == "" and not res[2].kept.any()
    assert as_tuple(res[1]) == as_tuple(res[3]) == golden_tuple(CASES[0])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("utg_core") / "utg_core_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(out), str(HERE / "native" / "utg_core_host.cpp")], check=True)
    return out


def test_core_header_under_sanitizers_writes_the_golden_records(exe, tmp_path):
    gold = tmp_path / "golden.txt"
    utg_cases.write_cases(gold, CASES)
    r = subprocess.run([str(exe), str(gold)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = "".join(l for l in open(utg_cases.GOLDEN / "utg_expected.txt") if not l.startswith("#"))
    assert r.stdout == want
    rnd = tmp_path / "random.txt"
    cases = random_set()[:60]
    utg_cases.write_cases(rnd, cases)
    r = subprocess.run([str(exe), str(rnd)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = tmp_path / "random_out.txt"
    out.write_text(r.stdout)
    got = utg_cases.read_expected(out)
    for c in cases:
        read, alns, p = utg_cases.to_inputs(c)
        (res,) = utgcns.run([read], [alns], p, device=False)
        g = got[c.name]
        assert g.error == (res.status != 0), c.name
        if not g.error:
            assert (g.fastq, g.trace, g.windows) == (res.fastq, res.trace, res.windows), c.name


"""The siamaera stage on the host (proovread_amd.siamaera over pr_siam_*; bin/siamaera).

The stage is defined by DESIGN.md §9 (parity with blastn is unpinned); the library is held
equal to the plain-Python restatement tests/siamaera_ref.py, its extension also to
oracle/sw_oracle.c osw_extend, its record editing to the reference's Fastq::Seq / Fasta::Seq
(tests/golden/siamaera_records.txt).  Runs without a GPU.
"""
import os
import random
import subprocess
import sys
from pathlib import Path

import pytest

import oracle_bind
import siamaera_ref as R
from proovread_amd import siamaera as S

ROOT = Path(__file__).resolve().parent.parent
SETS = (("pass1", R.PASS1), ("pass2", R.PASS2))


def _aligner(name):
    return getattr(S.default_params(), name)


def _b(s):
    return s.encode()


# ---------------------------------------------------------------------------- extension
def test_default_parameter_sets():
    p = S.default_params()
    assert (p.seq_min_len, p.term_ignore_len, p.trim, p.filter_inconclusive, p.aln_min_idy) == (150, 10, 5, 1, 97.5)
    for name, prm in SETS:
        al = getattr(p, name)
        assert {k: getattr(al, k) for k in prm} == prm


@pytest.mark.parametrize("name,prm", SETS)
def test_extend_equals_oracle_and_ref(name, prm):
    al = _aligner(name)
    ref = R.extension_ref()[name]
    n_end = 0
    for k, (q, t, h0) in enumerate(R.extension_pairs()):
        got = S.extend(_b(q), _b(t), h0, al)
        sc, outs = oracle_bind.sw_extend(q, t, h0, w=prm["w"], a=prm["a"], b=prm["b"], o_del=prm["o"], e_del=prm["e"],
                                         o_ins=prm["o"], e_ins=prm["e"], end_bonus=0, zdrop=prm["zdrop"])
        assert got[:3] == (sc, outs[0], outs[1]), (k, len(q), len(t), h0)
        assert got == ref[k], (k, len(q), len(t), h0)
        assert got[3] <= got[4] and got[4] >= max(got[1], got[2])
        n_end += got[1] == len(q)
    assert n_end > 20   # the set reaches the query's end often enough to matter


def test_extend_empty_side_is_not_extended():
    assert S.extend(b"", b"ACGT", 28) == (28, 0, 0, 0, 0)
    assert S.extend(b"ACGT", b"", 28) == (28, 0, 0, 0, 0)


# ---------------------------------------------------------------------------- seeds
def test_seeds_equal_ref_on_edge_lengths():
    n = 0
    for r in R.seed_edge_reads():
        got = S.seeds(_b(r))
        assert got == R.seeds(R.nt4(r), 28), len(r)
        n += len(got)
    assert n > 100
    # a palindrome's main anti-diagonal is one seed from end to end; N at the centre splits it
    x = R.rand_seq(random.Random(5), 32)
    assert S.seeds(_b(x + R.rc(x)))[0] == (0, 63, 64)
    assert S.seeds(_b(x + R.rc(x)[:13])) == []                     # a run of 26
    assert S.seeds(_b(x + R.rc(x)[:14])) == [(18, 45, 28)]         # ... of 28, up to the read's end
    pal = x + R.rc(x)
    assert S.seeds(_b(pal[:31] + "N" + pal[32:]))[:2] == [(0, 63, 31), (33, 30, 31)]


# ---------------------------------------------------------------------------- known answers
KNOWN = [
    ("joined", [(1, 800, 800, 1)], (S.TRIM, 405, 800)),
    ("split", [(1, 400, 840, 441), (441, 840, 400, 1)], (S.TRIM, 445, 840)),
    ("short_tail", [(251, 400, 590, 441), (441, 590, 400, 251)], (S.TRIM, 0, 395)),
    ("short_head", [(1, 150, 340, 191), (191, 340, 150, 1)], (S.TRIM, 195, 590)),
    ("random", [], (S.KEEP, 0, 1000)),
]


@pytest.mark.parametrize("name,want_hsps,want", KNOWN)
def test_known_answers(name, want_hsps, want):
    read = R.known()[name]
    hs, st = S.hsps([_b(read)], device=False)
    assert st.tolist() == [0]
    assert [h[:4] for h in hs[0]] == want_hsps
    assert (hs[0], 0) == R.hsps(R.nt4(read))
    assert all(h[4] == h[5] == h[6] == h[1] - h[0] + 1 for h in hs[0])   # perfect arms: every column a match
    dec, st, summ = S.run([_b(read)], device=False)
    assert tuple(dec[0]) == want and st.tolist() == [0]
    assert tuple(dec[0]) == R.run(R.nt4(read))[:3]
    assert summ == {"scanned": 1, "trimmed": int(want[0] == S.TRIM), "inconclusive": 0, "flagged": 0}


def test_stubby_palindrome_is_not_searched():
    read = R.known()["stubby"]
    assert len(read) == 140 and S.hsps([_b(read)], device=False)[0][0]   # it does align with itself
    dec, _, summ = S.run([_b(read)], device=False)
    assert tuple(dec[0]) == (S.KEEP, 0, 140) and summ["trimmed"] == 0


def test_joined_record_tag():
    read = R.known()["joined"]
    out, _ = S.filter_records([("r1", "", _b(read), b"I" * len(read))], device=False)
    assert out == [("r1", "SUBSTR:405 SIAMAERA:405,800", _b(read[405:]), b"I" * 395)]


# ---------------------------------------------------------------------------- mutated arms
def _mutated(rate):
    K = R.known()
    rng = random.Random(1000 + int(rate * 100))
    return K["X"] + K["J"] + R.rc(R.mutate(rng, K["X"], rate))


@pytest.mark.parametrize("rate", [0.01, 0.02, 0.04])
def test_mutated_arms_equal_ref(rate):
    read = _mutated(rate)
    hs, st = S.hsps([_b(read)], device=False)
    assert (hs[0], int(st[0])) == R.hsps(R.nt4(read))
    assert all(100.0 * h[5] >= 97.5 * h[4] for h in hs[0])
    every, _ = S.hsps([_b(read)], min_idy=0.0, device=False)
    assert every[0] == R.hsps(R.nt4(read), R.PASS1, 0.0)[0]
    assert [h for h in every[0] if 100.0 * h[5] >= 97.5 * h[4]] == hs[0]
    assert all(h[5] < h[4] for h in every[0])    # the arms do differ


def test_identity_threshold_decides_mutated_arms():
    """By the ref, the 1 % arm passes pass 1 (the read is trimmed at the joint) and the 4 % arm
    aligns end to end but fails the 97.5 % threshold (the read stays)."""
    lo, hi = _mutated(0.01), _mutated(0.04)
    assert R.run(R.nt4(lo))[:3] == (R.TRIM, 445, len(lo))
    assert R.hsps(R.nt4(hi)) == ([], 0) and len(R.hsps(R.nt4(hi), R.PASS1, 0.0)[0]) == 2
    dec, _, _ = S.run([_b(lo), _b(hi)], device=False)
    assert dec.tolist() == [[S.TRIM, 445, len(lo)], [S.KEEP, 0, len(hi)]]


def test_pass2_and_inconclusive_reads_equal_ref():
    """More than 2 alignments after the filter: pass 2 runs; its list resolves one read and
    leaves the other inconclusive (dropped, or kept with --no-filter-inconclusive)."""
    M = R.multi_arm_reads()
    for name, want in (("resolved", (S.TRIM, 5, 965)), ("inconclusive", (S.DROP, 0, 1800))):
        read = M[name]
        h1 = R.hsps(R.nt4(read))[0]
        assert len(R.spurious(h1, len(read))) > 2, name
        dec, st, summ = S.run([_b(read)], device=False)
        assert tuple(dec[0]) == want == R.run(R.nt4(read))[:3], name
        assert summ["inconclusive"] == int(name == "inconclusive") and st.tolist() == [0]
    read = M["inconclusive"]
    dec, _, summ = S.run([_b(read)], S.default_params(filter_inconclusive=0), device=False)
    assert tuple(dec[0]) == (S.KEEP, 0, 1800) == R.run(R.nt4(read), filter_inconclusive=False)[:3]
    assert summ["inconclusive"] == 1 and summ["trimmed"] == 0
    recs = [("a", "", _b(M["inconclusive"]), None), ("b", "", _b(R.known()["random"]), None)]
    assert S.filter_records(recs, device=False)[0] == recs[1:]
    assert S.filter_records(recs, S.default_params(filter_inconclusive=0), device=False)[0] == recs


# ---------------------------------------------------------------------------- decision
B0, B1 = (1, 400, 1000, 601), (601, 1000, 400, 1)
DECISIONS = [
    # name, L, pass 1 list, pass 2 list, filter_inconclusive, (action, from, to, inconclusive)
    # t = int(0.05 * 1000 + 0.5) + 1 = 51: a partner 50 off still counts, the spurious hit goes
    ("tolerance-in", 1000, [B0, (601, 1000, 450, 51), (300, 350, 700, 651)], [], 1, (S.TRIM, 605, 1000, False)),
    # 51 off: B0 loses its partner; the one hit left ends at the read's end: int(199 + 601 - 5 + .5)
    ("tolerance-out", 1000, [B0, (601, 1000, 451, 52), (300, 350, 700, 651)], [], 1, (S.TRIM, 0, 795, False)),
    # a self-symmetric hit of 80 <= 0.7 * 150 is removed; the pair is left: j = 601 - 1 + 5
    ("short-joint", 1000, [B0, B1, (480, 560, 560, 480)], [], 1, (S.TRIM, 605, 1000, False)),
    # B0 has two partners that have none themselves: B0 is pushed twice, and two hits take the
    # split rule (one hit would give int(199 + 1 + 5 + .5) = 205)
    ("duplicate", 1000, [B0, (700, 900, 400, 1), (720, 950, 405, 3)], [], 1, (S.TRIM, 605, 1000, False)),
    # a self-symmetric hit of 110 stays: three hits, no pass-2 result
    ("inconclusive-drop", 1000, [B0, B1, (450, 560, 560, 450)], [], 1, (S.DROP, 0, 1000, True)),
    ("inconclusive-keep", 1000, [B0, B1, (450, 560, 560, 450)], [], 0, (S.KEEP, 0, 1000, True)),
    # ... and with one: pass 2's list replaces it
    ("pass2-replaces", 1000, [B0, B1, (450, 560, 560, 450)], [B0, B1], 1, (S.TRIM, 605, 1000, False)),
    ("neither-end", 1000, [(200, 400, 800, 600)], [], 1, (S.KEEP, 0, 1000, False)),
    ("two-neither-end", 1000, [(200, 400, 800, 600), (600, 800, 400, 200)], [], 1, (S.KEEP, 0, 1000, False)),
    ("stubby", 140, [(1, 140, 140, 1)], [], 1, (S.KEEP, 0, 140, False)),
]


@pytest.mark.parametrize("name,L,h1,h2,fi,want", DECISIONS, ids=[d[0] for d in DECISIONS])
def test_decision(name, L, h1, h2, fi, want):
    p = S.default_params(filter_inconclusive=fi)
    assert S.decide(L, h1, h2, p) == want
    assert R.decide(L, h1, h2, filter_inconclusive=bool(fi)) == want


def test_tolerance_in_case_by_hand():
    """tolerance-in: the pair survives the filter, the first hit starts at the read's start:
    j = sae - 1 + trim = 601 - 1 + 5."""
    assert R.spurious([B0, (601, 1000, 450, 51), (300, 350, 700, 651)], 1000) == [B0, (601, 1000, 450, 51)]
    # the first qualifying hit wins: B0 (qas 1), whose sae is 601
    assert R.decide(1000, [B0, (601, 1000, 450, 51)])[:3] == (R.TRIM, 605, 1000)


# ---------------------------------------------------------------------------- records and outputs
def _golden():
    txt = (ROOT / "tests" / "golden" / "siamaera_records.txt").read_bytes()
    for block in txt.split(b"END\n"):
        if not block:
            continue
        head, rec = block.split(b"\n", 1)
        f = head.decode("latin-1").split("\t")
        assert f[0] == "CASE"
        yield f[1], f[2], int(f[3]), f[4], f[5].encode(), f[6].encode(), rec


def test_record_editing_equals_reference_modules():
    from proovread_amd.seqfilter import _rec, format_record
    n = 0
    for kind, form, j, head, seq, qual, want in _golden():
        r = _rec(head[1:].encode("latin-1"), seq, qual if kind == "fastq" else None)
        e = S.edit_record(r, j, len(seq)) if form == "tail" else S.edit_record(r, 0, j)
        assert format_record(e, kind == "fasta", 0) == want, (kind, form, j, head)
        n += 1
    assert n == 9


def _fastq(reads):
    return "".join(f"@r{k} d{k}\n{r}\n+\n{'I' * len(r)}\n" for k, r in enumerate(reads)).encode()


def _cli(args, data=b""):
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "proovread_amd.siamaera", *args], input=data, capture_output=True, env=env)


def test_cli_host_stdin_to_stdout():
    K = R.known()
    reads = [K["random"], K["split"], K["stubby"], K["short_tail"]]
    r = _cli(["--host", "--blast-path", "/nowhere", "-c", "x.cfg"], _fastq(reads))
    assert r.returncode == 0, r.stderr
    q = "I"
    want = (f"@r0 d0\n{reads[0]}\n+\n{q * 1000}\n"
            f"@r1 d1 SUBSTR:445 SIAMAERA:445,840\n{reads[1][445:]}\n+\n{q * 395}\n"
            f"@r2 d2\n{reads[2]}\n+\n{q * 140}\n"
            f"@r3 d3 SUBSTR:0,395 SIAMAERA:0,395\n{reads[3][:395]}\n+\n{q * 395}\n")
    assert r.stdout.decode() == want
    err = r.stderr.decode()
    assert "Summary:\n4 reads scanned\n2 siamaeras trimmed (50.00%)\n0 potential siamaeras with multiple, " \
           "unresolved HSPs filtered (0.00%)" in err
    # FASTA in, FASTA out (one line per sequence, as Fasta::Seq prints)
    r = _cli(["--host"], f">a x\n{reads[1][:420]}\n{reads[1][420:]}\n".encode())
    assert r.returncode == 0 and r.stdout.decode() == f">a x SUBSTR:445 SIAMAERA:445,840\n{reads[1][445:]}\n"


def test_cli_version_and_shim():
    r = _cli(["-V"])
    assert r.returncode == 0 and r.stdout == b"0.01\n"
    shim = ROOT / "bin" / "siamaera"
    assert os.access(shim, os.X_OK) and "proovread_amd.siamaera" in shim.read_text()


def _loop_result():
    from proovread_amd import correct
    rng = random.Random(31)
    K = R.known()
    plain = [R.rand_seq(rng, 900), R.rand_seq(rng, 1200)]
    arm = R.rand_seq(rng, 700)
    sia = arm + K["J"] + R.rc(arm)
    seqs = [plain[0], sia, plain[1]]
    reads = correct.LongReads(["lr0", "lr1", "lr2"], [_b(s) for s in seqs], [b"I" * len(s) for s in seqs])
    return correct.LoopResult(reads, [], [], []), sia


def test_write_outputs_with_siamaera_loses_the_arm(tmp_path):
    from proovread_amd import correct
    from proovread_amd.seqfilter import read_records
    res, sia = _loop_result()
    plain, on = str(tmp_path / "plain"), str(tmp_path / "on")
    assert correct.write_outputs(res, plain) is None
    summ = correct.write_outputs(res, on, siamaera=True, siamaera_device=False)
    assert summ == {"scanned": 3, "trimmed": 1, "inconclusive": 0, "flagged": 0}
    a, b = read_records(plain + ".trimmed.fq"), read_records(on + ".trimmed.fq")
    assert [r[0] for r in a] == [r[0] for r in b] == ["lr0", "lr1", "lr2"]
    assert a[1][2] == _b(sia) and b[1][2] == _b(sia[745:]) and len(b[1][3]) == 695
    assert b[1][1].endswith("SUBSTR:745 SIAMAERA:745,1440")
    assert (a[0], a[2]) == (b[0], b[2])
    assert [r[2] for r in read_records(on + ".trimmed.fa")] == [r[2] for r in b]
    for ext in (".untrimmed.fq", ".chim.tsv", ".ignored.tsv"):
        assert Path(plain + ext).read_bytes() == Path(on + ext).read_bytes()


def test_default_outputs_are_what_seqfilter_alone_writes(tmp_path):
    """siamaera=False (the default) leaves every file as the SeqFilter calls write it."""
    from proovread_amd import correct, seqfilter
    res, _ = _loop_result()
    pre = str(tmp_path / "d")
    correct.write_outputs(res, pre)
    ref = str(tmp_path / "ref")
    assert seqfilter.run(["--trim-win", "12,5", "--min-length", "500", "--substr", pre + ".chim.tsv", "--in",
                          pre + ".untrimmed.fq", "--out", ref + ".fq", "--phred-offset", "33"]) == 0
    seqfilter.run(["--in", ref + ".fq", "--out", ref + ".fa", "--fasta", "--phred-offset", "33"])
    assert Path(pre + ".trimmed.fq").read_bytes() == Path(ref + ".fq").read_bytes()
    assert Path(pre + ".trimmed.fa").read_bytes() == Path(ref + ".fa").read_bytes()
    assert Path(pre + ".untrimmed.fq").read_text() == res.reads.fastq()


# ---------------------------------------------------------------------------- capacities
def test_flagged_reads_pass_unchanged():
    """More than 1,024 seeds: the read is flagged, has no alignments, is written unchanged and
    counted; the call succeeds."""
    at = "AT" * 700
    assert len(R.seeds(R.nt4(at), 28)) > R.MAX_SEEDS
    hs, st = S.hsps([_b(at), _b(R.known()["joined"])], device=False)
    assert st.tolist() == [S.SEED_OVERFLOW, 0] and hs[0] == [] and len(hs[1]) == 1
    recs = [("a", "", _b(at), None), ("b", "", _b(R.known()["joined"]), None)]
    out, summ = S.filter_records(recs, device=False)
    assert out[0] == recs[0] and len(out[1][2]) == 395
    assert summ == {"scanned": 2, "trimmed": 1, "inconclusive": 0, "flagged": 1}
    assert R.hsps(R.nt4(at)) == ([], R.SEED_OVERFLOW)

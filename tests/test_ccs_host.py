"""ccs-1 on the host: grouping and mapping against the plain-Python restatement (ccs_ref.py),
the consensus against the C oracle of Sam::Seq and against records the reference's Perl engine
wrote, the accuracy of the rules on simulated ZMWs, and the command line."""
import io
import random
import re
from pathlib import Path

import pytest

import casefmt
import ccs_cases
import ccs_ref
import oracle_bind
from proovread_amd import ccseq, tasks as T

GOLDEN = Path(__file__).resolve().parent / "golden"
ROLE = {ccseq.SECONDARY: "secondary", ccseq.PRIMARY: "primary", ccseq.SINGLE: "single"}


# ---------------------------------------------------------------------------- grouping
def _ids(spec):
    """'a:300 a:200 b:100' -> ids of ZMWs a, b, .. and the lengths"""
    ids, lens, at = [], [], 0
    for k, tok in enumerate(spec.split()):
        z, n = tok.split(":")
        ids.append(f"m140101_x/{ord(z)}/{at}_{at + int(n)}")
        lens.append(int(n))
        at += int(n) + 30
    return ids, lens


@pytest.mark.parametrize("spec", [
    "a:300 a:200",                      # two subreads, the first strictly longer
    "a:200 a:300", "a:250 a:250",       # otherwise the second
    "a:100 a:900 a:300 a:50",           # more than two: the second
    "a:100 b:100 c:100 c:90 d:100",     # singles; a lone last record is lost
    "a:100 a:90 b:70",
    "a:100 b:100 b:200 b:300 c:10 c:20",
])
def test_grouping_equals_the_restatement(spec):
    ids, lens = _ids(spec)
    role, grp, ng = ccseq.group(ids, lens)
    want_roles, want_groups = ccs_ref.group_ref(ids, lens)
    assert [ROLE[int(r)] for r in role] == want_roles
    got = [[k for k in range(len(ids)) if grp[k] == g] for g in range(ng)]
    assert got == want_groups
    assert all(grp[k] == -1 for k in range(len(ids)) if not any(k in g for g in want_groups))


def test_a_lone_last_record_is_lost():
    ids, lens = _ids("a:100 a:90 b:70")
    recs = [(i, "d", b"A" * n, b"5" * n) for i, n in zip(ids, lens)]
    out, stats = ccseq.ccs_records(recs, device=False)
    assert [r[0] for r in out] == [ids[0]] and stats["secondary"] == 2 and stats["single"] == 0


@pytest.mark.parametrize("ids,kind,index", [
    (["m1/1/0_10", "m1/1/20_30", "read7"], "not_subread", 2),
    (["m1/1/0_10", "m1/2/0_10x", "m/1/0_10", "m1/1/20_30"], "not_subread", 2),
    (["m1/1/0_10", "m1//0_10"], "not_subread", 1),
    (["xm1/1/0_10"], "not_subread", 0),
    (["m1/1/0_10", "m1/2/0_10", "m1/1/0_10"], "not_unique", 2),
    (["m1/1/0_10 desc".split()[0], "m1/1/0_", "m1/1/0_10"], "not_subread", 1),
])
def test_ids_ccseq_dies_on(ids, kind, index):
    with pytest.raises(ccs_ref.BadId) as want:
        ccs_ref.group_ref(ids, [10] * len(ids))
    assert (want.value.kind, want.value.index) == (kind, index)
    with pytest.raises(ccseq.SubreadIdError) as got:
        ccseq.group(ids, [10] * len(ids))
    assert got.value.index == index
    assert got.value.kind == (ccseq.ID_NOT_SUBREAD if kind == "not_subread" else ccseq.ID_NOT_UNIQUE)


# ---------------------------------------------------------------------------- mapping
def _sim_groups(seed, n, lo, hi, passes, **kw):
    rng = random.Random(seed)
    out = []
    for z in range(n):
        insert, recs = ccs_ref.sim_zmw(rng, "m150101_1_s1_p0", z, rng.randrange(lo, hi + 1), rng.randrange(*passes), **kw)
        ids = [r[0] for r in recs]
        role, _, _ = ccseq.group(ids, [len(r[1]) for r in recs])
        out.append((insert, ids, ([r[1].encode() for r in recs], [r[2].encode() for r in recs], list(role).index(ccseq.PRIMARY))))
    return out


def _check_mapping(groups, w):
    p = ccseq.default_params(w=w)
    rp = dict(ccs_ref.PARAMS, w=w)
    got = ccseq.map_groups(groups, p, device=False, threads=4)
    for (seqs, _, ref), ga in zip(groups, got):
        assert ga[ref] is None   # -e: the reference is not aligned to itself
        for t, a in enumerate(ga):
            if t != ref:
                assert a == ccs_ref.map_ref(seqs[ref].decode(), seqs[t].decode(), rp), (w, t)
    return got


@pytest.mark.parametrize("w,n,hi", [(8, 6, 260), (300, 3, 200)])
def test_mapping_equals_the_restatement(w, n, hi):
    groups = [g for _, _, g in _sim_groups(100 + w, n, 120, hi, (3, 6))]   # partial first and last passes
    got = _check_mapping(groups, w)
    alns = [a for ga in got for a in ga if a is not None]
    assert len(alns) >= 2 * n
    assert any(a[0] == 1 for a in alns) and any(a[0] == 0 for a in alns)   # both strands
    assert any("I" in a[3] for a in alns) and any("D" in a[3] for a in alns)


def test_mapping_clips_ns_and_no_seed():
    rng = random.Random(9)
    ref = ccs_cases.rand_seq(rng, 200)
    inner = ref[40:160]
    with_n = inner[:50] + "NNN" + inner[53:]
    clipped = ccs_cases.rand_seq(rng, 17) + inner + ccs_cases.rand_seq(rng, 11)
    rev = ccs_ref.revcomp(clipped)
    foreign = ccs_cases.rand_seq(random.Random(10), 150)
    seqs = [clipped, ref, with_n, rev, foreign, "N" * 60]
    grp = ([s.encode() for s in seqs], [b"5" * len(s) for s in seqs], 1)
    for w in (8, 300):
        (ga,) = _check_mapping([grp], w)
        assert ga[0][0] == 0 and ga[3][0] == 1 and ga[0][2] >= 600 and ga[3][2] >= 600   # both strands, >= the 120 matches
        assert re.fullmatch(r"\d+S[0-9MID]+\d+S", ga[0][3]) and re.fullmatch(r"\d+S[0-9MID]+\d+S", ga[3][3])   # -Y: soft clips
        assert ga[2][0] == 0 and ga[2][1] == 40 and ga[2][3] == "120M" and ga[2][2] == 117 * 5 - 3   # N scores -1
        assert ga[4] is None and ga[5] is None   # no seed, no alignment


# ---------------------------------------------------------------------------- consensus
def _oracle(case, **over):
    o = oracle_bind.run_case(case, **dict(ccs_cases.ORACLE_OVER, **over))
    assert o["rc"] == 0, o
    return o


def _host_fastq(rid, res):
    return f"@{rid}\n{res[1].decode()}\n+\n{res[2].decode('latin-1')}\n"


def _check_case(name, ref, rq, alns, **pover):
    case = ccs_cases.to_case(name, ref, rq, alns)
    grp, ga = ccs_cases.to_group(ref, rq, alns)
    (res,) = ccseq.consensus_groups([grp], [ga], ccseq.default_params(**pover), device=False)
    o = _oracle(case, **({"trim": pover["trim"]} if "trim" in pover else {}))
    assert res[0] == 0
    assert _host_fastq(case.ref_id, res) == o["fastq"], name
    assert res[3].decode() == o["trace"], name
    return case, o


@pytest.fixture(scope="module")
def hand():
    return ccs_cases.hand_cases()


@pytest.mark.parametrize("name", ["ins_tie_rank", "skip_277", "skip_354", "skip_384", "del_ins_pair", "leading_ins",
                                  "del_quals", "ref_alone"])
def test_consensus_equals_the_oracle_on_hand_cases(hand, name):
    _check_case(name, *hand[name])


def _without(case, k, **over):
    return _oracle(casefmt.Case(case.name, case.params, case.ref, [ln for j, ln in enumerate(case.sam) if j != k]), **over)


def test_the_hand_cases_reach_what_they_are_for(hand):
    """From the oracle alone: each skip, the D+I pair, the leading insertion and the rank tie occur."""
    # Seq.pm:277, 354, 384: the first alignment changes nothing; without trimming the latter two would
    for name, by_trim in (("skip_277", False), ("skip_354", True), ("skip_384", True)):
        ref, rq, alns = hand[name]
        case = ccs_cases.to_case(name, ref, rq, alns)
        assert _oracle(case)["fastq"] == _without(case, 0)["fastq"]
        assert (_oracle(case, trim=0)["fastq"] != _without(case, 0, trim=0)["fastq"]) == by_trim
    assert len(hand["skip_277"][2][0][0]) == 50
    s, _, _, cig = hand["skip_354"][2][0]
    assert 60 / len(s) < 0.7 and cig == "25S60M15S"
    s, _, _, cig = hand["skip_384"][2][0]
    assert len(s) == 1000 and 701 / 1000 >= 0.7 > 699 / 1000 and int(1000 * 0.001 + 0.5) == 1
    assert cig == "299S350M1D349M1I1M"
    kept = list(hand["skip_384"][2])   # the same 701 bases without a tail to cut are added
    kept[0] = (s[:999] + hand["skip_384"][0][30 + 700], kept[0][1], 30, "299S350M1D351M")
    case = ccs_cases.to_case("skip_384", hand["skip_384"][0], hand["skip_384"][1], kept)
    assert _oracle(case)["fastq"] != _without(case, 0)["fastq"]
    # the D+I pair: the consensus has the insertion's bases in place of the gap, and a mismatch for 1D1I
    ref, rq, alns = hand["del_ins_pair"]
    o = _oracle(ccs_cases.to_case("del_ins_pair", ref, rq, alns))
    seq = o["fastq"].split("\n")[1]
    s = alns[0][0]
    assert seq == ref[:40] + s[40:43] + ref[42:72] + s[73] + ref[73:] and s[73] != ref[72]   # column 40 a gap, 41 TGA, 72 a mismatch
    assert o["trace"] == "M" * 40 + "IMDD" + "M" * 88
    # the leading insertion: trimmed with Trim 1 (the oracle writes the same as for a clip), a state without
    ref, rq, alns = hand["leading_ins"]
    case = ccs_cases.to_case("leading_ins", ref, rq, alns)
    as_clip = ccs_cases.to_case("leading_ins", ref, rq, [(alns[0][0], alns[0][1], alns[0][2], "3S20M2D90M"), alns[1]])
    assert _oracle(case)["fastq"] == _oracle(as_clip)["fastq"]
    assert _oracle(case, trim=0)["fastq"] != _oracle(as_clip, trim=0)["fastq"]
    # the tie: ATT wins column 50 although AGG comes first in the column
    ref, rq, alns = hand["ins_tie_rank"]
    o = _oracle(ccs_cases.to_case("ins_tie_rank", ref, rq, alns))
    assert o["fastq"].split("\n")[1] == ref[:51] + "TT" + ref[51:]
    flipped = _oracle(ccs_cases.to_case("ins_tie_rank", ref, rq, alns[::-1]))
    assert flipped["fastq"].split("\n")[1] == ref[:51] + "TT" + ref[51:]   # seen first either way: not column order


def test_leading_insertion_state_without_trimming(hand):
    """Seq.pm:425-428 (`$i == 0`): reachable only with Trim 0; the stage keeps the branch."""
    _check_case("leading_ins", *hand["leading_ins"], trim=0)
    _check_case("del_quals", *hand["del_quals"], trim=0)


@pytest.mark.parametrize("w", [8, 300])
def test_consensus_of_mapped_groups_equals_the_oracle(w):
    sims = _sim_groups(40 + w, 5, 150, 300, (2, 7))
    groups = [g for _, _, g in sims]
    p = ccseq.default_params(w=w)
    results, alns, _ = ccseq.run_groups(groups, p, device=False, threads=4)
    assert results == ccseq.consensus_groups(groups, alns, p, device=False)
    for (_, ids, grp), ga, res in zip(sims, alns, results):
        seqs, quals, ref = grp
        case = casefmt.Case("sim", {"qual_weighted": "1", "use_ref_qual": "1"},
                            ["@" + ids[ref], seqs[ref].decode(), "+", quals[ref].decode()], ccseq.sam_lines(ids, grp, ga))
        o = _oracle(case)
        assert _host_fastq(ids[ref], res) == o["fastq"] and res[3].decode() == o["trace"]


def test_malformed_alignments_are_flagged(hand):
    ref, rq, alns = hand["skip_277"]
    grp, ga = ccs_cases.to_group(ref, rq, alns)
    for bad in ("139M", "140M6D", "70M3S67M", "150M", "140N"):
        ga2 = list(ga)
        ga2[2] = (0, 5 if bad != "150M" else 20, 100, bad)
        (res,) = ccseq.consensus_groups([grp], [ga2], device=False)
        assert res[0] == ccseq.BAD_ALN and res[1] == b""


# ---------------------------------------------------------------------------- Perl goldens
def test_host_consensus_equals_the_perl_records():
    cases = casefmt.read_cases(GOLDEN / "ccs_cases.txt")
    expect = casefmt.read_expect(GOLDEN / "ccs_expected.txt")
    assert len(cases) >= 10
    for case in cases:
        e = expect[case.name]
        assert not e.error, case.name
        alns = ccs_cases.case_alns(case)
        grp, ga = ccs_cases.to_group(case.ref[1], case.ref[3], alns)
        (res,) = ccseq.consensus_groups([grp], [ga], device=False)
        assert res[0] == 0
        assert [f"@{case.ref_id} CCS:primary", res[1].decode(), "+", res[2].decode("latin-1")] == e.fastq, case.name
        assert res[3].decode() == e.trace, case.name


# ---------------------------------------------------------------------------- accuracy
def test_consensus_is_closer_to_the_insert_than_the_reference_subread():
    """SURVEY.md §8d's CLR error model, >= 5 alternating-strand passes: the summed edit distance
    of the primary outputs to their inserts is strictly below that of the subreads they replace."""
    sims = _sim_groups(2024, 6, 250, 400, (5, 8))
    results, _, _ = ccseq.run_groups([g for _, _, g in sims], device=False, threads=8)
    before = after = 0
    for (insert, _, (seqs, _, ref)), res in zip(sims, results):
        assert res[0] == 0
        sub = seqs[ref].decode()
        target = ccs_ref.revcomp(insert) if ref % 2 else insert   # odd passes read the other strand
        before += ccs_ref.edit_distance(sub, target)
        after += ccs_ref.edit_distance(res[1].decode(), target)
    print(f"edit distance to the inserts: reference subreads {before}, consensus {after}")
    assert after < before


# ---------------------------------------------------------------------------- interfaces
def _fastq(recs):
    return "".join(f"@{i} movie=1\n{s}\n+\n{q}\n" for i, s, q in recs).encode()


def test_cli_writes_ccseqs_records_and_summary(monkeypatch):
    rng = random.Random(4)
    _, z1 = ccs_ref.sim_zmw(rng, "m1", 1, 200, 4)
    _, z2 = ccs_ref.sim_zmw(rng, "m1", 2, 150, 1, partial=False)
    _, z3 = ccs_ref.sim_zmw(rng, "m1", 3, 150, 2)
    _, z4 = ccs_ref.sim_zmw(rng, "m1", 4, 150, 1, partial=False)
    recs = z1 + z2 + z3 + z4
    monkeypatch.setattr("sys.stdin", io.TextIOWrapper(io.BytesIO(_fastq(recs))))
    out, err = io.BytesIO(), io.StringIO()
    assert ccseq.main(["--host", "--threads", "2", "--pre", "x", "--chunk_seqs", "7", "--bwa-path", "/nowhere"], out, err) == 0
    lines = out.getvalue().decode().split("\n")
    heads = [ln for ln in lines if ln.startswith("@m1/")]
    ref3 = z3[0][0] if len(z3[0][1]) > len(z3[1][1]) else z3[1][0]
    assert heads == [f"@{z1[1][0]} CCS:primary", f"@{z2[0][0]} movie=1", f"@{ref3} CCS:primary"]   # the lone last record is lost
    k = lines.index(heads[1])
    assert lines[k + 1:k + 4] == [z2[0][1], "+", z2[0][2]]   # a single passes unchanged
    log = err.getvalue()
    assert "Reading STDIN" in log
    assert re.search(r"\[ccseq\] Processed 8 subreads from 3 reads\n", log)
    assert re.search(r"\[ccseq\]   2 consensus \+ 1 bypassed single subreads\n", log)
    results, _, _ = ccseq.run_groups([([r[1].encode() for r in z1], [r[2].encode() for r in z1], 1)], device=False)
    assert lines[1] == results[0][1].decode() and lines[3] == results[0][2].decode()


def test_cli_exits_255_on_a_foreign_id(monkeypatch, tmp_path):
    f = tmp_path / "in.fq"
    f.write_bytes(_fastq([("m1/1/0_60", "A" * 60, "5" * 60), ("read_2", "A" * 60, "5" * 60)]))
    out, err = io.BytesIO(), io.StringIO()
    assert ccseq.main(["--host", "--reads", str(f)], out, err) == 255
    assert out.getvalue() == b"" and "Not a valid PacBio subread id: read_2" in err.getvalue()


def test_modes_with_ccs():
    assert T.MODE_TASKS["sr"] == ("read-long", "ccs-1") + T.MODE_TASKS["sr-noccs"][1:]
    assert T.MODE_TASKS["mr"] == ("read-long", "ccs-1") + T.MODE_TASKS["mr-noccs"][1:]
    assert T.noccs_mode("sr") == "sr-noccs" and T.noccs_mode("mr") == "mr-noccs"
    assert T.mode_for(100) == "sr-noccs" and T.hcr_mask("ccs-1") == "20,41,80,130,60,0.7"
    from proovread_amd import correct
    assert correct.subread_ids(["m1/1/0_9", "m2/7/3_4 x"]) and not correct.subread_ids(["m1/1/0_9", "r2"])
    assert correct.parse_args(["-l", "a", "-s", "b", "-p", "c", "-m", "sr"]).mode == "sr"
    assert correct.LoopConfig().mode is None

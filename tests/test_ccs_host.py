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


# ---------------------------------------------------------------------------- mapping: built cases
# Each case is checked twice from the restatement alone: that it reaches the edge it was built
# for, and that the host path returns what the restatement returns.  tests/test_ccs_gpu.py runs
# the same cases on the device.
def _host_maps(case):
    (ga,) = ccseq.map_groups([ccs_cases.pair_group(case)], ccseq.default_params(**case.over), device=False, threads=1)
    assert ga[0] is None
    assert ga[1] == ccs_cases.map_expected(case)
    return ga[1]


def _centre(case):
    p = ccs_cases.ref_params(case)
    return ccs_ref.centre(case.ref, case.query, p["k"], p["w"])


def _best_cells(case):
    """The number of band cells that hold the best score."""
    rev, d0 = _centre(case)
    stats = {}
    ccs_ref.align(case.ref, ccs_ref.revcomp(case.query) if rev else case.query, d0, ccs_cases.ref_params(case), stats)
    return stats["n_best"]


def test_the_case_lists_name_every_case():
    assert list(ccs_cases.band_cases()) == ccs_cases.BAND_NAMES
    assert list(ccs_cases.band_edge_cases()) == ccs_cases.EDGE_NAMES
    assert list(ccs_cases.overhang_cases()) == ccs_cases.OVERHANG_NAMES
    assert list(ccs_cases.tie_cases()) == ccs_cases.TIE_NAMES
    assert list(ccs_cases.tandem_cases()) == ccs_cases.TANDEM_NAMES
    assert list(ccs_cases.seed_cases()) == ccs_cases.SEED_NAMES
    assert list(ccs_cases.hand_cases()) == ccs_cases.HAND_NAMES


@pytest.mark.parametrize("name", ccs_cases.BAND_NAMES)
def test_band_gap_crosses_two_runs_of_the_scan(name):
    """One gap of the full length between the flanks, at least two lanes' runs of cells long."""
    case = ccs_cases.band_cases()[name]
    w, n, op, strand = ccs_cases.band_shape(name)
    assert case.over == {"w": w} and n >= 2 * ccs_cases.cells_per_lane(w) and n <= w
    want = ccs_cases.map_expected(case)
    assert want is not None and want[0] == strand
    gaps = [int(x) for x, o in re.findall(r"(\d+)([MIDS])", want[3]) if o == op]
    assert gaps == [n], want
    _host_maps(case)


@pytest.mark.parametrize("name", ccs_cases.EDGE_NAMES)
def test_band_gap_opens_on_the_edge_of_the_band(name):
    """The flank before the gap lies w diagonals from the centre: the insertion opens in the
    band's first cell (lane 0's carry reaches the centre's lane), the deletion in its last."""
    case = ccs_cases.band_edge_cases()[name]
    w, kind = case.over["w"], name[name.index("_") + 1:]
    rev, d0 = _centre(case)
    want = ccs_cases.map_expected(case)
    assert want is not None and want[0] == rev == int(kind == "rev")
    gaps = [int(x) for x, o in re.findall(r"(\d+)([MIDS])", want[3]) if o == ("D" if kind == "del" else "I")]
    assert gaps == [w] and w >= 2 * ccs_cases.cells_per_lane(w), want
    # the flank before the gap starts at reference base 30 and query base 0: diagonal 30
    assert want[1] == 30 and (30 - d0 == -w if kind == "del" else 30 - d0 == w)
    _host_maps(case)


def test_cells_per_lane_changes_where_the_bands_are():
    assert [ccs_cases.cells_per_lane(w) for w in (8, 31, 32, 63, 64, 300, 512)] == [1, 1, 2, 2, 3, 10, 17]
    assert 2 * 31 + 2 == 64   # w = 31: lane 63 holds the cell right of the band


@pytest.mark.parametrize("name", ccs_cases.OVERHANG_NAMES)
def test_band_overhangs_the_reference(name):
    case = ccs_cases.overhang_cases()[name]
    want = ccs_cases.map_expected(case)
    rev, d0 = _centre(case)
    w, lr, lq = case.over["w"], len(case.ref), len(case.query)
    assert rev == 0 and want[0] == 0
    if name.endswith("_end"):
        assert d0 == lr - 60 > 0 and re.search(r"M40S$", want[3]) and not re.match(r"\d+S", want[3])
        assert d0 - w > 0   # the rows start inside the reference, left of the query
        assert (lr - 1) - d0 + w >= lq or w == 31   # at w = 64 the last row's band passes the query's end
    else:
        assert d0 == -40 < 0 and re.match(r"40S\d+M", want[3]) and not want[3].endswith("S")
        assert -d0 - w < 0 or w == 31   # at w = 64 the first row's band starts left of the query
        assert lq - 1 + d0 + w < lr - 1   # the band leaves the query before the reference ends
    _host_maps(case)


@pytest.mark.parametrize("name", ccs_cases.TIE_NAMES)
def test_tie_scores(name):
    """a = b = e = 1, o = 0: the best score is held by several cells, so the first in (i, j)
    order has to be found, and M >= E >= F decides many cells."""
    case = ccs_cases.tie_cases()[name]
    assert len(case.ref) == len(case.query) == 150 and case.over == ccs_cases.TIE_SCORES
    assert ccs_cases.map_expected(case) is not None
    got = _host_maps(case)
    if name == "unrelated":
        assert _best_cells(case) >= 2
    else:
        assert "I" in got[3] and "D" in got[3] and got[2] >= 100


@pytest.mark.parametrize("name", ccs_cases.TANDEM_NAMES)
def test_tandem_repeat(name):
    case = ccs_cases.tandem_cases()[name]
    want = ccs_cases.map_expected(case)
    assert want == (0, 20, 750, "150M")
    # the same score one unit on: the first of several maximal cells wins
    assert ccs_ref.map_ref(case.ref[50:], case.query, ccs_cases.ref_params(case))[2] == 750
    if name == "w300":
        assert _best_cells(case) >= 2   # all of them inside the band
    if name == "w8":   # the bucket tie: equal pair sums several buckets apart
        sums = ccs_cases.pair_sums(case)
        top = sorted(k for k, v in sums.items() if v == max(sums.values()))
        assert len(top) >= 2 and top[-1][1] - top[0][1] >= 2 and top[0][0] == 0
    _host_maps(case)


@pytest.mark.parametrize("name", ccs_cases.SEED_NAMES)
def test_seed_cases(name):
    case = ccs_cases.seed_cases()[name]
    want = ccs_cases.map_expected(case)
    fwd, rev = ccs_cases.both_seeds(case)
    sums = ccs_cases.pair_sums(case)
    w, lr, lq = ccs_cases.ref_params(case)["w"], len(case.ref), len(case.query)
    if name.startswith("orient_tie"):
        assert case.query == ccs_ref.revcomp(case.query)
        best = max(sums.values())
        assert {o for (o, _), v in sums.items() if v == best} == {0, 1}   # both orientations hold the maximum
        assert want[0] == 0 and want[3] == "120M"
        if name == "orient_tie_w1":
            nb = ccs_cases.n_buckets(case)
            assert 2 * nb > 512   # a thread of the 256 sees candidates of both orientations
    elif name.startswith("key_tie"):
        assert not rev and sorted(s[2] for s in fwd) == [9, 9, 12, 12, 12]
        top = [s for s in fwd if s[2] == 12]
        assert len({ccs_cases.dshift(case, s) // w for s in top}) == 1   # one bucket
        assert len({s[0] - s[1] for s in top}) == 3                      # three diagonals
        assert (len({s[0] for s in top}) == 3) == (name == "key_tie_i")  # decided by i, or by the diagonal alone
        win = min(top, key=lambda s: (s[0], s[0] - s[1]))
        assert _centre(case) == (0, win[0] - win[1])
        p = ccs_cases.ref_params(case)
        right = ccs_ref.align(case.ref, case.query, win[0] - win[1], p)
        assert right == want[1:] and 60 <= right[1] < 118
        for s in top:   # a band around either loser finds the beads: the choice shows in the result
            if s != win:
                assert ccs_ref.align(case.ref, case.query, s[0] - s[1], p)[1] >= 118
    elif name == "one_9mer":
        assert [s[2] for s in fwd + rev] == [9] and want is not None and want[0] == 0 and want[2] >= 45
    elif name == "one_8mer":
        assert fwd + rev == [] and want is None
        assert case.ref[40:48] in case.query   # the 8-mer is there
    elif name.startswith("diag_"):
        assert lr + lq - 1 == int(name[5:]) and want is not None
        assert want[0] == (name == "diag_256")
    elif name.startswith("cand_"):
        assert w == 1 and 2 * ccs_cases.n_buckets(case) == int(name[5:]) and want is not None
        assert want[0] == (name != "cand_254") and want[3] == f"{lq}M"
    else:
        assert not rev and [s[2] for s in fwd] == [10, 9] and len({s[0] - s[1] for s in fwd}) == 1
        assert ("N" in case.ref) == (name == "n_in_ref") and ("N" in case.query) == (name == "n_in_query")
        assert want is not None and want[0] == 0 and want[2] >= 19 * 5 - 1
    _host_maps(case)


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
                                  "del_quals", "ref_alone", "rev_ins_wins"])
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
    # the reverse-strand subread's insertion: GT wins column 40, and its first carrier is the first alignment
    ref, rq, alns = hand["rev_ins_wins"]
    assert [a[4:] for a in alns] == [(1,), (), ()] and all(60 <= len(a[0]) <= 80 for a in alns)
    o = _oracle(ccs_cases.to_case("rev_ins_wins", ref, rq, alns))
    assert o["fastq"].split("\n")[1] == ref[:41] + "GT" + ref[41:]
    assert _oracle(ccs_cases.to_case("rev_ins_wins", ref, rq, alns[1:]))["fastq"].split("\n")[1] == ref[:41] + "CC" + ref[41:]


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


@pytest.mark.parametrize("bad", ccs_cases.BAD_ALNS)
def test_a_malformed_alignment_between_healthy_groups(hand, bad):
    """The flagged group is empty; its neighbours in the batch are what they are alone."""
    groups, alns, over_slot = ccs_cases.malformed_batch(hand, bad)
    res = ccs_cases.consensus_raw(groups, alns, over_slot, device=False)
    assert res[1] == (ccseq.BAD_ALN, b"", b"", b"")
    for k in (0, 2):
        assert res[k][0] == 0 and len(res[k][1]) > 100
        assert [res[k]] == ccseq.consensus_groups([groups[k]], [alns[k]], device=False)
    if bad == "over_slot":   # the count alone is wrong: the same alignment is healthy
        assert ccs_cases.consensus_raw(groups, alns, (), device=False)[1][0] == 0


@pytest.mark.parametrize("name", list(ccs_cases.TILES))
def test_tile_boundary_cases(name):
    """From the oracle: the gap and the three-base state stand in exactly the columns built,
    so the sequence and the trace both differ in length from the reference."""
    L, dels, inss = ccs_cases.TILES[name]
    _, o = _check_case(name, *ccs_cases.tile_case(name))
    assert o["trace"] == ccs_cases.tile_trace(name)
    cols, at = [], 0   # the trace by column
    for c in range(L):
        n = 3 if c in inss else 1
        cols.append(o["trace"][at:at + n])
        at += n
    assert all(cols[c] == "I" for c in dels) and all(cols[c] == "MDD" for c in inss)
    assert [c for c in range(L) if cols[c] != "M"] == sorted(dels + inss)
    assert len(o["fastq"].split("\n")[1]) == L - len(dels) + 2 * len(inss) != L
    assert len(o["trace"]) == L + 2 * len(inss) != L
    assert L <= 256 or any(c % 256 in (255, 0) for c in dels + inss)   # a choice on a tile's edge


def test_tile_cases_cover_the_lengths():
    assert {t[0] for t in ccs_cases.TILES.values()} >= {255, 256, 257, 512, 513}
    assert (260, (255,), (256,)) in ccs_cases.TILES.values() and (516, (511,), (512,)) in ccs_cases.TILES.values()


def test_more_cigar_ops_than_a_block_has_threads():
    ref, rq, alns = ccs_cases.many_ops_case()
    s, _, _, cig = alns[0]
    assert len(re.findall(r"\d+[MID]", cig)) == 601
    assert ccs_cases.kept_ops(cig, len(s)) == 601 > 256   # the taboo is one base: the 2M and the 20M at the ends stay
    assert ccs_cases.kept_ops("299S350M1D349M1I1M", 1000) == 3   # skip_384's tail: the 1I1M goes
    _, o = _check_case("many_ops", ref, rq, alns)
    assert o["trace"].count("I") == 150 and o["trace"].count("D") == 150   # its gaps and insertions win their columns


def test_full_house_of_300_base_subreads():
    ids, grp = ccs_cases.full_house()
    assert len(grp[0]) == ccseq.MAX_SUBREADS and all(len(s) == 300 for s in grp[0])
    results, alns, _ = ccseq.run_groups([grp], device=False, threads=4)
    assert sum(a is not None for a in alns[0]) == ccseq.MAX_SUBREADS - 1
    o = _oracle(ccs_cases.zmw_case(ids, grp, alns[0]))
    assert o["kept"] == "1" * (ccseq.MAX_SUBREADS - 1)   # every alignment is used
    assert results[0][0] == 0 and _host_fastq(ids[grp[2]], results[0]) == o["fastq"] and results[0][3].decode() == o["trace"]


# ---------------------------------------------------------------------------- chunks
def test_chunk_batch_passes_one_launch():
    """More groups, and more pairs, than one launch takes, and the groups around 65,535 differ."""
    groups = ccs_cases.chunk_groups()
    assert len(groups) == 65540 > 65535 and sum(len(g[0]) - 1 for g in groups) > 65535
    assert all(len(s) == 60 for s in groups[65534][0]) and 60 > ccseq.default_params().min_aln_length
    results, alns = ccs_cases.chunk_host()
    edge = results[65533:65540]
    assert len({r[1] for r in edge}) == 7 and all(r[0] == 0 and len(r[1]) >= 59 for r in edge)
    assert all(ga[1] is None and ga[0] is not None and ga[0][0] == int(g % 3 == 2) for g, ga in enumerate(alns))
    assert all(r[0] == 0 and r[1] for r in results)


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

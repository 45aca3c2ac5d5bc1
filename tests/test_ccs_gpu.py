"""ccs-1 on the device equals the host path: status, alignments and consensus bytes of every
group, at both bands, at each capacity and just beyond it.

The built cases of tests/ccs_cases.py run on the device against the references the host tests
use (tests/test_ccs_host.py asserts there, without a device, that each case reaches its edge):
the mapping against the plain-Python restatement ccs_ref.map_ref, the consensus against the C
oracle of Sam::Seq and the Perl records, byte for byte.  The chunk loops of the device path go
round twice on more than 65,535 pairs and groups; their 1 GiB budgets (direction bytes per
align launch, column entries per consensus launch) need about 64 pairs of 16,384 bases at
w = 512, some 10^9 cells on the host reference, and are left out."""
import random
import time
from pathlib import Path

import pytest

import casefmt
import ccs_cases
import ccs_ref
import oracle_bind
from proovread_amd import _abi, ccseq

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"


def _group(recs):
    ids = [r[0] for r in recs]
    role, _, ng = ccseq.group(ids, [len(r[1]) for r in recs])
    assert ng == 1
    return [r[1].encode() for r in recs], [r[2].encode() for r in recs], list(role).index(ccseq.PRIMARY)


def _zmws(seed, n, lo=200, hi=700, passes=(2, 8)):
    rng = random.Random(seed)
    return [_group(ccs_ref.sim_zmw(rng, "m150101_1_s1_p0", z, rng.randrange(lo, hi + 1), rng.randrange(passes[0], passes[1] + 1))[1])
            for z in range(n)]


@pytest.fixture(scope="module")
def ctx():
    return _abi.default_context()


def _same(groups, p, ctx):
    host = ccseq.run_groups(groups, p, device=False, threads=8)
    dev = ccseq.run_groups(groups, p, device=True, ctx=ctx)
    for g, (hr, ha, dr, da) in enumerate(zip(host[0], host[1], dev[0], dev[1])):
        assert ha == da, f"group {g}: alignments"
        assert hr == dr, f"group {g}: status / consensus"
    return host, dev


@pytest.mark.parametrize("w", [8, 300])
def test_device_equals_host(ctx, w):
    groups = _zmws(11 + w, 12)
    host, dev = _same(groups, ccseq.default_params(w=w), ctx)
    assert sum(a is not None for ga in host[1] for a in ga) >= 20
    assert any(a is not None and a[0] == 1 for ga in host[1] for a in ga)
    assert all(r[0] == 0 and len(r[1]) > 100 for r in host[0])
    assert dev[2] > 0.0


def test_hooks_on_the_device(ctx):
    groups = _zmws(5, 4, 200, 300)
    p = ccseq.default_params(w=8)
    alns = ccseq.map_groups(groups, p, device=True, ctx=ctx)
    assert alns == ccseq.map_groups(groups, p, device=False)
    assert ccseq.consensus_groups(groups, alns, p, device=True, ctx=ctx) == ccseq.consensus_groups(groups, alns, p, device=False)


def _exact_len(rng, n, passes):
    """A group whose subreads all have exactly n bases."""
    insert = "".join(rng.choice("ACGT") for _ in range(n + n // 4 + 200))
    recs, at = [], 0
    for k in range(passes):
        s = ccs_ref.noisy(rng, insert if k % 2 == 0 else ccs_ref.revcomp(insert), 0.02, 0.01, 0.005)
        s = s[:n] if k % 2 == 0 else s[-n:]
        assert len(s) == n
        recs.append((f"m2/{n}/{at}_{at + n}", s, "".join(chr(33 + rng.randint(5, 20)) for _ in s)))
        at += n + 40
    return _group(recs)


def test_capacities_and_the_calls_after(ctx):
    rng = random.Random(3)
    p = ccseq.default_params(w=8)
    small = _zmws(21, 3, 200, 300, (3, 4))
    at_len, over_len = _exact_len(rng, ccseq.MAX_LEN, 2), _exact_len(rng, ccseq.MAX_LEN + 1, 2)
    at_n, over_n = _exact_len(rng, 80, ccseq.MAX_SUBREADS), _exact_len(rng, 80, ccseq.MAX_SUBREADS + 1)
    groups = [small[0], at_len, over_len, small[1], at_n, over_n, small[2]]
    host, dev = _same(groups, p, ctx)
    assert [r[0] for r in dev[0]] == [0, 0, ccseq.TOO_LONG, 0, 0, ccseq.TOO_MANY, 0]
    assert dev[0][2][1] == b"" and dev[0][5][1] == b"" and all(a is None for a in dev[1][2] + dev[1][5])
    assert dev[1][1][0] is not None and len(dev[0][1][1]) > ccseq.MAX_LEN // 2
    assert sum(a is not None for a in dev[1][4]) == ccseq.MAX_SUBREADS - 1
    _same(small, p, ctx)   # the next call on the context


# ---------------------------------------------------------------------------- mapping: built cases
def _device_maps(case, ctx):
    (ga,) = ccseq.map_groups([ccs_cases.pair_group(case)], ccseq.default_params(**case.over), device=True, ctx=ctx)
    assert ga[0] is None
    assert ga[1] == ccs_cases.map_expected(case)


@pytest.mark.parametrize("name", ccs_cases.BAND_NAMES)
def test_band_gap_crosses_two_runs_of_the_scan(ctx, name):
    """A gap of at least two lanes' runs of cells: the carries meet across whole runs."""
    _device_maps(ccs_cases.band_cases()[name], ctx)


@pytest.mark.parametrize("name", ccs_cases.EDGE_NAMES)
def test_band_gap_opens_on_the_edge_of_the_band(ctx, name):
    """The insertion opens in the band's first cell, so lane 0's carry decides every run up
    to the centre; the deletion is entered from the band's last cell."""
    _device_maps(ccs_cases.band_edge_cases()[name], ctx)


@pytest.mark.parametrize("name", ccs_cases.OVERHANG_NAMES)
def test_band_overhangs_the_reference(ctx, name):
    _device_maps(ccs_cases.overhang_cases()[name], ctx)


@pytest.mark.parametrize("name", ccs_cases.TIE_NAMES)
def test_tie_scores(ctx, name):
    _device_maps(ccs_cases.tie_cases()[name], ctx)


@pytest.mark.parametrize("name", ccs_cases.TANDEM_NAMES)
def test_tandem_repeat(ctx, name):
    """Several maximal cells (w = 300) and equal pair sums buckets apart (w = 8)."""
    _device_maps(ccs_cases.tandem_cases()[name], ctx)


@pytest.mark.parametrize("name", ccs_cases.SEED_NAMES)
def test_seed_cases(ctx, name):
    _device_maps(ccs_cases.seed_cases()[name], ctx)


def test_mapping_cases_in_one_batch(ctx):
    """Every case of the default scores at w = 8 as one group each: pairs of different lengths,
    mapped and unmapped, share the launches."""
    cases = [c for c in list(ccs_cases.seed_cases().values()) + list(ccs_cases.tandem_cases().values()) if c.over == {"w": 8}]
    assert len(cases) >= 10
    got = ccseq.map_groups([ccs_cases.pair_group(c) for c in cases], ccseq.default_params(w=8), device=True, ctx=ctx)
    assert [ga[1] for ga in got] == [ccs_cases.map_expected(c) for c in cases]
    assert any(ga[1] is None for ga in got)


# ---------------------------------------------------------------------------- consensus: built cases
def _oracle(case, **over):
    o = oracle_bind.run_case(case, **dict(ccs_cases.ORACLE_OVER, **over))
    assert o["rc"] == 0, o
    return o


def _equals_oracle(case, res, o):
    assert res[0] == 0, case.name
    assert f"@{case.ref_id}\n{res[1].decode()}\n+\n{res[2].decode('latin-1')}\n" == o["fastq"], case.name
    assert res[3].decode() == o["trace"], case.name


def _device_case(ctx, name, ref, rq, alns, **pover):
    case = ccs_cases.to_case(name, ref, rq, alns)
    grp, ga = ccs_cases.to_group(ref, rq, alns)
    (res,) = ccseq.consensus_groups([grp], [ga], ccseq.default_params(**pover), device=True, ctx=ctx)
    o = _oracle(case, **pover)
    _equals_oracle(case, res, o)
    return o


@pytest.fixture(scope="module")
def hand():
    return ccs_cases.hand_cases()


@pytest.mark.parametrize("name,trim", [(n, 1) for n in ccs_cases.HAND_NAMES] + [("leading_ins", 0), ("del_quals", 0)])
def test_hand_cases_equal_the_oracle(ctx, hand, name, trim):
    _device_case(ctx, name, *hand[name], **({} if trim else {"trim": 0}))


def _built_cases(hand):
    named = [(n, hand[n]) for n in ccs_cases.HAND_NAMES] + [(n, ccs_cases.tile_case(n)) for n in ccs_cases.TILES]
    return named + [("many_ops", ccs_cases.many_ops_case())]


def test_built_cases_in_one_batch(ctx, hand):
    """Groups of different lengths and numbers of alignments share a launch."""
    named = _built_cases(hand)
    packed = [ccs_cases.to_group(*c) for _, c in named]
    assert len({len(c[0]) for _, c in named}) >= 8 and {len(c[2]) for _, c in named} >= {1, 2, 3}
    res = ccseq.consensus_groups([g for g, _ in packed], [ga for _, ga in packed], device=True, ctx=ctx)
    for (name, c), r in zip(named, res):
        case = ccs_cases.to_case(name, *c)
        _equals_oracle(case, r, _oracle(case))


PERL_CASES = casefmt.read_cases(GOLDEN / "ccs_cases.txt")


@pytest.fixture(scope="module")
def perl_expect():
    return casefmt.read_expect(GOLDEN / "ccs_expected.txt")


def _equals_perl(case, res, e):
    assert not e.error and res[0] == 0, case.name
    assert [f"@{case.ref_id} CCS:primary", res[1].decode(), "+", res[2].decode("latin-1")] == e.fastq, case.name
    assert res[3].decode() == e.trace, case.name


@pytest.mark.parametrize("case", PERL_CASES, ids=[c.name for c in PERL_CASES])
def test_device_consensus_equals_the_perl_records(ctx, perl_expect, case):
    grp, ga = ccs_cases.to_group(case.ref[1], case.ref[3], ccs_cases.case_alns(case))
    (res,) = ccseq.consensus_groups([grp], [ga], device=True, ctx=ctx)
    _equals_perl(case, res, perl_expect[case.name])


def test_perl_records_in_one_batch(ctx, perl_expect):
    assert len(PERL_CASES) >= 10
    packed = [ccs_cases.to_group(c.ref[1], c.ref[3], ccs_cases.case_alns(c)) for c in PERL_CASES]
    res = ccseq.consensus_groups([g for g, _ in packed], [ga for _, ga in packed], device=True, ctx=ctx)
    for case, r in zip(PERL_CASES, res):
        _equals_perl(case, r, perl_expect[case.name])


@pytest.mark.parametrize("bad", ccs_cases.BAD_ALNS)
def test_a_malformed_alignment_between_healthy_groups(ctx, hand, bad):
    """The block of the flagged group returns early; its neighbours are what they are alone
    (test_hand_cases_equal_the_oracle holds them against the oracle)."""
    groups, alns, over_slot = ccs_cases.malformed_batch(hand, bad)
    res = ccs_cases.consensus_raw(groups, alns, over_slot, device=True, ctx=ctx)
    assert res[1] == (ccseq.BAD_ALN, b"", b"", b"")
    for k in (0, 2):
        assert res[k][0] == 0 and len(res[k][1]) > 100
        assert [res[k]] == ccseq.consensus_groups([groups[k]], [alns[k]], device=True, ctx=ctx)
    assert res == ccs_cases.consensus_raw(groups, alns, over_slot, device=False)


@pytest.mark.parametrize("name", list(ccs_cases.TILES))
def test_tile_boundary_cases(ctx, name):
    """A gap and a three-base state on the edges of the kernel's tiles of 256 columns."""
    o = _device_case(ctx, name, *ccs_cases.tile_case(name))
    assert o["trace"] == ccs_cases.tile_trace(name)


def test_more_cigar_ops_than_a_block_has_threads(ctx):
    _device_case(ctx, "many_ops", *ccs_cases.many_ops_case())


def test_full_house_of_300_base_subreads(ctx):
    ids, grp = ccs_cases.full_house()
    host, dev = _same([grp], ccseq.default_params(), ctx)
    assert sum(a is not None for a in dev[1][0]) == ccseq.MAX_SUBREADS - 1
    case = ccs_cases.zmw_case(ids, grp, dev[1][0])
    o = _oracle(case)
    assert o["kept"] == "1" * (ccseq.MAX_SUBREADS - 1)
    _equals_oracle(case, dev[0][0], o)


# ---------------------------------------------------------------------------- chunks
def test_chunk_loops_go_round_twice(ctx):
    """65,540 groups of one pair each: the align launches and the consensus launches both take
    a second chunk.  The host path alone is the reference here: the plain-Python restatement
    would need minutes for 65,540 pairs (tests/test_ccs_host.py holds the host path against it
    on every other case)."""
    groups = ccs_cases.chunk_groups()
    t0 = time.perf_counter()
    host = ccs_cases.chunk_host()
    t1 = time.perf_counter()
    dev = ccseq.run_groups(groups, ccseq.default_params(w=8), device=True, ctx=ctx)
    t2 = time.perf_counter()
    print(f"chunk batch: host path {t1 - t0:.2f} s (0 if an earlier test ran it), device path {t2 - t1:.2f} s, kernels {dev[2]:.1f} ms")
    assert len(dev[0]) == len(dev[1]) == len(groups) == 65540
    bad = [g for g in range(len(groups)) if dev[1][g] != host[1][g] or dev[0][g] != host[0][g]]
    assert not bad, (len(bad), bad[:5])
    edge = dev[0][65533:65540]
    assert len({r[1] for r in edge}) == 7 and all(r[0] == 0 and len(r[1]) >= 59 for r in edge)
    assert all(ga[0] is not None for ga in dev[1][65533:65540])

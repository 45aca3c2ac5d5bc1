"""The unitig consensus (bam2cns --utg-mode) on the device equals the host path: status, kept
flags, overlap windows, sequence, quality and trace of every read -- on the golden cases, on
seeded random reads, at the tile and block edges of the scans, at the wave and block edges of
the contained filter, beyond its on-chip path, at each capacity and just beyond it."""
import random

import pytest

import utg_cases
from proovread_amd import _abi, bam2cns, cns, utgcns

pytestmark = pytest.mark.gpu

CASES = utg_cases.read_cases()
EXPECTED = utg_cases.read_expected()
FULL = dict(qual_weighted=True, fallback_phred=30, rep_coverage=7, min_ncscore=3.3)
PARAM_SETS = [utgcns.UtgParams(**FULL), utgcns.UtgParams(**FULL, invert_scores=True, max_ins_length=2),
              utgcns.UtgParams(qual_weighted=True, trim=0), utgcns.UtgParams(rep_coverage=2, use_ref_qual=False, indel_taboo_length=0,
                                                                              indel_taboo=0.05)]


@pytest.fixture(scope="module")
def ctx():
    return _abi.default_context()


def as_tuple(res):
    return res.status, res.seq, res.qual, res.trace, [bool(k) for k in res.kept], list(res.windows)


def same(reads, alns, p, ctx):
    host = utgcns.run(reads, alns, p, device=False, threads=8)
    dev = utgcns.run(reads, alns, p, device=True, ctx=ctx)
    for k, (h, d) in enumerate(zip(host, dev)):
        assert as_tuple(d) == as_tuple(h), f"read {k} ({reads[k].id})"
    return host


def synthetic(rng, name, L, n, spans=(55, 70), score=(200, 400), stack=None, qual=True):
    """A read of L columns with n alignments of a span drawn from `spans`, around `stack` if given."""
    ref = utg_cases.rand_seq(rng, L)
    read = cns.LongRead(name, ref, utg_cases.rand_qual(rng, L, 0, 40) if qual else None, "")
    lines = []
    for i in range(n):
        span = min(L, rng.randrange(spans[0], spans[1] + 1))
        start = rng.randrange(0, L - span + 1) if stack is None else max(0, min(L - span, stack + rng.randrange(-30, 31)))
        ops = utg_cases.noisy_ops(rng, span, rng.choice([0.0, 0.02]))
        lines.append(utg_cases.sam_line(rng, f"u{i}", name, ref, start, ops, rng.randrange(*score) * span // 60,
                                        mism=0.05, qual="*" if i % 3 == 0 else None))
    return read, [cns.SamRecord.from_line(s) for s in lines]


def test_golden_cases(ctx):
    """Each case with its own options against the reference's record; then all of them in one
    launch under each option set against the host path."""
    for c in CASES:
        read, alns, p = utg_cases.to_inputs(c)
        (res,) = utgcns.run([read], [alns], p, device=True, ctx=ctx)
        e = EXPECTED[c.name]
        if e.error:
            assert res.status == utgcns.BAD_ALN and res.seq == ""
        else:
            kept = [s.split("\t")[0] for s, k in zip(c.sam, res.kept) if k]
            assert (res.status, res.fastq, res.trace, kept, res.windows) == (0, e.fastq, e.trace, e.kept, e.windows), c.name
    ins = [utg_cases.to_inputs(c) for c in CASES if not c.fasta]
    for p in PARAM_SETS:
        host = same([i[0] for i in ins], [i[1] for i in ins], p, ctx)
        # with inverted scores step 1 drops the malformed hit before any pass parses its CIGAR
        assert [r.id for r in host if r.status] == ([] if p.invert_scores else ["lr_bad_cigar_eq"])


@pytest.mark.parametrize("k", range(len(PARAM_SETS)))
def test_random_reads_in_one_launch(ctx, k):
    ins = [utg_cases.to_inputs(c) for c in utg_cases.random_cases(7, 300)]
    for fasta in (False, True):
        sel = [i for i in ins if (i[0].qual is None) == fasta]
        host = same([i[0] for i in sel], [i[1] for i in sel], PARAM_SETS[k], ctx)
        assert len(sel) > 20 and any(r.windows for r in host) == (PARAM_SETS[k].rep_coverage is not None)


def test_random_reads_with_their_own_options(ctx):
    for c in utg_cases.random_cases(11, 40):
        read, alns, p = utg_cases.to_inputs(c)
        same([read], [alns], p, ctx)


def test_scan_tile_and_block_edges(ctx):
    rng = random.Random(21)
    reads, alns = [], []
    for L in (255, 256, 257, 1023, 1025, 512, 51, 1):
        r, a = synthetic(rng, f"len{L}", L, 12 if L > 60 else 1, spans=(51, min(max(L, 51), 200)), stack=L // 2)
        if L < 51:
            a = []
        reads.append(r), alns.append(a)
    for p in PARAM_SETS[:2] + [utgcns.UtgParams(rep_coverage=0), utgcns.UtgParams(rep_coverage=3, qual_weighted=True)]:
        same(reads, alns, p, ctx)
    # a run of high coverage that reaches the last column of a read of exactly one tile
    r = cns.LongRead("tail", reads[1].seq, reads[1].qual, "")
    a = [cns.SamRecord.from_line(utg_cases.sam_line(rng, f"t{i}", "tail", r.seq, 256 - 60 - i, [(60 + i, "M")], 300)) for i in range(4)]
    host = same([r], [a], utgcns.UtgParams(rep_coverage=3), ctx)
    assert host[0].windows and sum(host[0].windows[-1]) == 256


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_alignment_count_edges(ctx, n):
    rng = random.Random(n)
    r1, a1 = synthetic(rng, f"n{n}", 900, n, spans=(52, 140))
    r2, a2 = synthetic(rng, f"n{n}s", 700, n, spans=(52, 90), stack=350)
    for p in (utgcns.UtgParams(qual_weighted=True), utgcns.UtgParams(**FULL), utgcns.UtgParams(rep_coverage=40, qual_weighted=True)):
        host = same([r1, r2], [a1, a2], p, ctx)
    assert any(0 < r.kept.sum() < n for r in host)


def test_filter_beyond_its_on_chip_path_and_at_the_limit(ctx):
    rng = random.Random(33)
    r1, a1 = synthetic(rng, "hbm", 3000, 2100, spans=(52, 64))
    r2, a2 = synthetic(rng, "max_alns", 600, utgcns.MAX_ALNS, spans=(60, 60))
    r3, a3 = synthetic(rng, "small", 400, 5, spans=(60, 200))
    p = utgcns.UtgParams(qual_weighted=True, rep_coverage=3000, fallback_phred=30)   # no window: the filter sees every hit
    host = same([r1, r2, r3], [a1, a2, a3], p, ctx)
    assert [r.status for r in host] == [0, 0, 0] and 0 < host[0].kept.sum() < 2100 and 0 < host[1].kept.sum() < utgcns.MAX_ALNS
    same([r2, r3], [a2, a3], utgcns.UtgParams(**FULL), ctx)


def test_longest_read_and_beyond_the_limits_in_one_launch(ctx):
    rng = random.Random(44)
    L = utgcns.MAX_LEN
    ref = utg_cases.rand_seq(rng, L)
    longest = cns.LongRead("longest", ref, utg_cases.rand_qual(rng, L, 0, 40), "")
    la = [cns.SamRecord.from_line(utg_cases.sam_line(rng, n, "longest", ref, st, utg_cases.noisy_ops(rng, sp, 0.01), 5 * sp))
          for n, st, sp in (("a", 0, 150000), ("b", 120000, L - 120000))]
    too_long = cns.LongRead("too_long", ref + "A", longest.qual + "5", "")
    small, sa = synthetic(rng, "small", 500, 9, spans=(60, 300))
    many, ma = synthetic(rng, "too_many", 300, utgcns.MAX_ALNS + 1, spans=(60, 60))
    p = utgcns.UtgParams(**FULL)
    host = same([small, too_long, longest, many, small], [sa, la, la, ma, sa], p, ctx)
    assert [r.status for r in host] == [0, utgcns.TOO_LONG, 0, utgcns.TOO_MANY, 0]
    assert len(host[2].seq) > 260000 and host[2].kept.all() and as_tuple(host[0]) == as_tuple(host[4])
    # a second call on the same context
    again = utgcns.run([small], [sa], p, device=True, ctx=ctx)
    assert as_tuple(again[0]) == as_tuple(host[0])
    grp = _abi.mem_stats()["groups"].get("utg")     # the call's buffers go through the context's accounting and are gone
    assert grp is None or (grp["cur"] == 0 and grp["peak"] > 0)


@pytest.mark.parametrize("bam", [False, True], ids=["sam", "bam"])
def test_cli_on_the_device_writes_the_golden_records(tmp_path, bam):
    for c in CASES:
        argv = utg_cases.write_files(c, tmp_path, bam=bam) + ["--prefix", str(tmp_path / c.name)]
        e = EXPECTED[c.name]
        try:
            rc = bam2cns.main(argv)
        except SystemExit as x:
            rc = x.code
        assert rc == (255 if e.error else 0), c.name
        if not e.error:
            assert (tmp_path / (c.name + ".fq")).read_text() == e.fastq, c.name
            assert (tmp_path / (c.name + ".debug.trace")).read_text() == e.fastq + e.trace + "\n", c.name

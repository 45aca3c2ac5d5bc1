"""The device BAM decoder (bam_kernels.hip) against the host decoder pr_bam_decode_alns, field by
field, and cns.run_bam (records decoded and grouped per long read on the device, then the
consensus) against the Perl engine's golden vectors -- the bar of test_cns_gpu._check."""
import ctypes as C
import io
from pathlib import Path

import numpy as np
import pytest

import bam_cases
import bamio as test_bamio
import casefmt
from cns_case_util import case_inputs, params_key
from proovread_amd.bam2cns import _BamAlns

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
CASES = casefmt.read_cases(GOLD / "cns_cases.txt")
EXPECT = casefmt.read_expect(GOLD / "cns_expected.txt")
PR_ERR_ARG, PR_ERR_SAM = -1, -3


def gpu_decode(body: bytes):
    from proovread_amd import _abi
    L = _abi.lib()
    L.pr_bam_alns_free.argtypes = [C.POINTER(_BamAlns)]
    L.pr_bam_alns_free.restype = None
    a = _BamAlns()
    rc = L.pr_bam_decode_alns_gpu(_abi.default_context().h, body, len(body), C.byref(a))
    if rc:
        return rc, None
    try:
        return 0, bam_cases.take_alns(a)
    finally:
        L.pr_bam_alns_free(C.byref(a))


def last_error() -> str:
    from proovread_amd import _abi
    return _abi.lib().pr_last_error().decode()


@pytest.fixture(scope="module")
def synthetic():
    """A small correction job mapped with the bwa-proovread drop-in: (long reads, reference
    names with one read that gets no records, the SAM records as a sorted BAM record stream)."""
    from proovread_amd import bamio, bwa_proovread, synth
    from proovread_amd import tasks as T
    import tempfile
    d = synth.simulate(5, 30000, 12, 3000, 15.0)
    with tempfile.TemporaryDirectory() as td:
        lr_fa, sr_fq = Path(td) / "lr.fa", Path(td) / "sr.fq"
        lr_fa.write_text("".join(f">lr{i}\n{d.lr_str(i)}\n" for i in range(d.n_lr)))
        sr_fq.write_text("".join(f"@sr{i}\n{d.sr_str(i)}\n+\n{'I' * len(d.sr_str(i))}\n" for i in range(d.n_sr)))
        out = io.StringIO()
        assert bwa_proovread.mem(T.bwa_argv("bwa-sr-1") + [str(lr_fa), str(sr_fq)], out=out, log=io.StringIO()) == 0
    lines = [ln for ln in out.getvalue().split("\n") if ln and not ln.startswith("@")]
    names = [f"lr{i}" for i in range(d.n_lr)]
    names.insert(5, "lr_none")   # a long read without a record, in the middle
    body = bamio._native_sort(bam_cases.encode(lines, names))
    return d, names, body


def test_decoder_equals_host_on_every_record_shape():
    body = bam_cases.encode(bam_cases.sam_lines())
    rc, want = bam_cases.host_decode(body)
    assert rc == 0 and len(want["rid"]) == len(bam_cases.LSEQS) * 8 * len(bam_cases.NCIGS)
    rc, got = gpu_decode(body)
    assert rc == 0, last_error()
    bam_cases.assert_same(got, want)


def test_decoder_equals_host_on_a_mapped_job(synthetic):
    _, names, body = synthetic
    rc, want = bam_cases.host_decode(body)
    assert rc == 0
    n = len(want["rid"])
    assert n >= 3000                                   # many waves, many workgroups of every pass
    assert 5 not in set(want["rid"].tolist()) and {4, 6} <= set(want["rid"].tolist())
    rc, got = gpu_decode(body)
    assert rc == 0, last_error()
    bam_cases.assert_same(got, want)


def test_empty_stream():
    rc, got = gpu_decode(b"")
    assert rc == 0 and len(got["rid"]) == 0 and len(got["seq"]) == 0 and len(got["cig"]) == 0


def test_malformed_aux_in_mid_stream_is_refused():
    good = bam_cases.encode(bam_cases.sam_lines()[:40])
    for bad in bam_cases.malformed_records()[::9]:
        body = good + bad + good   # never last: even an unchecked walk would stay inside the buffer
        assert bam_cases.host_decode(body)[0] == PR_ERR_SAM
        assert gpu_decode(body)[0] == PR_ERR_SAM
        assert last_error() == "bad BAM aux field"


def test_size_errors_as_the_host_decoder():
    rec = bam_cases.encode(["q1\t0\tlr0\t5\t60\t4M\t*\t0\t0\tACGT\tIIII"])
    for body, text in ((rec + rec[:3], "truncated BAM record"), (rec + rec[:-1], "bad BAM record size")):
        assert bam_cases.host_decode(body)[0] == PR_ERR_ARG and last_error() == text
        assert gpu_decode(body)[0] == PR_ERR_ARG and last_error() == text


# ---------------------------------------------------------------------------- run_bam
def _check(case, r):
    e = EXPECT[case.name]
    assert r.status == 0, (case.name, r.status)
    assert r.fastq.rstrip("\n").split("\n") == e.fastq, case.name
    assert r.trace == e.trace, case.name
    assert r.chim_lines() == e.chim, case.name
    assert "".join(str(int(x)) for x in r.kept) == e.kept, case.name


def _golden_batches():
    """The golden cases the BAM path can carry, grouped by consensus parameters, each group cut
    into batches of distinct read ids.  BAM stores 4-bit bases, so a lower-case base of the SAM
    text comes back upper-case and the consensus sees another read (test_bam2cns_cli.py): such
    cases are left to the SAM-text tests."""
    groups = {}
    for c in CASES:
        if EXPECT[c.name].error or c.p("noref") == "1" or c.p("qual_weighted") == "1":
            continue
        if any(ch.islower() for l in c.sam for ch in l.split("\t")[9]):
            continue
        lr, _, p = case_inputs(c)
        batches = groups.setdefault(params_key(p), (p, []))[1]
        for b in batches:
            if all(c.ref_id != x[0].ref_id for x in b):
                b.append((c, lr))
                break
        else:
            batches.append([(c, lr)])
    return list(groups.values())


def _write_bam(path, items):
    test_bamio.write_bam(str(path), [(c.ref_id, len(c.ref[1])) for c, _ in items], [l for c, _ in items for l in c.sam])


def test_run_bam_matches_reference_golden(tmp_path):
    from proovread_amd import cns
    n = 0
    for k, (params, batches) in enumerate(_golden_batches()):
        for j, items in enumerate(batches):
            bam = tmp_path / f"g{k}_{j}.bam"
            _write_bam(bam, items)
            res = cns.run_bam([lr for _, lr in items], str(bam), params)
            for (c, _), r in zip(items, res):
                _check(c, r)
                n += 1
    assert n > 20


def test_run_bam_read_order_ranges_and_repeated_ids(tmp_path):
    """The reads in another order than the BAM header's references (each read's records move as
    a block), in three ranges (the stream decoded once per range), with a repeated read id and
    a read the file does not know."""
    from proovread_amd import cns
    params, batches = max(_golden_batches(), key=lambda g: len(g[1][0]))
    items = batches[0]
    assert len(items) >= 3
    bam = tmp_path / "x.bam"
    _write_bam(bam, items)
    order = list(reversed(items)) + [items[1]]
    reads = [lr for _, lr in order] + [cns.LongRead("unknown_read", "ACGT" * 30, "I" * 120)]
    for split in (1, 3):
        res = cns.run_bam(reads, str(bam), params, split=split)
        assert len(res) == len(reads)
        for (c, _), r in zip(order, res):
            _check(c, r)
        assert res[-1].status == 0 and len(res[-1].kept) == 0
        assert res[-1].fastq == cns.run_chunk(reads[-1:], [[]], params)[0].fastq


def test_unsorted_stream_is_refused(tmp_path, synthetic):
    from proovread_amd import _abi, bamio, cns
    d, names, body = synthetic
    reads = [cns.LongRead(f"lr{i}", d.lr_str(i), "I" * len(d.lr_str(i))) for i in range(d.n_lr)]
    n1 = int.from_bytes(body[:4], "little") + 4
    swapped = body[n1:] + body[:n1]          # the first record (reference 0) goes last
    with pytest.raises(RuntimeError, match="not coordinate-sorted"):
        cns.run_bam_records(reads, names, swapped, cns.CnsParams(coverage=11.25))
    assert bamio._native_sort(swapped) == body
    res = cns.run_bam_records(reads, names, body, cns.CnsParams(coverage=11.25))
    assert all(r.status == 0 for r in res) and sum(len(r.kept) for r in res) >= 3000
    ms = C.c_double(-1.0)
    _abi.check(_abi.lib().pr_bam_decode_last_ms(_abi.default_context().h, C.byref(ms)), "pr_bam_decode_last_ms")
    assert ms.value > 0.0


def test_text_scores_reach_their_columns():
    """AS:Z scores are numified on the host and patched into the device column: with the reads
    ordered differently from the references, and a coverage low enough that the scores decide which
    alignments are kept, the result equals the host-decoded batch's."""
    import random
    from proovread_amd import bam2cns, cns
    rng = random.Random(3)
    refs = ["".join(rng.choice("ACGT") for _ in range(600)) for _ in range(3)]
    lines = []
    for r, ref in enumerate(refs):
        for k in range(60):
            p = rng.randrange(0, 500)
            seq = list(ref[p:p + 100])
            for j in rng.sample(range(100), 3):
                seq[j] = rng.choice("ACGT")
            lines.append(f"q{r}_{k}\t0\tlr{r}\t{p + 1}\t60\t100M\t*\t0\t0\t{''.join(seq)}\t{'I' * 100}\tAS:Z: {rng.randrange(100, 500)}.5x")
    names = ["lr0", "lr1", "lr2"]
    body = bamio_sorted(lines, names)
    reads = [cns.LongRead(f"lr{r}", refs[r], "5" * 600) for r in (2, 0, 1)]
    params = cns.CnsParams(coverage=3.0)
    rc, cols = bam_cases.host_decode(body)
    assert rc == 0 and (cols["score"] > 100).all()
    want = cns.run_packed(reads, bam2cns.pack_bam_chunk(reads, names, cols), params)
    got = cns.run_bam_records(reads, names, body, params)
    for g, w in zip(got, want):
        assert (g.status, g.fastq, g.trace) == (0, w.fastq, w.trace)
        assert np.array_equal(g.kept, w.kept) and 0 < g.kept.sum() < len(g.kept)


def bamio_sorted(lines, names):
    from proovread_amd import bamio
    return bamio._native_sort(bam_cases.encode(lines, names))


def test_run_bam_equals_bam2cns_host_decoder(synthetic):
    """The device-decoded batch gives the consensus the host-decoded batch gives
    (pr_bam_decode_alns + pack_bam_chunk + pr_cns_run), a read without records included."""
    from proovread_amd import bam2cns, cns
    d, names, body = synthetic
    reads = [cns.LongRead(f"lr{i}", d.lr_str(i), "I" * len(d.lr_str(i))) for i in range(d.n_lr)]
    reads.insert(3, cns.LongRead("lr_none", "ACGTTGCA" * 50, "5" * 400))
    params = cns.CnsParams(coverage=11.25, detect_chimera=True)
    rc, cols = bam_cases.host_decode(body)
    assert rc == 0
    want = cns.run_packed(reads, bam2cns.pack_bam_chunk(reads, names, cols), params)
    got = cns.run_bam_records(reads, names, body, params)
    assert len(got[3].kept) == 0
    for g, w in zip(got, want):
        assert (g.id, g.status, g.fastq, g.trace, g.chim) == (w.id, w.status, w.fastq, w.trace, w.chim)
        assert np.array_equal(g.kept, w.kept)
        assert np.array_equal(g.bin_bases, w.bin_bases)

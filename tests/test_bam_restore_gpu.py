"""PR_BAM_RESTORE_SEQ on the device (bam_donor_kernel, bam_lookup_kernel, bam_unpack_restore_kernel;
DESIGN.md §10): a stream with `*` SEQ on its secondary records, decoded with the option, against
the same stream rewritten by the plain-Python rule (bam_restore_cases.restore) and decoded by the
path that was there before the option -- columns and pools, the consensus, the loop's files."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import bam_cases
import bam_restore_cases as rc
from proovread_amd.bam2cns import _BamAlns

pytestmark = pytest.mark.gpu

BATCH = ("lr0", "lr1", "lr2")
PARENT_TEXT = "Cannot handle BAM secondary alignments without seq/qual"


def decode(body: bytes, flags: int):
    """pr_bam_decode_alns_gpu (flags None) or pr_bam_decode_alns_gpu_opts -> (rc, columns, restored)."""
    from proovread_amd import _abi
    L = _abi.lib()
    L.pr_bam_alns_free.argtypes = [C.POINTER(_BamAlns)]
    L.pr_bam_alns_free.restype = None
    a = _BamAlns()
    nr = C.c_int64(-1)
    h = _abi.default_context().h
    if flags is None:
        code = L.pr_bam_decode_alns_gpu(h, body, len(body), C.byref(a))
    else:
        code = L.pr_bam_decode_alns_gpu_opts(h, body, len(body), flags, C.byref(a), C.byref(nr))
    if code:
        return code, None, nr.value
    try:
        return 0, bam_cases.take_alns(a), nr.value
    finally:
        L.pr_bam_alns_free(C.byref(a))


def last_error() -> str:
    from proovread_amd import _abi
    return _abi.lib().pr_last_error().decode()


@pytest.fixture(scope="module")
def job():
    """The directed stream: long reads, its lines, the oracle's lines, both as record streams."""
    from proovread_amd import bamio, cns
    lrs, lines = rc.directed()
    want_lines, donor_of = rc.restore(lines, kept=set(BATCH))
    assert rc.restore(lines)[0] == want_lines          # every `*` record lies on a read of the batch
    body, want_body = bam_cases.encode(lines, rc.NAMES), bam_cases.encode(want_lines, rc.NAMES)
    assert bamio._native_sort(body) == body and bamio._native_sort(want_body) == want_body
    reads = [cns.LongRead(k, lrs[k], "5" * len(lrs[k])) for k in BATCH]
    return {"lrs": lrs, "lines": lines, "want_lines": want_lines, "donor_of": donor_of, "body": body,
            "want_body": want_body, "reads": reads}


def same_results(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g.id, g.status, g.fastq, g.trace, g.chim_lines()) == (w.id, 0, w.fastq, w.trace, w.chim_lines())
        assert np.array_equal(g.kept, w.kept)


def test_decode_equals_the_decode_of_the_restored_stream(job):
    code, want, _ = decode(job["want_body"], None)
    assert code == 0, last_error()
    code, host = bam_cases.host_decode(job["want_body"])
    assert code == 0
    bam_cases.assert_same(want, host)
    code, got, nr = decode(job["body"], 1)
    assert code == 0, last_error()
    assert nr == len(job["donor_of"]) >= 50
    bam_cases.assert_same(got, want)          # field by field, pool byte by pool byte
    assert not (got["flags"] & 4).any() and (got["flags"] & 2).any()
    # flags = 0 is the call without options
    code, plain, _ = decode(job["body"], None)
    code0, plain0, nr0 = decode(job["body"], 0)
    assert code == 0 and code0 == 0 and nr0 == 0
    bam_cases.assert_same(plain0, plain)
    assert int((plain["flags"] & 4).astype(bool).sum()) == len(job["donor_of"])


@pytest.mark.parametrize("split", [1, 2])
def test_consensus_equals_the_restored_stream(job, split):
    """split = 2: lr2's records take donors that lie on lr0 and lr1, reads of the other range."""
    from proovread_amd import cns
    params = cns.CnsParams(coverage=30.0, detect_chimera=True)
    want = cns.run_bam_records(job["reads"], rc.NAMES, job["want_body"], params, split=split)
    assert sum(len(r.kept) for r in want) >= 100
    got = cns.run_bam_records(job["reads"], rc.NAMES, job["body"], params, split=split, restore_seq=True)
    same_results(got, want)
    # without the option the stream is refused as it always was
    with pytest.raises(RuntimeError, match=PARENT_TEXT) as e:
        cns.run_bam_records(job["reads"], rc.NAMES, job["body"], params, split=split)
    assert "PR_ERR_NOSEQ" in str(e.value)


def test_every_donor_is_found_behind_its_collisions():
    lines = rc.probing()
    n = len(lines) // 2
    assert n == 2000 and n - len({rc.fnv_home_slot(f"q{i:04d}", 0, 4095) for i in range(n)}) >= 200
    want_lines, donor_of = rc.restore(lines)
    assert donor_of == {i: n + i for i in range(n)}
    code, want, _ = decode(bam_cases.encode(want_lines, ["lr0", "lr1"]), None)
    assert code == 0, last_error()
    code, got, nr = decode(bam_cases.encode(lines, ["lr0", "lr1"]), 1)
    assert code == 0, last_error()
    assert nr == n
    bam_cases.assert_same(got, want)
    # every primary SEQ is unique, so the bases a record got name its donor
    seqs = got["seq"].reshape(2 * n, 24)
    assert len({bytes(r) for r in seqs[n:]}) == n
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    for i in range(n):
        d = bytes(seqs[n + i])
        assert bytes(seqs[i]) == (d[::-1].translate(comp) if i % 2 else d), i


def test_the_lower_record_index_wins():
    lines = ["d\t0\tlr0\t9\t60\t4M\t*\t0\t0\tGGGG\tIIII", "d\t256\tlr0\t10\t0\t4M\t*\t0\t0\t*\t*",
             "d\t0\tlr0\t11\t60\t4M\t*\t0\t0\tACGT\t5555", "d\t1024\tlr1\t1\t60\t4M\t*\t0\t0\tTTTT\t*",
             "d\t272\tlr1\t2\t0\t1H3M\t*\t0\t0\t*\t*"] + [f"d\t0\tlr1\t{3 + k}\t60\t4M\t*\t0\t0\tAAAA\t*" for k in range(300)]
    want_lines, donor_of = rc.restore(lines)
    assert donor_of == {1: 0, 4: 0}
    code, want, _ = decode(bam_cases.encode(want_lines, ["lr0", "lr1"]), None)
    code1, got, nr = decode(bam_cases.encode(lines, ["lr0", "lr1"]), 1)
    assert code == 0 and code1 == 0 and nr == 2
    bam_cases.assert_same(got, want)
    assert bytes(got["seq"][4:8]) == b"GGGG" and bytes(got["seq"][16:19]) == b"CCC"


@pytest.mark.parametrize("case", sorted(rc.REFUSALS))
def test_refusals_between_two_exact_calls(job, case):
    """The rule's refusals (tests/test_bam_restore_host.py shows each on the host build first),
    from both entry points, between two calls that must stay exact on the same context."""
    from proovread_amd import _abi, cns
    lines, code, index = rc.REFUSALS[case]
    qname = lines[index].split("\t")[0]
    body = bam_cases.encode(lines, ["lr0"])
    params = cns.CnsParams(coverage=30.0)
    code_w, want, _ = decode(job["want_body"], None)
    want_cns = cns.run_bam_records(job["reads"], rc.NAMES, job["want_body"], params)

    got = decode(body, 1)
    assert got[0] == code and f"({qname})" in last_error() and f"record {index} " in last_error()
    code_g, again, nr = decode(job["body"], 1)
    assert code_w == 0 and code_g == 0 and nr == len(job["donor_of"])
    bam_cases.assert_same(again, want)

    reads = [cns.LongRead("lr0", "ACGT" * 30, "5" * 120)]
    with pytest.raises(RuntimeError, match=_abi.ERRORS[code]) as e:
        cns.run_bam_records(reads, ["lr0"], body, params, restore_seq=True)
    assert f"({qname})" in str(e.value)
    bd = _abi.CnsBounds()                                # nothing is left resident
    assert _abi.lib().pr_cns_resident_bounds(_abi.default_context().h, C.byref(bd)) == -1
    same_results(cns.run_bam_records(job["reads"], rc.NAMES, job["body"], params, restore_seq=True), want_cns)
    # the same stream without the option: the refusal that was always there
    with pytest.raises(RuntimeError, match=PARENT_TEXT):
        cns.run_bam_records(reads, ["lr0"], body, params)
    assert decode(body, 0)[0] == 0                       # (the plain decoder has never refused a record without SEQ)


def _write_job(td: Path, job):
    from proovread_amd import bamio
    head = "".join(f"@SQ\tSN:{n}\tLN:{len(job['lrs'].get(n, 'A' * rc.REPEAT))}\n" for n in rc.NAMES)
    for tag, lines in (("raw", job["lines"]), ("restored", job["want_lines"])):
        (td / f"{tag}.sam").write_text(head + "".join(ln + "\n" for ln in lines))
        with open(td / f"{tag}.sam") as fh:
            bamio.write_bam_from_sam(fh, str(td / f"{tag}.unsorted.bam"))
        bamio.sort_bam(str(td / f"{tag}.unsorted.bam"), str(td / f"{tag}.bam"))


@pytest.mark.parametrize("mode", ["sam", "bam"])
def test_loop_equals_the_run_on_the_restored_file(job, tmp_path, mode):
    from proovread_amd import correct
    _write_job(tmp_path, job)
    lrs = [(k, job["lrs"][k].encode(), b"5" * len(job["lrs"][k])) for k in BATCH]
    out = {}
    for tag, restore in (("raw", True), ("restored", False)):
        cfg = correct.LoopConfig(coverage=40.0, restore_seq=restore, **{mode: str(tmp_path / f"{tag}.{mode}")})
        res = correct.run(lrs, b"", cfg)
        assert [e.task for e in res.log] == ["read-long", "read-" + mode] and res.log[1].n_tasks >= 60
        pre = str(tmp_path / f"{tag}_{mode}")
        correct.write_outputs(res, pre, min_length=100)
        out[tag] = (list(res.reads.ids), [bytes(x) for x in res.reads.seqs], [bytes(x) for x in res.reads.quals], list(res.chim),
                    {ext: Path(pre + ext).read_text() for ext in (".untrimmed.fq", ".trimmed.fq", ".chim.tsv")})
    assert out["raw"] == out["restored"]
    assert out["raw"][0] == list(BATCH) and out["raw"][4][".trimmed.fq"]
    with pytest.raises(RuntimeError, match=PARENT_TEXT):
        correct.run(lrs, b"", correct.LoopConfig(coverage=40.0, **{mode: str(tmp_path / f"raw.{mode}")}))
    # the command line: the stock-style file goes through with the flag and fails as before without it
    (tmp_path / "lr.fq").write_text("".join(f"@{k}\n{job['lrs'][k]}\n+\n{'5' * len(job['lrs'][k])}\n" for k in BATCH))
    argv = ["-l", str(tmp_path / "lr.fq"), "--" + mode, str(tmp_path / f"raw.{mode}"), "--coverage", "40", "-p"]
    assert correct.main(argv + [str(tmp_path / "cli"), "--restore-secondary-seq"]) == 0
    assert (tmp_path / "cli.untrimmed.fq").read_text() == out["raw"][4][".untrimmed.fq"]
    with pytest.raises(RuntimeError, match=PARENT_TEXT):
        correct.main(argv + [str(tmp_path / "cli_plain")])

"""`correct --sam` / `correct --bam` end to end on a small synthetic job mapped with the
bwa-proovread drop-in, against the existing pipeline pieces run by hand on the same file:
bam2cns over 100-read chunks with correct_sr_mt's parameters (bin/proovread:1534-1619), merged,
then write_outputs."""
import io
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

COVERAGE = 50.0
FILES = (".untrimmed.fq", ".chim.tsv", ".trimmed.fq")
N_READS = 44


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """lr.fq (40 long reads of about 4.5 kb and four chimeras of two of them each), x.sam as the
    drop-in writes it (short-read order) and x.bam, its coordinate-sorted BAM."""
    from proovread_amd import bamio, bwa_proovread, synth
    from proovread_amd import tasks as T
    td = tmp_path_factory.mktemp("sam_bam_modes")
    d = synth.simulate(11, 60000, 40, 4300, 15.0)
    lrs = [d.lr_str(i) for i in range(d.n_lr)]
    for a, b, cut in ((2, 30, 2200), (5, 25, 1500), (12, 36, 3000), (20, 1, 2600)):
        lrs.append(lrs[a][:cut] + lrs[b][cut:])   # chimeric reads: two loci joined
    names = [f"lr{i}" for i in range(len(lrs))]
    (td / "lr.fq").write_text("".join(f"@{n}\n{s}\n+\n{'5' * len(s)}\n" for n, s in zip(names, lrs)))
    (td / "lr.fa").write_text("".join(f">{n}\n{s}\n" for n, s in zip(names, lrs)))
    (td / "sr.fq").write_text("".join(f"@sr{i}\n{d.sr_str(i)}\n+\n{'I' * len(d.sr_str(i))}\n" for i in range(d.n_sr)))
    with open(td / "x.sam", "w") as out:
        assert bwa_proovread.mem(T.bwa_argv("bwa-sr-1") + [str(td / "lr.fa"), str(td / "sr.fq")], out=out,
                                 log=io.StringIO()) == 0
    with open(td / "x.sam") as fh:
        bamio.write_bam_from_sam(fh, str(td / "unsorted.bam"))
    bamio.sort_bam(str(td / "unsorted.bam"), str(td / "x.bam"))
    return td


def by_hand(job, pre: str, detect_chimera: bool) -> None:
    """read-long, bam2cns per 100-read chunk, merge, write_outputs."""
    from proovread_amd import bam2cns, cns, correct
    from proovread_amd.bwa_proovread import read_fastx
    names, seqs, quals = read_fastx(str(job / "lr.fq"))
    reads, ignored = correct.read_long(list(zip(names, seqs, quals)), 400)
    ref = pre + ".read-long.fq"
    Path(ref).write_text(reads.fastq())
    recs = reads.fastq().split("\n")
    args = ["--bam", str(job / "x.bam"), "--ref", ref, "--prefix", pre + ".cns", "--append", "--max-ref-seqs", "100",
            "--coverage", cns.perl_num(min(COVERAGE, 15.0) * 0.75), "--bin-size", "20", "--max-ins-length", "0",
            "--use-ref-qual"] + (["--detect-chimera"] if detect_chimera else [])
    for first in range(0, len(reads.ids), 100):
        off = sum(len(x) + 1 for x in recs[:4 * first])
        assert bam2cns.main(args + ["--ref-offset", str(off)]) == 0
    n2, s2, q2 = read_fastx(pre + ".cns.fq")
    assert n2 == reads.ids
    correct.write_outputs(correct.LoopResult(correct.LongReads(n2, s2, q2), raw_chim(pre), ignored, []), pre)


def read(pre: str):
    return {ext: Path(pre + ext).read_text() for ext in FILES}


def raw_chim(pre: str):
    """bam2cns's own chimera lines (before ChimeraToSeqFilter)."""
    return [ln for ln in Path(pre + ".cns.chim.tsv").read_text().split("\n") if ln]


@pytest.fixture(scope="module")
def outputs(job):
    from proovread_amd import correct
    from proovread_amd.bwa_proovread import read_fastx
    pre = {k: str(job / k) for k in ("bam", "sam", "hand", "hand_chim")}
    base = ["-l", str(job / "lr.fq"), "--coverage", str(COVERAGE)]
    assert correct.main(base + ["--bam", str(job / "x.bam"), "-p", pre["bam"]]) == 0
    assert correct.main(base + ["--sam", str(job / "x.sam"), "-p", pre["sam"]]) == 0
    by_hand(job, pre["hand"], False)
    by_hand(job, pre["hand_chim"], True)
    out = {k: read(p) for k, p in pre.items()}
    # the tasks' own chimera lines (before ChimeraToSeqFilter), from the loop the command line runs
    lrs = list(zip(*read_fastx(str(job / "lr.fq"))))
    for k in ("sam", "bam"):
        res = correct.run(lrs, b"", correct.LoopConfig(coverage=COVERAGE, **{k: str(job / ("x." + k))}))
        out[k]["lines"] = res.chim
        out[k]["tasks"] = [e.task for e in res.log]
    out["hand"]["lines"], out["hand_chim"]["lines"] = raw_chim(pre["hand"]), raw_chim(pre["hand_chim"])
    return out


def test_bam_mode_equals_the_pipeline_by_hand(outputs):
    got, want = outputs["bam"], outputs["hand"]
    assert got["tasks"] == ["read-long", "read-bam"]
    assert got[".untrimmed.fq"].count("\n") == 4 * N_READS and got[".trimmed.fq"]
    for ext in FILES:
        assert got[ext] == want[ext], ext


def test_sam_mode_equals_bam_mode_but_detects_chimeras(outputs):
    sam, bam = outputs["sam"], outputs["bam"]
    assert sam["tasks"] == ["read-long", "read-sam"]
    assert sam[".untrimmed.fq"] == bam[".untrimmed.fq"]            # the same consensus from the unsorted SAM
    # read-sam detects chimeras, read-bam does not (proovread.cfg:205-211): the only difference
    assert bam["lines"] == [] and outputs["hand"]["lines"] == []
    assert len(sam["lines"]) >= 1 and sam["lines"] == outputs["hand_chim"]["lines"]
    for ext in FILES:
        assert sam[ext] == outputs["hand_chim"][ext], ext

"""proovread's sam / bam modes on the host side: the task tables (proovread.cfg:130-132, 205-211,
259-273) and the command line's rules for --sam / --bam / -m (bin/proovread:346-350, 628-632).
No device work."""
import pytest

from proovread_amd import correct, tasks as T


def test_mode_tasks():
    assert T.MODE_TASKS["sam"] == ("read-long", "read-sam")
    assert T.MODE_TASKS["bam"] == ("read-long", "read-bam")
    # the modes that were there stay as they were
    assert T.MODE_TASKS["sr-noccs"][0] == "read-long" and T.MODE_TASKS["sr-noccs"][-1] == "bwa-sr-finish"
    assert T.MODE_TASKS["mr-noccs"][-1] == "bwa-mr-finish"


def test_detect_chimera_table_keeps_the_read_bam_quirk():
    assert T.DETECT_CHIMERA == {"DEF": 0, "bwa-sr-finish": 1, "bwa-mr-finish": 1, "read-sam": 1}
    assert T.detect_chimera("read-sam") is True
    assert T.detect_chimera("read-bam") is False   # not listed in proovread.cfg:205-211: falls to DEF
    assert T.detect_chimera("bwa-sr-finish") and T.detect_chimera("bwa-mr-finish")
    assert not T.detect_chimera("bwa-sr-3") and not T.detect_chimera("bwa-mr-1")


def test_bin_size_and_coverage_of_the_new_modes():
    assert T.bin_size("sam") == 20 and T.bin_size("bam") == 20
    assert T.bin_size("sr-noccs") == 20 and T.bin_size("mr-noccs") == 50
    assert T.sr_coverage("read-sam") == 15.0 and T.sr_coverage("read-bam") == 15.0   # DEF
    assert T.mode_for(100) == "sr-noccs" and T.mode_for(151) == "mr-noccs"           # unchanged


@pytest.fixture()
def files(tmp_path):
    out = {}
    for name in ("lr.fq", "sr.fq", "x.sam", "x.bam"):
        p = tmp_path / name
        p.write_text("")
        out[name] = str(p)
    return out


def test_short_reads_are_optional_only_with_sam_or_bam(files, capsys):
    with pytest.raises(SystemExit):
        correct.parse_args(["-l", files["lr.fq"], "-p", "out"])
    assert "--sam" in capsys.readouterr().err
    a = correct.parse_args(["-l", files["lr.fq"], "-p", "out", "--sam", files["x.sam"]])
    assert a.short_reads == [] and a.sam == files["x.sam"] and a.bam is None
    a = correct.parse_args(["-l", files["lr.fq"], "-p", "out", "--bam", files["x.bam"]])
    assert a.short_reads == [] and a.bam == files["x.bam"]
    a = correct.parse_args(["-l", files["lr.fq"], "-p", "out", "-s", files["sr.fq"]])
    assert a.short_reads == [files["sr.fq"]] and a.sam is None and a.bam is None


def test_long_reads_stay_required(files):
    with pytest.raises(SystemExit):
        correct.parse_args(["-p", "out", "--bam", files["x.bam"]])
    with pytest.raises(SystemExit):
        correct.parse_args(["-p", "out", "-s", files["sr.fq"]])


def test_mode_follows_the_flag(files):
    base = ["-l", files["lr.fq"], "-p", "out"]
    assert correct.parse_args(base + ["--sam", files["x.sam"]]).mode == "sam"
    assert correct.parse_args(base + ["--bam", files["x.bam"]]).mode == "bam"
    # bin/proovread:628-632: --bam wins over --sam, and both over -m
    assert correct.parse_args(base + ["--sam", files["x.sam"], "--bam", files["x.bam"]]).mode == "bam"
    assert correct.parse_args(base + ["--sam", files["x.sam"], "-m", "sr-noccs"]).mode == "sam"
    assert correct.parse_args(base + ["-s", files["sr.fq"], "--bam", files["x.bam"]]).mode == "bam"
    assert correct.parse_args(base + ["-s", files["sr.fq"]]).mode is None          # by short-read length
    assert correct.parse_args(base + ["-s", files["sr.fq"], "-m", "mr-noccs"]).mode == "mr-noccs"
    assert correct.parse_args(base + ["-s", files["sr.fq"], "--mode", "sr-noccs"]).mode == "sr-noccs"


def test_bad_modes_and_missing_files_are_refused(files, tmp_path):
    base = ["-l", files["lr.fq"], "-p", "out"]
    with pytest.raises(SystemExit):
        correct.parse_args(base + ["-s", files["sr.fq"], "-m", "ccs-1"])
    with pytest.raises(SystemExit):   # mode sam without its file
        correct.parse_args(base + ["-s", files["sr.fq"], "-m", "sam"])
    with pytest.raises(SystemExit):
        correct.parse_args(base + ["--bam", str(tmp_path / "missing.bam")])
    with pytest.raises(SystemExit):
        correct.parse_args(base + ["--sam", str(tmp_path / "missing.sam")])


def test_loop_config_mode(files):
    assert correct.mode_of(correct.LoopConfig()) is None
    assert correct.mode_of(correct.LoopConfig(mode="mr-noccs")) == "mr-noccs"
    assert correct.mode_of(correct.LoopConfig(mode="mr-noccs", sam="x.sam")) == "sam"
    assert correct.mode_of(correct.LoopConfig(sam="x.sam", bam="x.bam")) == "bam"


def test_read_tasks_need_their_file():
    """run_tasks refuses read-sam / read-bam without the file before touching the stages."""
    srs = correct.ShortReads(b"")
    for task in ("read-sam", "read-bam"):
        with pytest.raises(ValueError, match=task):
            correct.run_tasks(object(), srs, [task], correct.LoopConfig(), task[5:], 200, True)

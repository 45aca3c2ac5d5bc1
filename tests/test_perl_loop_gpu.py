"""perl/bin/prgpu-proovread on the GPU: the correction loop driven from Perl over the resident
XS entry points (perl/lib/Prgpu/Stages.pm) against proovread_amd.correct on the same inputs.

Each test runs correct.run + write_outputs in this process, then the Perl driver as one fresh
child on the same input files, and compares the five output files byte for byte and the task
log row by row: the sr job and the mr job of test_correct_loop, the bundled F.antasticus sample
with 50x short reads, a user configuration (-c), and the refusal of a task outside the loop.
This also puts write_outputs' ChimeraToSeqFilter / SeqFilter --trim-win path after a device
loop under a GPU test."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from proovread_amd import correct
from proovread_amd.seqfilter import read_records
from test_correct_loop import _exact, _inputs, _kmers, _sample_inputs

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "perl" / "bin" / "prgpu-proovread"
XS_SO = ROOT / "perl" / "lib" / "auto" / "Prgpu" / "Prgpu.so"
XS_SRC = ROOT / "perl" / "Prgpu.xs"
FILES = ("untrimmed.fq", "chim.tsv", "ignored.tsv", "trimmed.fq", "trimmed.fa")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("perl") is None, reason="no perl")]


@pytest.fixture(scope="module", autouse=True)
def xs_module():
    if not XS_SO.exists() or XS_SO.stat().st_mtime < XS_SRC.stat().st_mtime:
        subprocess.run(["make", "-s", "-C", str(ROOT / "perl")], check=True)
    return XS_SO


def _write_inputs(tmp_path, lrs, srd):
    with open(tmp_path / "lr.fx", "wb") as f:
        for rid, s, q in lrs:
            f.write(b">%s\n%s\n" % (rid.encode(), s) if q is None else b"@%s\n%s\n+\n%s\n" % (rid.encode(), s, q))
    (tmp_path / "sr.fq").write_bytes(srd)
    return ["-l", str(tmp_path / "lr.fx"), "-s", str(tmp_path / "sr.fq")]


def _driver(args):
    return subprocess.run(["perl", str(DRIVER), *args], capture_output=True, text=True, timeout=600)


def _task_rows(path):
    rows = [ln.split("\t") for ln in Path(path).read_text().split("\n") if ln and not ln.startswith("#")]
    assert all(len(r) == 7 for r in rows)
    return [(r[0], int(r[1]), int(r[2]), int(r[3]), int(r[4]), r[6]) for r in rows], [r[5] for r in rows]


def _compare(tmp_path, lrs, srd, cfg, extra=()):
    """The Python loop and the Perl driver on the same inputs -> (Python result, driver stderr)."""
    want = correct.run(lrs, srd, cfg)
    correct.write_outputs(want, str(tmp_path / "py"))
    r = _driver(_write_inputs(tmp_path, lrs, srd) + ["-p", str(tmp_path / "pl"), "--coverage", str(cfg.coverage), *extra])
    assert r.returncode == 0, r.stderr
    for f in FILES:
        py, pl = tmp_path / f"py.{f}", tmp_path / f"pl.{f}"
        assert py.exists() == pl.exists(), f
        if py.exists():
            assert pl.read_bytes() == py.read_bytes(), f
    rows, fracs = _task_rows(tmp_path / "pl.tasks.tsv")
    assert rows == [(e.task, e.n_sr, e.n_tasks, e.bpt, e.bpn, e.shortcut) for e in want.log]
    for e, f in zip(want.log, fracs):
        assert (f == "") == (e.masked_frac is None)
        if f:
            assert float(f) == pytest.approx(e.masked_frac, rel=1e-12)
    # the per-task lines correct.main prints
    lines = [f"{e.task}: {e.n_sr} short reads, masked {100 * e.masked_frac:.1f}% {e.shortcut}"
             for e in want.log if e.masked_frac is not None]
    assert [ln for ln in r.stderr.split("\n") if "short reads, masked" in ln] == lines
    return want, r.stderr


def _check_trimmed(pre, want):
    """What test_loop_outputs_on_sample asserts of the trimmed reads, after the device loop."""
    un = read_records(pre + ".untrimmed.fq")
    assert [x[2] for x in un] == want.reads.seqs
    tr = read_records(pre + ".trimmed.fq")
    fa = read_records(pre + ".trimmed.fa")
    assert tr and [x[2] for x in tr] == [x[2] for x in fa]
    full = dict(zip(want.reads.ids, want.reads.seqs))
    for x in tr:
        rid = x[0].split()[0]
        base = rid.rsplit(".", 1)[0] if rid not in full else rid
        assert len(x[2]) >= 500 and x[2] in full[base], rid
    return tr


def test_sr_job(tmp_path):
    _, lrs, srd = _inputs(seed=6)
    want, _ = _compare(tmp_path, lrs, srd, correct.LoopConfig(coverage=40.0))
    assert [e.task for e in want.log][:2] == ["read-long", "bwa-sr-1"] and want.log[-1].task == "bwa-sr-finish"
    assert want.log[1].n_sr < 6400 and want.log[1].n_tasks > 0       # sampled, seeded
    for pre in ("py", "pl"):
        _check_trimmed(str(tmp_path / pre), want)


def test_mr_job(tmp_path):
    _, lrs, srd = _inputs(seed=10, sr_len=300)
    want, _ = _compare(tmp_path, lrs, srd, correct.LoopConfig(coverage=40.0))
    assert want.log[1].task == "bwa-mr-1" and want.log[-1].task == "bwa-mr-finish"   # bin size 50 in -b/-l
    _check_trimmed(str(tmp_path / "pl"), want)


def test_bundled_sample(tmp_path):
    from test_fantasticus_chain import FX
    G, lrs, srd = _sample_inputs()
    want = correct.run(lrs, srd, correct.LoopConfig(coverage=50.0))
    correct.write_outputs(want, str(tmp_path / "py"))
    (tmp_path / "sr.fq").write_bytes(srd)
    r = _driver(["-l", str(FX / "F.antasticus_long_error.fq"), "-s", str(tmp_path / "sr.fq"), "-p", str(tmp_path / "pl")])
    assert r.returncode == 0, r.stderr
    for f in FILES:
        assert (tmp_path / f"pl.{f}").read_bytes() == (tmp_path / f"py.{f}").read_bytes(), f
    rows, _ = _task_rows(tmp_path / "pl.tasks.tsv")
    assert rows == [(e.task, e.n_sr, e.n_tasks, e.bpt, e.bpn, e.shortcut) for e in want.log]
    tr = _check_trimmed(str(tmp_path / "pl"), want)
    assert len(tr) >= 100
    km = _kmers(G)
    for pre in ("py", "pl"):     # the contamination read ends uncorrected, the genomic reads corrected
        n = 0
        for x in read_records(str(tmp_path / f"{pre}.untrimmed.fq")):
            if x[0].startswith("long_contamination"):
                assert _exact(x[2], km) < 0.5, x[0]
                n += 1
        assert n >= 1


def test_user_config(tmp_path):
    _, lrs, srd = _inputs(seed=6)
    lrs = lrs + [("lr_600", lrs[0][1][:600], None)]       # kept by default (>= 300), dropped by lr-min-length 1000
    (tmp_path / "user.cfg").write_text(
        "'mode-tasks' => {'sr-noccs' => ['read-long', 'bwa-sr-1', 'bwa-sr-finish']},\n"
        "'mask-shortcut-frac' => 0.5,\n'lr-min-length' => 1000,\n'chimera-filter' => {'--min-score' => 0.01},\n")
    cfg = correct.LoopConfig(coverage=40.0, tasks=("read-long", "bwa-sr-1", "bwa-sr-finish"), mask_shortcut_frac=0.5,
                             lr_min_length=1000)
    want, err = _compare(tmp_path, lrs, srd, cfg, extra=["-c", str(tmp_path / "user.cfg")])
    assert [e.task for e in want.log] == ["read-long", "bwa-sr-1", "bwa-sr-finish"]
    assert (tmp_path / "pl.ignored.tsv").read_text() == "lr_600\tstubby\n"
    assert err.count("config key 'chimera-filter' is not used") == 1


def test_task_outside_the_loop_is_refused(tmp_path):
    _, lrs, srd = _inputs(seed=6)
    (tmp_path / "user.cfg").write_text(
        "'mode-tasks' => {'sr-noccs' => ['read-long', 'bwa-sr-1', 'ccs-1', 'bwa-sr-finish']},\n")
    r = _driver(_write_inputs(tmp_path, lrs, srd) + ["-p", str(tmp_path / "pl"), "-c", str(tmp_path / "user.cfg")])
    assert r.returncode != 0 and "ccs-1" in r.stderr
    assert "short reads, masked" not in r.stderr and not list(tmp_path.glob("pl.*"))

#!/usr/bin/env python3
"""Time the correction loop under both hosts on the same files: `proovread_amd.correct` (Python
over ctypes) and `perl/bin/prgpu-proovread` (Perl over XS).  Both launch the same kernels through
the same resident entry points, so the device stage times should agree within run-to-run noise;
what differs is the host around them (parsing the inputs, sampling, the final outputs).

    python tools/time_perl_loop.py [--scale 0.1] [--out profiles/perl_loop_timing.json]
                                   [--workdir DIR] [--limit 600]

Writes a --scale share of the benchmark's workload (bench.py: 4.6 Mb genome, 13,800 x 10 kb long
reads, 50x 150 bp short reads; synth.simulate_reads) to a FASTA and a FASTQ file, then runs the
Python driver and the Perl driver on them, one after the other, each as a fresh process under
its own time limit; the second starts only if the first exits 0.  The Python driver runs as this
script's --python-child mode: correct.main's steps (read_fastx, run on GpuStages, write_outputs)
with a clock around each, since the module's command line prints no timing.  Recorded per
driver: the process wall clock, reading the input files, the loop, the final outputs, and per
task the device stage times (HIP events) and the host wall clock.  No pass/fail bar.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

GENOME, N_LR, SR_COV, SEED = 4_600_000, 13_800, 50.0, 20240229
FILES = ("untrimmed.fq", "chim.tsv", "ignored.tsv", "trimmed.fq", "trimmed.fa")


def write_inputs(work: Path, scale: float):
    import numpy as np
    from proovread_amd import synth
    gl, n_lr = int(GENOME * scale), max(1, int(N_LR * scale))
    n_sr = int(round(SR_COV * gl / 150))
    d = synth.simulate_reads(SEED, gl, n_lr, 10_000, n_sr, threads=8)
    acgt = np.frombuffer(b"ACGTN", np.uint8)
    lr = acgt[np.minimum(d.lr_seq, 4)].tobytes()
    sr = acgt[np.minimum(d.sr_seq, 4)].tobytes()
    with open(work / "lr.fa", "wb") as f:
        for i in range(n_lr):
            f.write(b">lr_%d\n%s\n" % (i, lr[int(d.lr_off[i]):int(d.lr_off[i + 1])]))
    with open(work / "sr.fq", "wb") as f:
        for i in range(n_sr):
            s = sr[int(d.sr_off[i]):int(d.sr_off[i + 1])]
            f.write(b"@sr%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    return {"genome": gl, "long_reads": n_lr, "long_read_bases": int(d.lr_off[-1]), "short_reads": n_sr}


def python_child(lr: str, sr: str, pre: str, out: str) -> int:
    t0 = time.perf_counter()
    from proovread_amd import correct
    from proovread_amd.bwa_proovread import read_fastx
    stages = correct.GpuStages()          # creates the device context, as the Perl driver does first
    t1 = time.perf_counter()
    names, seqs, quals = read_fastx(lr)
    with open(sr, "rb") as f:
        sr_data = f.read()
    t2 = time.perf_counter()
    res = correct.run(list(zip(names, seqs, quals)), sr_data, correct.LoopConfig(coverage=SR_COV), stages=stages)
    t3 = time.perf_counter()
    correct.write_outputs(res, pre)
    t4 = time.perf_counter()
    tasks = [{"task": e.task, "n_sr": e.n_sr, "n_tasks": e.n_tasks, "wall_ms": e.wall_ms, "pre_ms": e.pre_ms,
              "stage_ms": e.stage_ms, "part_ms": e.part_ms} for e in res.log]
    with open(out, "w") as f:
        json.dump({"context_ms": (t1 - t0) * 1e3, "read_files_ms": (t2 - t1) * 1e3, "loop_ms": (t3 - t2) * 1e3,
                   "outputs_ms": (t4 - t3) * 1e3, "total_ms": (t4 - t0) * 1e3, "tasks": tasks}, f)
    return 0


def _summ(t: dict, wall_s: float) -> dict:
    """One driver's record: the parts in ms, and per task the device stages and the host wall."""
    tasks = [x for x in t["tasks"] if x.get("stage_ms")]
    for x in tasks:
        x["device_ms"] = round(sum(x["stage_ms"].values()), 2)
    r = {"process_wall_s": round(wall_s, 3)}
    for k in ("context_ms", "read_files_ms", "sr_parse_ms", "loop_ms", "outputs_ms", "total_ms"):
        if k in t:
            r[k] = round(t[k], 1)
    r["loop_outside_tasks_ms"] = round(t["loop_ms"] - sum(x["wall_ms"] for x in tasks), 1)
    r["device_ms_all_tasks"] = round(sum(x["device_ms"] for x in tasks), 1)
    r["task_wall_ms_all_tasks"] = round(sum(x["wall_ms"] for x in tasks), 1)
    r["tasks"] = tasks
    return r


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "perl_loop_timing.json"))
    ap.add_argument("--workdir")
    ap.add_argument("--limit", type=int, default=600, help="seconds, per driver")
    ap.add_argument("--python-child", nargs=4, metavar=("LR", "SR", "PRE", "OUT"))
    a = ap.parse_args()
    if a.python_child:
        return python_child(*a.python_child)
    with tempfile.TemporaryDirectory(dir=a.workdir) as tmp:
        work = Path(tmp)
        rec = {"workload": write_inputs(work, a.scale), "scale": a.scale}
        lr, sr = str(work / "lr.fa"), str(work / "sr.fq")
        t = time.perf_counter()
        r = subprocess.run([sys.executable, __file__, "--python-child", lr, sr, str(work / "py"), str(work / "py.json")],
                           timeout=a.limit)
        py_wall = time.perf_counter() - t
        if r.returncode != 0:
            print(f"the Python driver exited {r.returncode}; the Perl driver was not started", file=sys.stderr)
            return 1
        t = time.perf_counter()
        r = subprocess.run(["perl", str(ROOT / "perl" / "bin" / "prgpu-proovread"), "-l", lr, "-s", sr, "-p", str(work / "pl"),
                            "--coverage", str(SR_COV), "--timing", str(work / "pl.json")], timeout=a.limit)
        pl_wall = time.perf_counter() - t
        if r.returncode != 0:
            print(f"the Perl driver exited {r.returncode}", file=sys.stderr)
            return 1
        rec["python"] = _summ(json.loads((work / "py.json").read_text()), py_wall)
        rec["perl"] = _summ(json.loads((work / "pl.json").read_text()), pl_wall)
        rec["outputs_equal"] = all((work / f"py.{f}").read_bytes() == (work / f"pl.{f}").read_bytes() for f in FILES)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in ("python", "perl"):
        print(k, {x: rec[k][x] for x in rec[k] if x != "tasks"})
    print("outputs equal:", rec["outputs_equal"])
    return 0


if __name__ == "__main__":
    sys.exit(main())

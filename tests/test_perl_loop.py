"""The host logic of the Perl correction loop (perl/lib/Prgpu/{Tasks,Control,ShortReads,Loop}.pm,
perl/bin/prgpu-proovread) against the Python modules it was ported from, without a GPU.

A helper (tests/perl_loop_helper.pl) runs the Perl side on JSON inputs; this file compares its
answers with proovread_amd.tasks, control, correct.ShortReads, correct.read_long and
correct.write_outputs: per-task option structs field by field, the sampler and the mask
shortcut, SeqChunker sampling on streams small enough to go wrong, read-long preprocessing,
and the five final files byte for byte.  Without a device the driver ends with the context's
error and writes nothing."""
import json
import os
import random
import shutil
import subprocess
from pathlib import Path

import pytest

from proovread_amd import control, correct, tasks as T

ROOT = Path(__file__).resolve().parent.parent
HELPER = Path(__file__).resolve().parent / "perl_loop_helper.pl"
DRIVER = ROOT / "perl" / "bin" / "prgpu-proovread"
XS_SO = ROOT / "perl" / "lib" / "auto" / "Prgpu" / "Prgpu.so"
XS_SRC = ROOT / "perl" / "Prgpu.xs"

pytestmark = pytest.mark.skipif(shutil.which("perl") is None, reason="no perl")


@pytest.fixture(scope="module", autouse=True)
def xs_module():
    # build() makes it; a fresh checkout, or one built before the resident bindings, gets it here
    if not XS_SO.exists() or XS_SO.stat().st_mtime < XS_SRC.stat().st_mtime:
        subprocess.run(["make", "-s", "-C", str(ROOT / "perl")], check=True)
    return XS_SO


def _helper(mode, payload, tmp_path):
    js = tmp_path / f"{mode}.json"
    js.write_text(json.dumps(payload))
    r = subprocess.run(["perl", str(HELPER), mode, str(js)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


# ---------------------------------------------------------------- tables
def test_tables_equal_tasks_py(tmp_path):
    names = sorted({t for m in ("sr-noccs", "mr-noccs") for t in T.MODE_TASKS[m] if t != "read-long"}
                   | {"bwa-mr-3", "bwa-sr-4"})
    modes = ["sr-noccs", "mr-noccs"]
    got = _helper("tables", {"tasks": names, "modes": modes, "lengths": [150, 151]}, tmp_path)
    for t in names:
        so, wo = T.options(t)
        g = got["tasks"][t]
        assert set(g["seed"]) == {n for n, _ in so._fields_} and set(g["sw"]) == {n for n, _ in wo._fields_}, t
        for n, _ in so._fields_:
            assert g["seed"][n] == getattr(so, n), (t, "seed", n)
        for n, _ in wo._fields_:
            assert g["sw"][n] == getattr(wo, n), (t, "sw", n)
        assert g["sr_coverage"] == T.sr_coverage(t), t
        assert g["hcr_mask"] == T.hcr_mask(t), t
        assert bool(g["detect_chimera"]) == T.detect_chimera(t), t
    assert got["tasks"]["bwa-mr-3"]["seed"]["min_seed_len"] == 13        # falls back to bwa-mr
    assert got["bin_size"] == {m: T.bin_size(m) for m in modes} == {"sr-noccs": 20, "mr-noccs": 50}
    assert got["mode_for"] == {"150": T.mode_for(150), "151": T.mode_for(151)} == {"150": "sr-noccs", "151": "mr-noccs"}
    assert got["mode_tasks"] == {m: list(T.MODE_TASKS[m]) for m in modes}


# ---------------------------------------------------------------- control
def test_cov2seqchunker_and_mask_shortcut(tmp_path):
    # one Sampler over the whole grid on both sides: first_chunk carries from call to call
    grid = [[c, tc] for c in (50.0, 40.0, 33.0, 20.0, 15.0) for tc in (15.0, 30.0, 40.0, 50.0, 7.5)]
    assert any(tc >= c for c, tc in grid)
    full = ["bwa-sr-1", "bwa-sr-2", "bwa-sr-3", "bwa-sr-4", "bwa-sr-5", "bwa-sr-6", "bwa-sr-finish"]
    cases = [
        {"tasks": full, "tc": 0, "frac": 0.5, "fracs": [], "shortcut_frac": 0.92, "min_gain": 0.03},          # below
        {"tasks": full, "tc": 1, "frac": 0.95, "fracs": [0.5], "shortcut_frac": 0.92, "min_gain": 0.03},      # above, tasks left
        {"tasks": full, "tc": 5, "frac": 0.95, "fracs": [0.5, 0.7], "shortcut_frac": 0.92, "min_gain": 0.03},  # last regular
        {"tasks": full, "tc": 2, "frac": 0.71, "fracs": [0.5, 0.7], "shortcut_frac": 0.92, "min_gain": 0.03},  # gain too small
        {"tasks": full, "tc": 4, "frac": 0.95, "fracs": [0.5], "shortcut_frac": 0.92, "min_gain": 0.03},      # one task to drop
        {"tasks": full, "tc": 1, "frac": 0.95, "fracs": [0.5], "shortcut_frac": 0, "min_gain": 0.03},         # switched off
    ]
    got = _helper("control", {"grid": grid, "sampling": 1, "shortcut": cases}, tmp_path)
    s = control.Sampler()
    want = [s.cov2seqchunker(c, tc) for c, tc in grid]
    assert got["sc"] == want
    assert any(w is None for w in want) and any(w is not None for w in want)
    res = []
    for c, g in zip(cases, got["shortcut"]):
        tasks, fracs = list(c["tasks"]), list(c["fracs"])
        r = control.mask_shortcut(tasks, c["tc"], c["frac"], fracs, c["shortcut_frac"], c["min_gain"])
        assert (g["res"], g["tasks"], g["fracs"]) == (r, tasks, fracs), c
        res.append((r, len(tasks)))
    assert res == [("continue", 7), ("skip", 3), ("", 7), ("skip", 4), ("skip", 6), ("", 7)]
    off = _helper("control", {"grid": grid[:3], "sampling": 0, "shortcut": []}, tmp_path)
    assert off["sc"] == [None, None, None]


# ---------------------------------------------------------------- sampling
def _fq(lens, name="r"):
    rnd = random.Random(11)
    return "".join("@%s%d\n%s\n+\n%s\n" % (name, i, "".join(rnd.choice("ACGTN") for _ in range(n)), "I" * n)
                   for i, n in enumerate(lens)).encode()


SCS = [{"--chunk-number": 0, "--chunk-step": 20, "--chunks-per-step": 6, "--first-chunk": 3},
       {"--chunk-number": 0, "--chunk-step": 2, "--chunks-per-step": 1, "--first-chunk": 2},
       {"--chunk-number": 0, "--chunk-step": 3, "--chunks-per-step": 2, "--first-chunk": 1},
       None]                                           # --no-sampling: one range of everything

STREAMS = {
    # more chunks than records: chunks of one byte, most of them empty
    "seven_in_1000": (_fq([7] * 7), 1000),
    # 176 bytes in 4 chunks of 44: records start at 44, 88 (no: 74..96 straddles 88) and 132
    "boundaries": (_fq([7, 7, 11, 7, 3, 7, 11, 3]), 4),
    # 154 bytes in 4 chunks of 39: the last chunk is short
    "not_divisible": (_fq([7] * 7), 4),
    "fasta_multiline": (b">a desc\nACGTAC\nGTNN\n>b\nacgt\n\n>c\nGG\nCC\nTT\n>d\nA\n", 3),
    # a blank line between records and CRLF ends: not plain 4-line FASTQ, the record parser
    "fastq_irregular": (b"@a\nACGT\n+\nIIII\n\n@b\r\nGGCCA\r\n+\r\nIIIII\r\n@c\nTT\n+\nII\n", 2),
}


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_sampling_equals_shortreads(name, tmp_path):
    data, n_chunks = STREAMS[name]
    (tmp_path / "sr.txt").write_bytes(data)
    got = _helper("sample", {"file": str(tmp_path / "sr.txt"), "chunk_number": n_chunks, "scs": SCS}, tmp_path)
    srs = correct.ShortReads(data, n_chunks)
    assert got["n"] == len(srs.lengths) and got["min_length"] == int(srs.lengths.min())
    assert got["pool"] == srs.pool.tobytes().hex()
    for sc, g in zip(SCS, got["samples"]):
        rg, off = srs.sample_ranges(sc)
        assert g["ranges"] == rg.tolist(), (name, sc)
        assert g["off"] == off.tolist(), (name, sc)
    if name == "seven_in_1000":       # ranges of empty chunks are dropped, not kept as [k, k]
        rg, _ = srs.sample_ranges(SCS[0])
        assert 0 < len(rg) < 7 and all(b > a for a, b in rg.tolist())
    if name == "boundaries":
        starts = [0, 22, 44, 74, 96, 110, 132, 162]
        assert len(data) == 176 and [data.index(b"@r%d\n" % i) for i in range(8)] == starts
        assert 44 in starts and any(a < 88 < b for a, b in zip(starts, starts[1:]))
        assert srs.cfirst.tolist() == [0, 2, 4, 6, 8]
    if name == "not_divisible":
        assert len(data) % n_chunks != 0 and srs.cfirst.tolist()[-1] == 7


# ---------------------------------------------------------------- read-long
def test_read_long_equals_correct_py(tmp_path):
    recs = [("r10", b"acgtRYacgt" * 30, None), ("r9", b"ACGT" * 80, b"#" * 320), ("r1", b"ACGT" * 10, None)]
    js = [[i, s.decode(), None if q is None else q.decode()] for i, s, q in recs]
    got = _helper("read_long", {"records": js, "stubby": 300}, tmp_path)
    reads, ign = correct.read_long(recs, 300)
    assert got["ids"] == reads.ids == ["r9", "r10"]
    assert got["ignored"] == ign == ["r1\tstubby"]
    assert [s.encode() for s in got["seqs"]] == reads.seqs and got["seqs"][1] == "ACGTNNACGT" * 30
    assert [q.encode() for q in got["quals"]] == reads.quals and got["quals"][1] == "$" * 300
    dup = _helper("read_long", {"records": [["a", "A" * 10, None], ["a", "C" * 10, None]], "stubby": 1}, tmp_path)
    assert "Non-unique long read id (a)" in dup["error"]
    # byfile order beyond one digit run, and ties in input order
    ids = ["m2/10/0_5", "m2/9/0_5", "m10/1", "m2/9/0_40", "x", "m2/9"]
    mixed = [(i, b"ACGT" * 3, None) for i in ids]
    got = _helper("read_long", {"records": [[i, s.decode(), None] for i, s, _ in mixed], "stubby": 1}, tmp_path)
    assert got["ids"] == correct.read_long(mixed, 1)[0].ids


# ---------------------------------------------------------------- final outputs
FILES = ("untrimmed.fq", "chim.tsv", "ignored.tsv", "trimmed.fq", "trimmed.fa")


def _result():
    rnd = random.Random(5)
    seq = lambda n: "".join(rnd.choice("ACGT") for _ in range(n))
    reads = [("cut", seq(2000), "I" * 2000),                                   # cut by a chimera line
             ("two", seq(1350), "I" * 600 + "!" * 50 + "I" * 700),             # two windows >= 500
             ("short", seq(650), "I" * 300 + "!" * 50 + "I" * 300),            # every piece < 500
             ("whole", seq(800), "I" * 800)]                                   # untouched
    # the first line of a read only opens it; the last read of the file is never written
    chim = ["cut\t900\t910\t0.5", "cut\t900\t910\t0.5", "cut\t1500\t1501\t0.001", "whole\t100\t200\t0.9"]
    return reads, chim, ["tiny\tstubby"]


@pytest.mark.parametrize("empty", [False, True])
def test_outputs_equal_write_outputs(empty, tmp_path):
    reads, chim, ign = ([], [], []) if empty else _result()
    ids = [r[0] for r in reads]
    res = correct.LoopResult(correct.LongReads(ids, [r[1].encode() for r in reads], [r[2].encode() for r in reads]),
                             chim, ign, [])
    correct.write_outputs(res, str(tmp_path / "py"))
    _helper("outputs", {"ids": ids, "seqs": [r[1] for r in reads], "quals": [r[2] for r in reads], "chim": chim,
                        "ignored": ign, "pre": str(tmp_path / "pl")}, tmp_path)
    for f in FILES:
        py, pl = tmp_path / f"py.{f}", tmp_path / f"pl.{f}"
        assert py.exists() == pl.exists(), f
        if py.exists():
            assert pl.read_bytes() == py.read_bytes(), f
    if empty:
        assert not (tmp_path / "pl.trimmed.fa").exists() and (tmp_path / "pl.trimmed.fq").read_bytes() == b""
        return
    assert (tmp_path / "pl.chim.tsv").read_text() == "cut\t0\t900\ncut\t910\n"
    heads = [ln[1:] for ln in (tmp_path / "pl.trimmed.fq").read_text().split("\n")[0::4] if ln]
    names = [h.split()[0] for h in heads]
    assert names == ["cut.1", "cut.2", "two.1", "two.2", "whole"]      # `short` is gone
    fa = (tmp_path / "pl.trimmed.fa").read_text()
    assert fa.count(">") == 5 and max(len(ln) for ln in fa.split("\n") if not ln.startswith(">")) == 80


# ---------------------------------------------------------------- the driver without a device
def test_driver_without_device_writes_nothing(tmp_path):
    (tmp_path / "lr.fq").write_text("@r\n%s\n+\n%s\n" % ("ACGT" * 100, "I" * 400))
    (tmp_path / "sr.fq").write_bytes(_fq([50] * 20))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")   # a child that sees no device, wherever this runs
    r = subprocess.run(["perl", str(DRIVER), "-l", str(tmp_path / "lr.fq"), "-s", str(tmp_path / "sr.fq"),
                        "-p", str(tmp_path / "out")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0
    assert "pr_ctx_create" in r.stderr and "no HIP device" in r.stderr
    assert not list(tmp_path.glob("out.*"))

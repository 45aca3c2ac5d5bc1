"""The on-chip chaining's mem_chain_flt (proovread_amd/csrc/seed_chain.h chain_read: the rank sort,
the -D pass over ballots with the kept list's first 64 entries in registers, the task bases as a
wave scan) compiled for the host (tests/native/seed_chain_dpass_host.cpp) on directed occurrence
lists -- every occurrence a chain of its own, with a chosen query interval and weight -- against a
plain statement of bwa's mem_chain_flt loop written in that file: the tasks array-equal and every
chain's kept value (0 / 1 / 2 / 3).

Reads of 1, 2, 63, 64, 65, 128, 129 and 512 chains (the first geometry's capacity) and of 1,536 (the
second's); kept lists past 64 and 128 entries; the dropping kept entry at kept index 0, 63, 64 and
65 with overlapping entries after it in its step of 64 and in a later step (which must not be
marked); chains shadowed twice; the four comparisons at equality and one off it; weight ties
decided by pos and by the stream index.  The plain statement counts each case and every count
must be non-zero.

One count must be zero: an overlapping kept entry *before* the dropping one.  The kept list is in
sorted order, so such an entry j has wj >= wk for the dropping entry k, and then wi < wk * D and
wk - wi >= 2 * min_seed_len hold for wj as well: entry j would have dropped the chain first.  The
dropping entry is always the first overlapping one."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "seed_chain_dpass_host.cpp"


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("seed_chain_dpass") / "libdpass.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", str(out), str(SRC)],
                   check=True)
    return C.CDLL(str(out))


@pytest.fixture(scope="module")
def result(lib):
    n = lib.dp_count_names(-1, None, 0)
    cnt, sizes = np.zeros(n, np.int64), np.zeros(8, np.int32)
    lib.dp_run.argtypes = [C.c_void_p, C.c_void_p]
    bad = lib.dp_run(cnt.ctypes.data, sizes.ctypes.data)
    names = []
    for k in range(n):
        buf = C.create_string_buffer(32)
        lib.dp_count_names(k, buf, 32)
        names.append(buf.value.decode())
    return bad, dict(zip(names, (int(v) for v in cnt))), [int(s) for s in sizes]


def test_tasks_and_kept_equal_the_plain_mem_chain_flt(result):
    bad, _, sizes = result
    assert bad == 0
    assert sizes == [1, 2, 63, 64, 65, 128, 129, 512]


def test_every_named_case_occurs(result):
    _, cnt, _ = result
    print(cnt)
    assert len(cnt) == 25
    for name, v in cnt.items():
        if name == "before":
            assert v == 0, cnt   # (cannot occur: the module's docstring)
        else:
            assert v > 0, (name, cnt)


def test_scan_ballot_and_broadcast_twins(lib):
    assert lib.dp_primitives() == 0


def test_sanitized_stand_alone_program(tmp_path):
    exe = tmp_path / "seed_chain_dpass_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-DSC_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", str(exe), str(SRC)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("ok")

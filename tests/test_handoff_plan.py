"""The hand-off's sort plan (proovread_amd/csrc/handoff_plan.h: which long reads sort in LDS and
which through HBM, runs, merge passes, scratch and LDS bytes, the 2^20 refusal), compiled for the
host (tests/native/handoff_plan_host.cpp) against a plain restatement."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
LDS_KEYS, MAX_ALNS = 16384, 1 << 20
OUTS = ("max_count", "sort_cap", "lds_bytes", "n_big", "big_keys", "max_big", "max_runs", "passes", "lds_big_bytes",
        "scratch_bytes", "refused_lr", "refused_count", "first")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("handoff_plan") / "libhandoff_plan_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", str(out),
                    str(ROOT / "tests" / "native" / "handoff_plan_host.cpp")], check=True)
    L = C.CDLL(str(out))
    L.handoff_plan_case.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.handoff_plan_case.restype = None
    L.handoff_max_alns.restype = C.c_int64
    assert L.handoff_out_count() == len(OUTS)
    assert (L.handoff_lds_keys(), L.handoff_max_alns(), L.handoff_merge_tile()) == (LDS_KEYS, MAX_ALNS, 2048)
    return L


def plan(lib, counts):
    a = np.array(counts, np.int64)
    o = np.zeros(len(OUTS), np.int64)
    bl, bo = np.full(len(a) + 1, -1, np.int32), np.full(len(a) + 2, -1, np.int64)
    lib.handoff_plan_case(a.ctypes.data, len(a), o.ctypes.data, bl.ctypes.data, bo.ctypes.data)
    p = dict(zip(OUTS, (int(v) for v in o)))
    p["big_lr"] = [int(v) for v in bl[:p["n_big"]]]
    p["big_off"] = [int(v) for v in bo[:p["n_big"] + 1]]
    assert (bl[p["n_big"]:] == -1).all() and (bo[p["n_big"] + 1:] == -1).all()
    return p


def ceil_log2(n):
    return 0 if n <= 1 else (n - 1).bit_length()


def restated(counts):
    """The plan in plain Python."""
    big = [(i, c) for i, c in enumerate(counts) if LDS_KEYS < c <= MAX_ALNS]
    small = [c for c in counts if c <= LDS_KEYS]
    over = [(i, c) for i, c in enumerate(counts) if c > MAX_ALNS]
    runs = [-(-c // LDS_KEYS) for _, c in big]
    first = counts[0] if counts else 0
    fr = -(-first // LDS_KEYS)
    return dict(max_count=max(counts, default=0), sort_cap=1 << ceil_log2(max(small, default=0)),
                lds_bytes=8 << ceil_log2(max(small, default=0)), n_big=len(big), big_keys=sum(c for _, c in big),
                max_big=max((c for _, c in big), default=0), max_runs=max(runs, default=0),
                passes=ceil_log2(max(runs, default=0)), lds_big_bytes=LDS_KEYS * 8 if big else 0,
                scratch_bytes=2 * 8 * sum(c for _, c in big), refused_lr=over[0][0] if over else -1,
                refused_count=over[0][1] if over else 0, first=(fr * 100 + ceil_log2(fr)) if counts else 0,
                big_lr=[i for i, _ in big], big_off=list(np.cumsum([0] + [c for _, c in big])))


SINGLE = [0, 1, 16384, 16385, 32768, 32769, 1 << 20, (1 << 20) + 1]
MIXED = [[], [5, 0, 70000, 16384, 16385, 3, 1 << 20, 40000], [20000, (1 << 20) + 1, 9, (1 << 20) + 7],
         [16384] * 3, [1000, 300, 17], [16385, 16385]]


@pytest.mark.parametrize("counts", [[c] for c in SINGLE] + MIXED, ids=lambda c: "-".join(map(str, c)) or "none")
def test_plan_equals_its_restatement(lib, counts):
    got, want = plan(lib, counts), restated(counts)
    assert got == want, {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert got["scratch_bytes"] == 2 * 8 * sum(counts[i] for i in got["big_lr"])
    assert got["lds_bytes"] <= 128 * 1024 and got["lds_big_bytes"] <= 128 * 1024


def test_thresholds(lib):
    """At the cap a read sorts in LDS with today's capacity; one more alignment is two runs and one
    merge pass; 2^20 is 64 runs and 6 passes; 2^20 + 1 is refused."""
    at, over = plan(lib, [16384]), plan(lib, [16385])
    assert (at["n_big"], at["sort_cap"], at["lds_bytes"], at["scratch_bytes"]) == (0, 16384, 128 * 1024, 0)
    assert (over["n_big"], over["max_runs"], over["passes"], over["sort_cap"]) == (1, 2, 1, 1)
    assert (plan(lib, [32768])["max_runs"], plan(lib, [32768])["passes"]) == (2, 1)
    assert (plan(lib, [32769])["max_runs"], plan(lib, [32769])["passes"]) == (3, 2)
    top = plan(lib, [1 << 20])
    assert (top["n_big"], top["max_runs"], top["passes"], top["refused_lr"]) == (1, 64, 6, -1)
    ref = plan(lib, [7, (1 << 20) + 1])
    assert (ref["refused_lr"], ref["refused_count"], ref["n_big"]) == (1, (1 << 20) + 1, 0)
    # the small reads' capacity does not follow the big ones
    assert plan(lib, [100, 50000])["sort_cap"] == 128

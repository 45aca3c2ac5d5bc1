"""seed_plan.h's newer decisions, compiled for the host (tests/native/seed_plan_batch_host.cpp):
pass 1b's batch size and waves for a lazy-table task (pass1b_batch), the budget of a chunk's
output slabs (out_budget) and pass 1's scratch budget at full occupancy (pass1_budget).  The
kernel lays `batch` slices per wave over the scratch, so pass1b_batch's result must stay inside
it whatever the inputs."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
GB = 1 << 30


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("seed_plan_batch") / "libseed_plan_batch_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", str(out),
                    str(ROOT / "tests" / "native" / "seed_plan_batch_host.cpp")], check=True)
    L = C.CDLL(str(out))
    L.batch_case.argtypes = [C.c_void_p, C.c_void_p]
    L.batch_case.restype = None
    L.out_budget_case.argtypes = [C.c_int64, C.c_int64]
    L.out_budget_case.restype = C.c_int64
    for f in (L.pass1_budget_case, L.scratch_budget_case):
        f.argtypes = [C.c_int64] * (3 if f is L.pass1_budget_case else 2)
        f.restype = C.c_int64
    return L


def batch(lib, n, waves, cap, sb, force=0):
    # wb as pass1b_run computes it (the waves at 64 reads each that the scratch holds)
    wb = min(cap // (64 * sb), (n + 63) // 64, waves)
    a, o = np.array([n, waves, cap, sb, wb, force], np.int64), np.zeros(2, np.int64)
    lib.batch_case(a.ctypes.data, o.ctypes.data)
    return int(o[0]), int(o[1]), wb


def test_batch_stays_inside_the_scratch_and_spreads_the_reads(lib):
    n_cases = 0
    for n, waves, cap, sb, force in itertools.product(
            [4097, 8320, 16384, 17821, 40000, 111151, 262144, 262145, 914286], [256, 375, 4096],
            [1 * GB, 3 * GB, 24 * GB, 40 * GB], [46_016, 75_000, 170_048, 1_500_032], [0, 1, 16, 63, 64, 1000]):
        b, w, wb = batch(lib, n, waves, cap, sb, force)
        if wb < 1:   # (pass1b_run skips the lane variant long before: it needs a wave per CU)
            continue
        n_cases += 1
        assert 1 <= b <= 64 and 1 <= w <= waves, (n, waves, cap, sb, force)
        assert w * b * sb <= cap, (n, waves, cap, sb, force)
        assert w <= (n + b - 1) // b
        if force:
            assert b == min(force, 64) or (b, w) == (64, wb)
        elif w * b >= n:   # one dequeue per wave: no wave takes more reads than an even share needs
            assert b == min(64, -(-n // waves))
    assert n_cases > 1000
    # configs[1]-like: a few ten thousand flagged reads over all of pass 1's waves, not a few hundred
    assert batch(lib, 40000, 4096, 30 * GB, 75_000)[:2] == (10, 4000)
    assert batch(lib, 40000, 4096, 30 * GB, 75_000, force=64)[:2] == (64, 625)
    # more reads than 64 a wave: pass 1's own shape
    assert batch(lib, 914286, 4096, 40 * GB, 75_000)[:2] == (64, 4096)


def test_out_budget_is_a_tenth_of_the_free_memory_between_8_and_16_gb(lib):
    assert lib.out_budget_case(20 * GB, 0) == 8 * GB
    assert lib.out_budget_case(100 * GB, 0) == 10 * GB
    assert lib.out_budget_case(92 * GB, 8 * GB) == 10 * GB
    assert lib.out_budget_case(250 * GB, 0) == 16 * GB
    # configs[1]'s finish task (914,286 reads x 384 slots x 40 bytes) is one chunk on a free MI355X
    assert 914_286 * 384 * 40 <= lib.out_budget_case(250 * GB, 0)


def test_pass1_budget_holds_every_resident_wave_where_a_quarter_of_the_memory_allows(lib):
    full = 4096 * 64 * 104_000   # configs[1]: 16 waves per CU x 64 slices of ~100 KB, 27.3 GB
    for free, have in itertools.product([10 * GB, 60 * GB, 100 * GB, 130 * GB, 150 * GB, 200 * GB, 280 * GB],
                                        [0, 24 * GB, 28 * GB]):
        base = lib.scratch_budget_case(free, have)
        got = lib.pass1_budget_case(free, have, full)
        assert got == (full if base < full <= (free + have) // 4 else base), (free, have)
        assert lib.pass1_budget_case(free, have, 8 * GB) == base        # fits the budget anyway
        assert lib.pass1_budget_case(free, have, 41 * GB) == base       # beyond the ceiling: as before
    # inside the loop: ~150 GB free, 15 % of it under the 24 GB floor -> the full 27.3 GB
    assert lib.scratch_budget_case(126 * GB, 24 * GB) == 24 * GB
    assert lib.pass1_budget_case(126 * GB, 24 * GB, full) == full
    # a crowded device keeps the floor
    assert lib.pass1_budget_case(60 * GB, 24 * GB, full) == 24 * GB

"""The device seeding driver's planning (proovread_amd/csrc/seed_plan.h: scratch budget, pass 1's
waves, output chunk, pass 1b's capacities and lane / wave / skip decision) and seed_core.h's
grow_caps, compiled for the host (tests/native/seed_plan_host.cpp) next to the inline arithmetic
they replaced, which that file keeps verbatim as parent_* functions.

Everything is equal over the sweep, with one deliberate exception asserted on its own: pass 1b
no longer grows its scratch to more than half of the memory then free; it goes on with the
buffer it has."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
GB = 1 << 30
LEN, HITS, IV, MEMS, SEEDS, CHAINS, OUT = 1, 2, 4, 8, 16, 32, 64
IN = ("qlen", "lazy", "flags", "n_flagged", "need_max", "need_sum", "need_n", "free", "have", "n_cu", "wpc", "balance",
      "n_sr", "lanes2", "force", "out_budget")
CAPS = ("lmax", "hits", "iv", "mems", "seeds", "chains", "out", "hi", "nopos", "lazy")
OUTS = (("budget", "wmax", "waves", "chunk") + tuple("cb." + k for k in CAPS) + tuple("cw." + k for k in CAPS)
        + ("want", "cap", "wb", "ww", "by_wave", "mode"))
SKIP, LANE, WAVE = 0, 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("seed_plan") / "libseed_plan_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", str(out),
                    str(ROOT / "tests" / "native" / "seed_plan_host.cpp")], check=True)
    L = C.CDLL(str(out))
    L.plan_case.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.plan_case.restype = None
    L.flagged_case.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.flagged_case.restype = None
    L.grow_case.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int, C.c_void_p]
    L.grow_case.restype = None
    assert L.plan_in_count() == len(IN) and L.plan_out_count() == len(OUTS)
    return L


def plan(lib, case: dict, which: int, keep_scratch: bool = False) -> dict:
    a = np.array([case[k] for k in IN], np.int64)
    o = np.zeros(len(OUTS), np.int64)
    lib.plan_case(a.ctypes.data, which, int(keep_scratch), o.ctypes.data)
    return dict(zip(OUTS, (int(v) for v in o)))


def small_hits(qlen: int) -> int:
    l = max(16, (qlen + 15) & ~15)
    return max(4096, 24 * l) if l > 160 else 4096


def sweep():
    flags = [0, LEN, HITS, IV, MEMS, SEEDS, CHAINS, OUT, HITS | MEMS, HITS | CHAINS, IV | SEEDS, HITS | LEN, MEMS | OUT,
             HITS | IV | MEMS | SEEDS | CHAINS]
    # free memory: the budget at its 24 GB floor, between the bounds, at its 40 GB ceiling; and a
    # crowded device, where the floor lies above half of what is free
    frees = [100 * GB, 200 * GB, 280 * GB, 30 * GB, 10 * GB]
    for qlen, lazy, fl, n_fl, need, free, have, force, (n_sr, balance) in itertools.product(
            [100, 150, 600, 950], [0, 1], flags, [4096, 4097, 23400], ["low", "under", "over"], frees, [0, 2 * GB, 30 * GB],
            [0, 1, 2], [(6000, 0), (24000, 0), (460000, 0), (460000, 1), (300000, 1)]):
        if n_fl > n_sr or (need != "low" and not fl & HITS):   # (no hit table overflowed: no need recorded)
            continue
        h = small_hits(qlen)
        need_max = {"low": h + 100, "under": 4 * h - 1, "over": 4 * h + 1}[need]
        # (the mean of the needs just under / over 4x pass 1's hits: by lane / by wave)
        need_n = n_fl if fl & HITS else 0
        yield dict(qlen=qlen, lazy=lazy, flags=fl, n_flagged=n_fl, need_max=need_max if need_n else 0,
                   need_sum=need_max * need_n, need_n=need_n, free=free, have=have, n_cu=256, wpc=16, balance=balance,
                   n_sr=n_sr, lanes2=256 * 8, force=force, out_budget=8192 << 20)


def test_plan_equals_the_inline_arithmetic_it_replaced(lib):
    n = n_kept = 0
    modes, grown, budgets = set(), 0, set()
    for case in sweep():
        want, got = plan(lib, case, 0), plan(lib, case, 1)
        n += 1
        if want["want"] and want["want"] > (case["free"] + case["have"]) // 2:
            # the one deliberate change: no growth beyond half of the free memory; the wave counts
            # and the decision are the parent's for the buffer as it is
            n_kept += 1
            assert got["want"] == 0 and got["cap"] == case["have"], case
            want = plan(lib, case, 0, keep_scratch=True)
            want["want"] = 0
        assert got == want, (case, {k: (want[k], got[k]) for k in OUTS if want[k] != got[k]})
        if case["flags"] & (LEN | OUT) or case["n_flagged"] <= 4096:
            assert got["mode"] == SKIP, case
        modes.add(got["mode"])
        grown += got["want"] != 0
        budgets.add(got["budget"])
    assert n > 50_000 and n_kept > 100 and grown > 1000
    assert modes == {SKIP, LANE, WAVE}
    assert {24 * GB, 40 * GB} < budgets


def test_pass1b_mode_follows_the_need_and_the_override(lib):
    base = dict(qlen=150, lazy=0, flags=HITS, n_flagged=23400, need_n=23400, free=200 * GB, have=30 * GB, n_cu=256, wpc=16,
                balance=0, n_sr=24000, lanes2=256 * 8, force=0, out_budget=8192 << 20)
    under = dict(base, need_max=4 * 4096 - 1, need_sum=(4 * 4096 - 1) * 23400)
    over = dict(base, need_max=4 * 4096 + 1, need_sum=(4 * 4096 + 1) * 23400)
    assert plan(lib, under, 1)["mode"] == LANE and plan(lib, over, 1)["mode"] == WAVE
    assert plan(lib, dict(under, force=2), 1)["mode"] == WAVE and plan(lib, dict(over, force=1), 1)["mode"] == LANE
    # 4,096 flagged reads are pass 2's; the lane variant needs a wave of 64 reads per CU
    assert plan(lib, dict(over, n_flagged=4096, need_n=4096), 1)["mode"] == SKIP
    assert plan(lib, dict(under, n_flagged=256 * 64 - 64, force=1), 1)["mode"] == SKIP
    assert plan(lib, dict(under, n_flagged=256 * 64 - 63, force=1), 1)["mode"] == LANE


def test_flagged_summary_equals_the_inline_loop(lib):
    rng = np.random.default_rng(5)
    for n in (0, 1, 64, 5000):
        st = (rng.integers(0, 128, n) * (rng.random(n) < 0.4)).astype(np.int32)
        no = rng.integers(-40000, 400, n).astype(np.int32)
        a, b = np.zeros(5, np.int64), np.zeros(5, np.int64)
        lib.flagged_case(st.ctypes.data, no.ctypes.data, n, 0, a.ctypes.data)
        lib.flagged_case(st.ctypes.data, no.ctypes.data, n, 1, b.ctypes.data)
        assert np.array_equal(a, b)
        assert n < 64 or a[0] > 0


def test_grow_caps_equals_the_three_rules_it_replaced(lib):
    def grow(qlen, small, flags, which):
        o = np.zeros(10, np.int64)
        lib.grow_case(qlen, small, flags, which, o.ctypes.data)
        return dict(zip(CAPS, (int(v) for v in o)))
    changed = 0
    for qlen, small, flags in itertools.product([100, 150, 600, 950], [0, 1], range(128)):
        base = grow(qlen, small, 0, 4)
        assert grow(qlen, small, flags, 3) == grow(qlen, small, flags, 0)   # pass 1b (hits sized before)
        later = grow(qlen, small, flags, 4)
        assert later == grow(qlen, small, flags, 1) == grow(qlen, small, flags, 2)   # later passes, host emulation
        for k, bit, f in (("hits", HITS, 4), ("iv", IV, 2), ("mems", MEMS, 2), ("seeds", SEEDS, 2), ("chains", CHAINS, 2)):
            assert later[k] == base[k] * (f if flags & bit else 1)
        assert all(later[k] == base[k] for k in ("lmax", "out", "hi", "nopos", "lazy"))
        changed += later != base
    assert changed > 900

"""The on-chip chaining's HIP-free core (proovread_amd/csrc/seed_chain.h: emit_occ + chain_read,
the wave's lanes one after the other) compiled for the host (tests/native/seed_chain_host.cpp)
against seed_core.h's map_after_occ on the same reads: the tasks array-equal -- order, rank,
chain, rmax0 / rmax1 -- and the SC_OVER_* flags, for the bwa-sr and the finish (-D 0.75) options
and -c 20 (every 3rd occurrence of an SMEM), with the scratch and the LDS image poisoned.

Capacities: the reads of seed_chain_cases sit at cap - 1, cap and cap + 1 of a geometry's seeds
and of its ranges; the cap + 1 read leaves it with the matching flag and comes back through the
next geometry (or the old path) with the same tasks, and its neighbours are exact.  A small
geometry (64 seeds, 32 ranges) and the kernel's two are checked that way."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import seed_chain_cases as cases
from proovread_amd.seed import SeedOpts

ROOT = Path(__file__).resolve().parents[1]
SC_OVER_SEEDS, SC_OVER_CHAINS = 16, 32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("seed_chain") / "libseedchain.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-pthread", "-o", str(out),
                    str(ROOT / "proovread_amd" / "csrc" / "seed.cpp"),
                    str(ROOT / "tests" / "native" / "seed_chain_host.cpp")], check=True)
    L = C.CDLL(str(out))
    L.pr_seed_opts_default.argtypes = [C.POINTER(SeedOpts), C.c_int]
    L.pr_seed_index_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.pr_seed_index_free.argtypes = [C.c_void_p]
    L.sc_chain_compare.argtypes = [C.c_void_p, C.POINTER(SeedOpts), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_void_p]
    return L


def geometry(lib):
    g = (C.c_int32 * 9)()
    lib.sc_chain_geometry(g)
    return list(g)


def opts(lib, which):
    o = SeedOpts()
    lib.pr_seed_opts_default(C.byref(o), 1 if which == "finish" else 0)
    if which == "finish":
        assert o.drop_ratio == 0.75
    if which == "c20":
        o.max_occ = 20
    return o


def compare(lib, data, o, geom, fill=0xA5):
    lr_seq, lr_off, sr_seq, sr_off, _ = data
    h = C.c_void_p()
    lr_seq, lr_off = np.ascontiguousarray(lr_seq, np.uint8), np.ascontiguousarray(lr_off, np.int64)
    assert lib.pr_seed_index_build(lr_seq.ctypes.data, lr_off.ctypes.data, len(lr_off) - 1, C.byref(h)) == 0
    n = len(sr_off) - 1
    res = np.zeros((n, 16), np.int32)
    sr_seq, sr_off = np.ascontiguousarray(sr_seq, np.uint8), np.ascontiguousarray(sr_off, np.int64)
    lib.sc_chain_compare(h, C.byref(o), sr_seq.ctypes.data, sr_off.ctypes.data, n, geom, 0, fill, res.ctypes.data)
    lib.pr_seed_index_free(h)
    return res


@pytest.fixture(scope="module")
def tiny_data():
    return cases.build([(64, 32)])   # (>= 20 occurrences: the -y round adds no shorter seeds)


@pytest.fixture(scope="module")
def kernel_data(lib):
    g = geometry(lib)
    return cases.build([(g[0], g[1]), (g[3], g[4])])


def check_edges(res, labels, ci, seeds_cap, ranges_cap, which):
    """the reads at the capacities: counts as built, the flag exactly beyond the capacity"""
    for k in (-1, 0, 1):
        s, r = res[labels[f"seeds{k:+d}.{ci}"]], res[labels[f"ranges{k:+d}.{ci}"]]
        if which != "c20":   # (-c 20 takes 20 of an SMEM's occurrences)
            assert s[0] == seeds_cap + k, (which, k, s)
            assert (s[2] == SC_OVER_SEEDS) == (k > 0) and s[2] in (0, SC_OVER_SEEDS), (which, k, s)
            if k <= 0:
                assert s[7] == seeds_cap + k
            assert (r[2] == SC_OVER_CHAINS) == (k > 0) and r[2] in (0, SC_OVER_CHAINS), (which, k, r)
            if k <= 0:
                assert r[1] == ranges_cap + k
        assert s[3] == 0 and r[3] == 0 and s[5] == 1 and r[5] == 1   # exact through the next geometry or the old path


@pytest.mark.parametrize("which", ["bwa-sr", "finish", "c20"])
def test_small_geometry_equals_map_after_occ_at_every_edge(lib, tiny_data, which):
    labels = tiny_data[4]
    res = compare(lib, tiny_data, opts(lib, which), 1)
    assert res[:, 5].all(), np.nonzero(res[:, 5] == 0)[0][:5]
    check_edges(res, labels, 0, 64, 32, which)
    # both ways out of the geometry were taken and most reads stayed in it
    assert (res[:, 2] == 0).sum() > 50
    if which == "bwa-sr":
        assert (res[:, 1] > 64).sum() == 0 and res[:, 4].sum() > 1000
        assert res[labels["mr_length"], 0] == 0 and res[labels["mr_length"], 4] > 0   # routed to the lane path
        for name in ("short", "short11", "no_smem", "empty", "all_n"):
            assert res[labels[name], 4] == 0 and res[labels[name], 5] == 1
        assert res[labels["equal_pos"], 6] >= 2   # two chains at one pos
        assert res[labels["seeds+0.0"], 1] == 1   # one range holds every occurrence
        assert res[labels["n_inside"], 4] > 0


@pytest.mark.parametrize("which", ["bwa-sr", "finish", "c20"])
def test_kernel_geometries_equal_map_after_occ_at_every_edge(lib, kernel_data, which):
    g = geometry(lib)
    labels = kernel_data[4]
    o = opts(lib, which)
    res = compare(lib, kernel_data, o, 0)   # the kernel's first geometry, then its second
    assert res[:, 5].all(), np.nonzero(res[:, 5] == 0)[0][:5]
    check_edges(res, labels, 0, g[0], g[1], which)
    # more than 64 ranges in one read (several ranges to a lane), one range with every occurrence
    if which != "c20":
        assert res[labels["ranges+0.0"], 1] > 64
    # the second geometry's edges: `tiny` first, so that the read reaches it (geom 2 = tiny, second)
    res2 = compare(lib, kernel_data, o, 2)
    assert res2[:, 5].all()
    res3 = compare(lib, kernel_data, o, 3)   # (the counts themselves, from a geometry nothing leaves)
    for k in (-1, 0, 1):
        if which != "c20":
            assert res3[labels[f"seeds{k:+d}.1"], 7] == g[3] + k
            assert res3[labels[f"ranges{k:+d}.1"], 1] == g[4] + k


@pytest.mark.parametrize("which", ["bwa-sr", "finish"])
def test_named_cases_occur_in_the_case_sets(lib, tiny_data, kernel_data, which):
    """The cases the comparison rests on are there, counted by the host build (seed_chain.h SCC_STAT):
    both case sets (the GPU test maps the kernel set), a geometry nothing leaves."""
    o = opts(lib, which)
    for data in (tiny_data, kernel_data):
        labels = data[4]
        res = compare(lib, data, o, 3)
        assert res[:, 5].all() and not res[:, 2].any()
        # two chains of one range, equal pos and equal weight: creation order alone decides
        t = res[labels["equal_pos"]]
        assert t[8] >= 2 and t[6] == 2 and t[4] > 0, t
        # a chain whose reference cover is below its query cover, and a chain that the smaller
        # cover puts behind
        w = res[labels["wr_lt"]]
        assert w[12] >= 1 and w[6] >= 2, w
        # chains opened before the head, between two chains and after the tail of their range
        assert res[:, 9].sum() > 0 and res[:, 10].sum() > 0 and res[:, 11].sum() > 0, res[:, 9:12].sum(0)
        if which == "finish":   # -D 0.75: chains dropped, kept though shadowing (1) and shadowed (2)
            assert res[:, 13].sum() > 0 and res[:, 14].sum() > 0 and res[:, 15].sum() > 0, res[:, 13:16].sum(0)


def test_most_occurrences_a_read_may_hand_over(lib, tiny_data):
    """OCC_MAX - 1 and OCC_MAX occurrences are chained (one chain, one task), OCC_MAX + 1 flagged"""
    h = C.c_void_p()
    lr_seq, lr_off = np.ascontiguousarray(tiny_data[0], np.uint8), np.ascontiguousarray(tiny_data[1], np.int64)
    assert lib.pr_seed_index_build(lr_seq.ctypes.data, lr_off.ctypes.data, len(lr_off) - 1, C.byref(h)) == 0
    out = (C.c_int32 * 6)()
    o = opts(lib, "bwa-sr")
    lib.sc_occ_max_edge.argtypes = [C.c_void_p, C.POINTER(SeedOpts), C.c_void_p]
    lib.sc_occ_max_edge(h, C.byref(o), out)
    lib.pr_seed_index_free(h)
    assert geometry(lib)[8] == 16384
    assert list(out) == [0, 1, 0, 1, SC_OVER_SEEDS, 0]


def test_result_does_not_depend_on_what_the_lds_held(lib, tiny_data):
    o = opts(lib, "finish")
    a, b = compare(lib, tiny_data, o, 1, fill=0x00), compare(lib, tiny_data, o, 1, fill=0xFF)
    assert np.array_equal(a, b) and a[:, 5].all()


def test_sanitized_stand_alone_program(tmp_path):
    """the same core in a stand-alone program (its own main) under ASan + UBSan: random reads,
    both option sets, every geometry"""
    exe = tmp_path / "seed_chain_asan"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-DSC_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-pthread", "-o", str(exe),
                    str(ROOT / "proovread_amd" / "csrc" / "seed.cpp"),
                    str(ROOT / "tests" / "native" / "seed_chain_host.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("ok")

"""Work counters of the seeding core on a bench-shaped sample (host-only statistics build:
seed.cpp with -DPR_SEED_STATS, tools/seed_stats.cpp).  Prints per-read averages of the
SC_STAT counters in seed_core.h.

    g++ -O2 -std=c++17 -fPIC -shared -pthread -DPR_SEED_STATS -o /tmp/libseedstats.so \
        proovread_amd/csrc/seed.cpp tools/seed_stats.cpp
    python tools/seed_stats.py /tmp/libseedstats.so [n_reads]

--dist: the per-read distribution (quantiles to 99.9 % and the maximum) of what the on-chip
chaining (seed_chain.h) has to hold -- occurrences handed over, ranges, chains, seeds, tasks --
and the share of reads beyond seed_chain_kernel's first geometry and beyond both (under pass 1's
capacities), from the host build of that code (its source is the test suite's native harness):

    g++ -O2 -std=c++17 -fPIC -shared -pthread -o /tmp/libseedchain.so \
        proovread_amd/csrc/seed.cpp tests/native/seed_chain_host.cpp
    python tools/seed_stats.py --dist /tmp/libseedchain.so [n_reads]

Three cases on the bench generator's reads: bwa-sr options on the raw long reads; the same with
70 % of every long read masked (N in 140 of every 200 bases: the iterations mask what they
corrected and keep islands); the finish options on long reads with 0.5 % residual error at twice
the short-read sample (a stand-in for the corrected reads of the loop).
"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from proovread_amd import synth  # noqa: E402
from proovread_amd.seed import SeedOpts, SeedTasks  # noqa: E402

NAMES = {0: "reads", 1: "mems", 2: "hits scanned (chaining)", 3: "occurrences chained", 4: "chain-search steps",
         5: "merges", 6: "new chains", 7: "shifted list elements", 8: "occ() lookups", 9: "occ() hit-list scans",
         10: "hit-list entries scanned", 11: "chains (ncv)", 12: "sum ncv^2", 13: "weight-sort moves",
         14: "chains after weight filter", 15: "tasks out", 16: "smem1 calls", 17: "backward intervals"}
QS = (0.5, 0.9, 0.99, 0.999)


def dist(lib_path: str, n: int) -> None:
    L = C.CDLL(lib_path)
    L.pr_seed_opts_default.argtypes = [C.POINTER(SeedOpts), C.c_int]
    L.pr_seed_index_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.pr_seed_index_free.argtypes = [C.c_void_p]
    L.sc_chain_compare.argtypes = [C.c_void_p, C.POINTER(SeedOpts), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_void_p]
    geo = (C.c_int32 * 9)()
    L.sc_chain_geometry(geo)
    print(f"first geometry: {geo[0]} seeds, {geo[1]} ranges, {geo[2]} bytes of LDS; second: {geo[3]} seeds, "
          f"{geo[4]} ranges, {geo[5]} bytes; a read hands over at most {geo[8]} occurrences")
    raw = synth.simulate(20261015 + 2, 4_600_000, 13_800, 10_000, 50.0, sr_frac=0.3)
    fin = synth.simulate(20261015 + 2, 4_600_000, 13_800, 10_000, 50.0, p_ins=0.002, p_del=0.002, p_sub=0.001,
                         sr_frac=0.6)
    masked = np.ascontiguousarray(raw.lr_seq, np.uint8).copy()
    for i in range(raw.n_lr):
        v = masked[raw.lr_off[i]:raw.lr_off[i + 1]]
        v[(np.arange(len(v)) % 200) < 140] = 4
    for name, d, lr, finish in (("bwa-sr, raw long reads", raw, raw.lr_seq, 0), ("bwa-sr, 70 % masked", raw, masked, 0),
                                ("finish, corrected long reads", fin, fin.lr_seq, 1)):
        seq = np.ascontiguousarray(lr, np.uint8)
        off = np.ascontiguousarray(d.lr_off, np.int64)
        h = C.c_void_p()
        assert L.pr_seed_index_build(seq.ctypes.data, off.ctypes.data, len(off) - 1, C.byref(h)) == 0
        o = SeedOpts()
        L.pr_seed_opts_default(C.byref(o), finish)
        m = min(n, d.n_sr)
        sr = np.ascontiguousarray(d.sr_seq[:d.sr_off[m]], np.uint8)
        so = np.ascontiguousarray(d.sr_off[:m + 1], np.int64)
        res = np.zeros((m, 16), np.int32)
        t = time.perf_counter()
        # the distribution from a geometry nothing leaves
        L.sc_chain_compare(h, C.byref(o), sr.ctypes.data, so.ctypes.data, m, 3, 0, 0, res.ctypes.data)
        L.pr_seed_index_free(h)
        # pass 1's capacities at 150 bp (seed_core.h device_caps_small) hold in the kernel as well
        P1_SEEDS, P1_CHAINS = 512, 384
        first = (res[:, 7] > geo[0]) | (res[:, 1] > geo[1])
        both = (res[:, 7] > min(geo[3], P1_SEEDS)) | (res[:, 6] > P1_CHAINS) | (res[:, 1] > geo[4]) | (res[:, 0] > geo[8])
        print(f"\n{name}: {m} reads, {time.perf_counter() - t:.1f} s; equal to map_read: {int(res[:, 5].sum())}; "
              f"beyond the first geometry: {int(first.sum())} ({100.0 * first.mean():.3f} %); beyond both under pass 1's "
              f"{P1_SEEDS} seeds / {P1_CHAINS} chains (to the later passes): {int(both.sum())} ({100.0 * both.mean():.3f} %)")
        print(f"{'per read':14s} {'mean':>8s} " + " ".join(f"{'q' + str(q):>8s}" for q in QS) + f" {'max':>8s}")
        ok = res[:, 2] == 0
        for col, label, rows in ((0, "occurrences", slice(None)), (1, "ranges", ok), (6, "chains", ok), (7, "seeds", ok),
                                 (4, "tasks", res[:, 3] == 0)):
            v = res[rows, col]
            print(f"{label:14s} {v.mean():8.1f} " + " ".join(f"{int(np.quantile(v, q)):8d}" for q in QS) + f" {int(v.max()):8d}")


if len(sys.argv) > 1 and sys.argv[1] == "--dist":
    dist(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 20000)
    sys.exit(0)

L = C.CDLL(sys.argv[1])
n = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
L.pr_seed_opts_default.argtypes = [C.POINTER(SeedOpts), C.c_int]
L.pr_seed_index_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
L.pr_seed_map.argtypes = [C.c_void_p, C.POINTER(SeedOpts), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                          C.POINTER(SeedTasks)]
d = synth.simulate(20261015 + 2, 4_600_000, 13_800, 10_000, 50.0, sr_frac=0.3)
seq = np.ascontiguousarray(d.lr_seq, np.uint8)
off = np.ascontiguousarray(d.lr_off, np.int64)
h = C.c_void_p()
assert L.pr_seed_index_build(seq.ctypes.data, off.ctypes.data, len(off) - 1, C.byref(h)) == 0
o = SeedOpts()
L.pr_seed_opts_default(C.byref(o), 0)
L.pr_seed_stat_reset()
sr = np.ascontiguousarray(d.sr_seq[:d.sr_off[n]], np.uint8)
so = np.ascontiguousarray(d.sr_off[:n + 1], np.int64)
out = SeedTasks()
t = time.perf_counter()
assert L.pr_seed_map(h, C.byref(o), sr.ctypes.data, so.ctypes.data, n, 8, C.byref(out)) == 0
dt = time.perf_counter() - t
st = (C.c_ulonglong * 24)()
L.pr_seed_stat_get(st)
r = max(1, st[0])
print(f"{n} reads, {dt:.2f} s on 8 threads (stats build)")
for k, name in NAMES.items():
    print(f"{k:2d} {name:28s} {st[k] / r:12.2f} per read")

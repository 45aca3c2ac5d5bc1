"""The lane phase's dropped accesses (seed_core.h: the range table reused from read to read
instead of cleared per read, mem_chain_flt without the kept-list scan at -D 0, the chain weight
in one walk) change no seed: the host path and the host run of the device path
(pr_seed_map_device_caps, which runs the range-table reuse) against the pure-Python oracle
(oracle/seed_oracle.py), seed for seed, for the bwa-sr and bwa-sr-finish option sets and one
set with -D 0.5; and the range table's reuse on one thread across a read that overflows the
chain capacity.  The reads also hold the edges of the two variants that were measured and not
kept (the read's N test from a 192-bit register mask, the SMEM rounds' final order
as a merge): N bases at the 64-bit word edges, read lengths 11 / 12 and 192 / 193, intervals of
all three rounds with one start."""
import sys
from pathlib import Path

import numpy as np
import pytest

from proovread_amd import seed

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
import seed_oracle as so  # noqa: E402

N = 4


def _cat(seqs):
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    return np.concatenate([np.asarray(x, np.uint8) for x in seqs]), off


def _rc(r):
    return [3 - x if x < 4 else 4 for x in reversed(r)]


def special_reads(G, R, rng):
    """(name, read): N bases at base 0, the last base and the 64-base word edges, read lengths at
    the 12-mer index's edge and at 192 / 193, the repeat R (overlapping chains, equal starts over
    the rounds), 600-base reads."""
    out = []
    base = [int(x) for x in G[500:692]]   # 192 bases

    def with_n(pos):
        r = list(base)
        for p in pos:
            r[p] = N
        return r
    for p in (0, 191, 63, 64, 127, 128):
        out.append((f"N@{p}", with_n([p])))
    out.append(("N@63,64,127,128,191", with_n([63, 64, 127, 128, 191])))
    out.append(("Nrun60-68", with_n(range(60, 69))))
    out.append(("Nrun124-131", with_n(range(124, 132))))
    out.append(("allN", [N] * 150))
    r150 = [int(x) for x in G[900:1050]]
    out.append(("N@last150", r150[:-1] + [N]))
    out.append(("N@0,last150", [N] + r150[1:-1] + [N]))
    for n in (11, 12, 13, 192, 193):
        out.append((f"len{n}", [int(x) for x in G[1500:1500 + n]]))
    out.append(("len600", [int(x) for x in G[2000:2600]]))
    out.append(("len600N", [int(x) if k not in (70, 200, 599) else N for k, x in enumerate(G[2100:2700])]))
    out.append(("repeat", [int(x) for x in R]))
    out.append(("repeat_rc", _rc([int(x) for x in R])))
    out.append(("repeat+N", [int(x) if k != 120 else N for k, x in enumerate(R)]))
    for k in range(6):   # ordinary reads with a substitution or two, either strand
        s0 = int(rng.integers(0, len(G) - 150))
        r = [int(x) for x in G[s0:s0 + 150]]
        r[int(rng.integers(0, 150))] = int(rng.integers(0, 4))
        out.append((f"ord{k}", _rc(r) if k % 2 else r))
    return out


@pytest.fixture(scope="module")
def case():
    """Long reads over a 4 kb genome with substitutions, and three that share the 150-base
    repeat R: A all of it, B its first 100 bases, C its first 40 -- the read R has three chains
    that overlap on the query with weights ~150 / ~100 / ~40 (-D 0.5 drops C's: 40 < 75 and
    150 - 40 >= 2 k; -D 0 keeps all), and intervals of all three rounds that start at base 0
    (the SMEM [0, 150), the re-seeded [0, 100) with two occurrences, the -y seed [0, 13))."""
    rng = np.random.default_rng(20261020)
    G = rng.integers(0, 4, 4000)
    R = rng.integers(0, 4, 150)
    lrs = []
    for i in range(5):
        s0 = int(rng.integers(0, 2800))
        lr = [int(x) for x in G[s0:s0 + 1200]]
        for j in rng.integers(0, len(lr), 30):
            lr[int(j)] = int(rng.integers(0, 4))
        if i == 2:
            lr[77] = N
        lrs.append(lr)
    lrs.append([int(x) for x in G[400:1700]])    # exact copies: the N and length reads' source
    lrs.append([int(x) for x in G[1900:2800]])
    for n in (150, 100, 40):   # A, B, C
        lrs.append([int(x) for x in rng.integers(0, 4, 300)] + [int(x) for x in R[:n]] +
                   [int(x) for x in rng.integers(0, 4, 300)])
    reads = special_reads(G, R, rng)
    lr_seq, lr_off = _cat(lrs)
    sr_seq, sr_off = _cat([r for _, r in reads])
    ix = seed.SeedIndex(lr_seq, lr_off)
    yield {"oidx": so.Index(lrs), "ix": ix, "names": [n for n, _ in reads], "reads": [r for _, r in reads],
           "sr_seq": sr_seq, "sr_off": sr_off, "n_lr": len(lrs)}
    ix.close()


def _opts(name):
    if name == "bwa-sr":
        return seed.default_opts(False), so.Opts()
    if name == "bwa-sr-finish":
        return seed.default_opts(True), so.Opts.finish()
    o = seed.default_opts(False)
    o.drop_ratio = 0.5
    return o, so.Opts(drop_ratio=0.5)


def _tuples(tasks):
    return [tuple(int(t[k]) for k in seed.TASK_DTYPE.names) for t in tasks]


@pytest.fixture(scope="module")
def oracle_tasks(case):
    """The oracle's seeds per option set and read, computed once."""
    out = {}
    for name in ("bwa-sr", "bwa-sr-finish", "drop0.5"):
        oo = _opts(name)[1]
        out[name] = [[tuple(t[k] for k in seed.TASK_DTYPE.names) for t in so.map_read(case["oidx"], oo, r, i)]
                     for i, r in enumerate(case["reads"])]
    return out


@pytest.mark.parametrize("name", ["bwa-sr", "bwa-sr-finish", "drop0.5"])
def test_host_and_device_caps_equal_oracle(case, oracle_tasks, name):
    o = _opts(name)[0]
    want = [t for per in oracle_tasks[name] for t in per]
    host = _tuples(case["ix"].map(case["sr_seq"], case["sr_off"], o, threads=2))
    n = len(case["reads"])
    by = [[t for t in host if t[0] == i] for i in range(n)]
    bad = [case["names"][i] for i in range(n) if by[i] != oracle_tasks[name][i]]
    assert not bad, bad
    assert host == want
    for threads in (1, 3):
        dev, st = case["ix"].map_device_caps(case["sr_seq"], case["sr_off"], o, threads=threads)
        assert not st.any(), [case["names"][i] for i in np.nonzero(st)[0]]
        assert _tuples(dev) == want
    seeded = {t[0] for t in want}
    assert case["names"].index("allN") not in seeded and case["names"].index("len11") not in seeded
    assert case["names"].index("len193") in seeded and case["names"].index("len600N") in seeded


def test_drop_shortcut_only_where_exact(case, oracle_tasks):
    """The read R: chains on A, B and C at -D 0, C's dropped at -D 0.5 (B's weight stays above
    half of A's) -- the shortcut that keeps every chain is taken only where no chain can drop."""
    i = case["names"].index("repeat")
    a, b, c = case["n_lr"] - 3, case["n_lr"] - 2, case["n_lr"] - 1
    keep_all = {t[1] for t in oracle_tasks["bwa-sr"][i]}
    dropped = {t[1] for t in oracle_tasks["drop0.5"][i]}
    assert {a, b, c} <= keep_all and len({t[8] for t in oracle_tasks["bwa-sr"][i]}) >= 3
    assert {a, b} <= dropped and c not in dropped


def test_equal_starts_across_rounds(case):
    """At least one read of the set has intervals of all three rounds with one start (the final
    order's ties: round order, then by end)."""
    oidx, O = case["oidx"], so.Opts()
    found = []
    for name, q in zip(case["names"], case["reads"]):
        if len(q) > 200:
            continue
        n, x, r1 = len(q), 0, []
        while x < n:
            if q[x] < 4:
                m1, x = so.smem1(oidx, q, x, 1)
                r1 += [m for m in m1 if m[1] - m[0] >= O.min_seed_len]
            else:
                x += 1
        r2 = []
        for p in r1:
            if p[1] - p[0] < int(O.min_seed_len * O.split_factor + .499) or p[2] > O.split_width:
                continue
            m1, _ = so.smem1(oidx, q, (p[0] + p[1]) >> 1, p[2] + 1)
            r2 += [m for m in m1 if m[1] - m[0] >= O.min_seed_len]
        r3, x = [], 0
        while x < n:
            if q[x] < 4:
                m, x = so.seed_strategy1(oidx, q, x, O.min_seed_len, O.max_mem_intv)
                if m is not None and m[2] > 0:
                    r3.append(m)
            else:
                x += 1
        if {m[0] for m in r1} & {m[0] for m in r2} & {m[0] for m in r3}:
            found.append(name)
    assert "repeat" in found, found


@pytest.fixture(scope="module")
def overflow_case():
    """4,200 long reads (more than device_caps().chains = 4,096): 80 bases cut from a 200 kb
    genome, one planted 40-mer, 60 random bases.  Reads of N, a prefix of the 40-mer, N have one start with
    hits (4,200 of them, within the slab's 8,192) and one chain per long read, so it is the
    chaining that overflows, in the thread's own slab, after it claimed the range-table slots of
    long reads 0 .. 4,095: the 12-base prefix under the bwa-sr options, the 17-base prefix under
    the finish options (the lazy table fills that one start only; under bwa-sr its six starts
    outgrow the hit table first, as the whole 40-mer's do, and it is chained in the grown slabs
    of the later passes).  The ordinary reads are the genome part of long reads below and above
    4,096, either strand, and 60 N followed by a long read's last 60 bases: their ranges are the
    ones the overflowing read claimed, and the latter's seed (query 60, 40 bases after the
    planted block) is one that the overflowing read's seed (query 50, at the block) would take
    into its chain -- a slot and range record left behind loses it."""
    rng = np.random.default_rng(77)
    G = rng.integers(0, 4, 200_000)
    k40 = rng.integers(0, 4, 40)
    starts = rng.integers(0, len(G) - 80, 4200)
    lrs = [np.concatenate([G[s:s + 80], k40, rng.integers(0, 4, 60)]) for s in starts]
    lr_seq, lr_off = _cat(lrs)
    ordinary = []
    for k, i in enumerate((3, 50, 700, 1999, 2500, 3100, 4000, 4095, 4096, 4150, 17, 2048)):
        r = [int(x) for x in lrs[i][:78]]
        ordinary.append(np.asarray(_rc(r) if k % 3 == 2 else r))
    for i in (5, 1000, 4090, 4100):
        ordinary.append(np.concatenate([np.full(60, N), lrs[i][120:]]))
    over = {n: np.concatenate([np.full(50, N), k40[:n], np.full(60, N)]) for n in (12, 17, 40)}
    ix = seed.SeedIndex(lr_seq, lr_off)
    yield ix, ordinary, over
    ix.close()


@pytest.mark.parametrize("finish", [False, True])
def test_range_table_reuse_across_an_overflowing_read(overflow_case, finish, monkeypatch):
    """One thread, one slab: an ordinary read, the reads that overflow, ordinary reads.  Every
    ordinary read gives the seeds it gives alone and the host path's, also from a slab that
    starts poisoned (the table is cleared by its owner, every read leaves it clear).  (With the
    reset of chain_seq's overflow returns taken out, neither option set passes: the finish set's
    seeds differ without the N-prefixed reads, and with them a stale range record takes a seed into
    a chain of the read before and the chaining does not end.)"""
    ix, ordinary, over = overflow_case
    o = seed.default_opts(finish)
    o.max_occ = 1 << 20   # (every occurrence a chain: -c would sample 500 of them)
    mine = over[17] if finish else over[12]   # the read whose chaining overflows in the slab
    order = [ordinary[0], mine, ordinary[1], ordinary[2], over[40], ordinary[3], mine] + ordinary[4:8] + \
            [ordinary[12], ordinary[13], over[12], over[17]] + ordinary[8:12] + ordinary[14:]
    is_ord = [any(r is x for x in ordinary) for r in order]
    seq, off = _cat(order)
    host = _tuples(ix.map(seq, off, o, threads=1))
    alone = {}
    for i, r in enumerate(order):
        if is_ord[i]:
            s1, o1 = _cat([r])
            t, st = ix.map_device_caps(s1, o1, o, threads=1)
            assert st[0] == 0
            alone[i] = [(i,) + x[1:] for x in _tuples(t)]
            assert len(alone[i]) > 0
    # the overflowing read alone, sampled below the capacity (-c 4000): it fits
    s1, o1 = _cat([mine])
    ocap = seed.default_opts(finish)
    ocap.max_occ = 4000
    assert ix.map_device_caps(s1, o1, ocap, threads=1)[1][0] == 0
    for fill in (None, "0xA5", "0x00"):
        if fill:
            monkeypatch.setenv("PRGPU_SCRATCH_FILL", fill)
        dev, st = ix.map_device_caps(seq, off, o, threads=1)
        if fill:
            monkeypatch.delenv("PRGPU_SCRATCH_FILL")
        dev = _tuples(dev)
        for i in range(len(order)):
            got = [t for t in dev if t[0] == i]
            if is_ord[i]:
                assert st[i] == 0 and got == alone[i], (fill, i)
                assert got == [t for t in host if t[0] == i], (fill, i)
            elif st[i] == 0:
                assert got == [t for t in host if t[0] == i], (fill, i)
            else:
                assert got == [], (fill, i)

"""Pass 1 of the device seeding with the lazy occurrence table and a hit budget per read
(seed_core.h materialize / collect_intv, Caps.budget), run on the host
(pr_seed_map_device_pass1: pass 1's small slices, one slice for every read in read order).

The finish options on a near-exact index (100 kb genome, 800 x 5 kb long reads at 0.2 % error,
~40x): exact short reads consult a few starts, reads with 10 % substitutions most of theirs, so
their pools pass a budget of 512 hits.  Exact and noisy reads alternate, so every exact read
maps on the slice a flagged read has just left through the early exit."""
import numpy as np

from proovread_amd import seed, synth

BUDGET = 512
OVER_HITS = 2   # seedc::SC_OVER_HITS


def _by_read(tasks, n):
    out = [[] for _ in range(n)]
    for t in tasks:
        out[int(t["sr"])].append(tuple(int(x) for x in t))
    return out


def _case():
    d = synth.simulate(23, 100_000, 800, 5000, 1.0, p_ins=0.0005, p_del=0.0005, p_sub=0.001)
    n = d.n_sr - d.n_sr % 2
    assert n >= 600
    sr = d.sr_seq[:d.sr_off[n]].reshape(n, 150).copy()
    rng = np.random.default_rng(5)
    noisy = np.arange(n) % 2 == 1
    sub = (rng.random(sr.shape) < 0.10) & noisy[:, None]
    sr[sub] = (sr[sub] + rng.integers(1, 4, int(sub.sum())).astype(np.uint8)) % 4
    return d, sr.reshape(-1), d.sr_off[:n + 1], noisy


def _eager_hits(ix, q):
    """The read's eager table: the occurrences of every 12-mer start, summed."""
    return sum(ix.occ(q[a:a + 12]) for a in range(len(q) - 11))


def test_budget_flags_exactly_the_reads_beyond_it_and_leaves_the_rest_alone():
    d, ss, so, noisy = _case()
    n = len(so) - 1
    ix = seed.SeedIndex(d.lr_seq, d.lr_off)
    o = seed.default_opts(True)
    want = _by_read(ix.map(ss, so, o, threads=4), n)
    t0, st0, hits0 = ix.map_device_pass1(ss, so, o, budget=0)
    t1, st1, hits1 = ix.map_device_pass1(ss, so, o, budget=BUDGET)
    b0, b1 = _by_read(t0, n), _by_read(t1, n)
    # without a budget: the slices hold every read of this set, and the pool's fill is known
    assert not st0.any()
    assert all(b0[i] == want[i] for i in range(n))
    # every unflagged read's tasks are what they were (and the host path's); a flagged read has none
    ok = st1 == 0
    assert all(b1[i] == b0[i] for i in range(n) if ok[i])
    assert all(b1[i] == [] for i in range(n) if not ok[i])
    # flagged on hits, and on nothing else, exactly the reads whose pool passes the budget
    assert np.array_equal(st1, np.where(hits0 > BUDGET, OVER_HITS, 0))
    assert np.array_equal(hits1[ok], hits0[ok])
    # ... which are most of the noisy reads and few of the exact ones
    assert (st1[noisy] != 0).mean() > 0.5 and (st1[noisy] == 0).sum() > 0
    assert (st1[~noisy] == 0).mean() > 0.75
    # the slice after a flagged read's early exit: the next read maps as on a fresh one
    after = [i for i in range(1, n) if ok[i] and not ok[i - 1]]
    assert len(after) > 100 and sum(len(want[i]) for i in after) > 100
    assert all(b1[i] == want[i] for i in after)
    # a flagged read reports a need that its whole eager table fits, so any lazy pool of it does
    for i in np.nonzero(~ok)[0]:
        q = ss[so[i]:so[i + 1]]
        assert hits1[i] >= _eager_hits(ix, q) >= hits0[i] > BUDGET
    ix.close()


def test_budget_at_or_above_the_capacity_and_eager_options_change_nothing():
    d, ss, so, _ = _case()
    ix = seed.SeedIndex(d.lr_seq, d.lr_off)
    o = seed.default_opts(True)
    t0, st0, hits0 = ix.map_device_pass1(ss, so, o, budget=0)
    for budget in (4096, 1 << 20):
        t1, st1, hits1 = ix.map_device_pass1(ss, so, o, budget=budget)
        assert np.array_equal(t1, t0) and np.array_equal(st1, st0) and np.array_equal(hits1, hits0)
    # the iteration options take the eager table: no pool, no budget
    oi = seed.default_opts(False)
    ta, sta, ha = ix.map_device_pass1(ss, so, oi, budget=0)
    tb, stb, hb = ix.map_device_pass1(ss, so, oi, budget=64)
    assert np.array_equal(ta, tb) and np.array_equal(sta, stb) and not ha.any() and not hb.any()
    ix.close()

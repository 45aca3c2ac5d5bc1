"""Long reads of more than 16,384 alignments through the device hand-off (pipe_big.hip: runs
sorted in LDS, merged in HBM) -- a deep pile-up, the boundaries of the run count, a long read in
bwa mode, the whole loop, and the refusal beyond 2^20.  Bar: equality with the CPU chains the
other iteration tests use, and with a host sort of what the SW stage reported."""
import ctypes as C
import dataclasses
import functools
import io
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_bind as ob
from pipeline_oracle import consensus_cases, sam_for_tasks

pytestmark = pytest.mark.gpu

TASK_FIELDS = ("t_sr", "t_lr", "t_strand", "t_qbeg", "t_rbeg", "t_slen")
ACGT = np.frombuffer(b"ACGT", np.uint8)
PARAMS = {False: {"coverage": "11.25", "use_ref_qual": "1", "detect_chimera": "0"},
          True: {"coverage": "22.5", "use_ref_qual": "0", "detect_chimera": "1"}}


def with_tasks(d, idx):
    """d with the tasks idx (in that order; an index may repeat)."""
    return dataclasses.replace(d, **{k: np.ascontiguousarray(getattr(d, k)[idx]) for k in TASK_FIELDS})


def only_reads(d, lo, hi):
    """Long reads [lo, hi) of d and their tasks (every short read stays)."""
    idx = np.nonzero((d.t_lr >= lo) & (d.t_lr < hi))[0]
    e = with_tasks(d, idx)
    a0, a1 = int(d.lr_off[lo]), int(d.lr_off[hi])
    return dataclasses.replace(e, lr_seq=np.ascontiguousarray(d.lr_seq[a0:a1]), lr_off=d.lr_off[lo:hi + 1] - a0,
                               lr_start=d.lr_start[lo:hi], t_lr=(e.t_lr - lo).astype(np.int32))


@pytest.fixture(scope="module")
def deep():
    """Two ~6.4 kb reads under 480x: 19,597 and 19,638 single-seed tasks."""
    from proovread_amd import synth
    d = synth.simulate(7, 9000, 2, 6000, 480)
    assert [int(x) for x in np.bincount(d.t_lr)] == [19597, 19638]
    return d


def launch(d, finish, binf=None):
    from proovread_amd import cns, iteration, sw
    it = iteration.Iteration(d)
    p = PARAMS[finish]
    opts = sw.default_opts(finish=finish)
    if binf:
        opts.bin_size, opts.bin_length = binf
    it.launch(opts, cns.CnsParams(coverage=float(p["coverage"]), use_ref_qual=p["use_ref_qual"] == "1",
                                  detect_chimera=p["detect_chimera"] == "1"))
    return it


def sw_outputs(it):
    """The resident SW batch's per-task outputs after an explicit-task launch."""
    from proovread_amd import sw
    L = it.L
    res = sw.SwResult(it.n_task)
    tot, nov = C.c_int64(), C.c_int64()
    assert L.pr_sw_cigar_total(it.ctx.h, C.byref(tot), C.byref(nov)) == 0
    res.size_cigar(tot.value)
    assert L.pr_sw_download(it.ctx.h, C.byref(res.c)) == 0
    return res


# ------------------------------------------------------------------ 1. parity, deep pile-up
@pytest.fixture(scope="module")
def deep_thinned(deep):
    """Read 0 whole (big), read 1 thinned to every fourth task (small)."""
    i0, i1 = np.nonzero(deep.t_lr == 0)[0], np.nonzero(deep.t_lr == 1)[0]
    return with_tasks(deep, np.concatenate([i0, i1[::4]]))


@pytest.fixture(scope="module")
def fast_chain(deep_thinned):
    """sam_for_tasks converts both reads to text and to nt4 again for every one of its 24.5 k
    tasks (~2 ms each on a 6.4 kb read).  The same chain with those conversions and the SW
    oracle's result per distinct call remembered (the filtered variant repeats the unfiltered
    one's calls): -> the dataset to hand it."""
    from proovread_amd import synth

    class Cached(synth.Dataset):
        __hash__ = object.__hash__
        lr_str = functools.lru_cache(maxsize=None)(synth.Dataset.lr_str)
        sr_str = functools.lru_cache(maxsize=None)(synth.Dataset.sr_str)

    nt4, sw_task, memo = ob.nt4, ob.sw_task, {}

    def sw_task_once(opts, q, ref, *a):
        k = (bytes(opts), q, ref, *a)
        if k not in memo:
            memo[k] = sw_task(opts, q, ref, *a)
        return memo[k]

    ob.nt4, ob.sw_task = functools.lru_cache(maxsize=None)(nt4), sw_task_once
    yield Cached(**{f.name: getattr(deep_thinned, f.name) for f in dataclasses.fields(deep_thinned)})
    ob.nt4, ob.sw_task = nt4, sw_task


@pytest.mark.parametrize("binf", [None, (20, 300.0)], ids=["nofilter", "b20-l300"])
@pytest.mark.parametrize("finish", [False, True], ids=["regular", "finish"])
def test_deep_pileup_matches_cpu_chain(deep_thinned, fast_chain, finish, binf):
    """The finish options report nearly nothing on raw reads: read 0 still sorts through HBM (its
    19,597 tasks decide that) and hands over what is left."""
    d = deep_thinned
    it = launch(d, finish, binf)
    got = it.results()
    st = it.handoff_stats()
    task = "bwa-sr-finish" if finish else "bwa-sr"
    sams = sam_for_tasks(fast_chain, task, bin_filter=binf)
    assert st.big_reads == 1 and st.big_alns == len(sams.get(0, []))
    assert st.max_alns == max(len(v) for v in sams.values())
    if not finish:   # all of read 0's tasks are reported; the filter must bite
        assert st.big_alns < 16384 if binf else st.big_alns == 19597
    for c, g in zip(consensus_cases(d, sams, PARAMS[finish]), got):
        want = ob.run_case(c)
        assert want["rc"] == 0 and g.status == 0, (c.name, want["rc"], g.status)
        assert g.fastq == want["fastq"], c.name
        assert g.trace == want["trace"], c.name
        assert "".join(l + "\n" for l in g.chim_lines()) == want["chim"], c.name
    # the small read beside the big one = the small read alone (the LDS path)
    alone = launch(only_reads(d, 1, 2), finish, binf)
    assert alone.handoff_stats().big_reads == 0
    a = alone.results()[0]
    assert (a.status, a.seq, a.qual, a.trace, a.chim) == (got[1].status, got[1].seq, got[1].qual, got[1].trace, got[1].chim)


# ------------------------------------------------------------------ 2. order and boundaries
@pytest.fixture(scope="module")
def reported(deep):
    """Read 0's tasks that the SW stage reports (score >= -T, CIGAR ok), in task order."""
    d0 = only_reads(deep, 0, 1)
    it = launch(d0, False)
    r = sw_outputs(it)
    ok = (r["pass"] != 0) & (r["status"] == 0)
    assert it.handoff_stats().max_alns == int(ok.sum()) > 16385
    return d0, np.nonzero(ok)[0]


def check_order(d, n_expected):
    it = launch(d, False)
    st = it.handoff_stats()
    r = sw_outputs(it)
    ok = np.nonzero((r["pass"] != 0) & (r["status"] == 0))[0]
    want = sorted((int(i) for i in ok), key=lambda i: (int(r["pos"][i]), int(d.t_strand[i]), i))
    assert st.max_alns == len(want) == n_expected
    assert [int(x) for x in it.handoff_order(0)] == want
    assert it.statuses()[0] == 0
    return st, r, want


@pytest.mark.parametrize("n", [16384, 16385, 32768, 32769])
def test_order_at_the_run_boundaries(reported, n):
    """Read 0 cut to n reported alignments (its reported tasks, taken twice over to reach 2 and 3
    runs: the second copy ties with the first in POS and strand)."""
    d0, ok = reported
    d = with_tasks(d0, np.concatenate([ok, ok])[:n])
    st, _, _ = check_order(d, n)
    assert st.big_reads == (0 if n <= 16384 else 1)
    assert st.big_alns == (0 if n <= 16384 else n)


def test_ties_across_a_run_boundary(reported):
    """40 copies of one task around index 16,384: equal (POS, strand) on both sides of the first
    run's end come out in task order."""
    d0, ok = reported
    idx = np.concatenate([ok[:16364], np.full(40, ok[9000]), ok[16364:16500]])
    st, r, want = check_order(with_tasks(d0, idx), len(idx))
    assert st.big_reads == 1
    block = [i for i in want if 16364 <= i < 16404]
    assert block == list(range(16364, 16404))
    assert len({(int(r["pos"][i]), int(with_tasks(d0, idx).t_strand[i])) for i in block}) == 1


# ------------------------------------------------------------------ 3. long read, bwa mode
def test_long_read_bwa_mode_matches_cpu_chain():
    """Two ~34 kb reads under 80x in bwa mode (every seed of the kept chains), the finish task
    with chimera detection: the big path feeds the chimera bins too.  The reads carry the error
    of corrected reads, which is what the finish task maps to (raw reads get 1 and 9 alignments
    under its options): 18,235 and 18,169 alignments."""
    from proovread_amd import seed, synth
    d = synth.simulate(7, 40000, 2, 34000, 80, p_ins=0.01, p_del=0.005, p_sub=0.002)
    ix = seed.SeedIndex(d.lr_seq, d.lr_off)
    d = synth.with_seeds(d, ix.map(d.sr_seq, d.sr_off, seed.default_opts(True), threads=4))
    ix.close()
    it = launch(d, True)
    got = it.results()
    st = it.handoff_stats()
    assert st.big_reads == 2 and st.max_alns > 16384
    sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "oracle"))
    import cpu_chain
    p = PARAMS[True]
    _, _, want, _ = cpu_chain.run_sample(d, range(d.n_lr), task="bwa-sr-finish", coverage=float(p["coverage"]),
                                         use_ref_qual=False, workers=8, detect_chimera=True, full=True)
    for i, (g, (rc, fq, trace, chim)) in enumerate(zip(got, want)):
        assert rc == 0 and g.status == 0, (i, rc, g.status)
        assert g.fastq == fq, i
        assert g.trace == trace, i
        assert "".join(l + "\n" for l in g.chim_lines()) == chim, i


# ------------------------------------------------------------------ 4. whole loop
def test_loop_with_a_big_read_matches_oracle_loop(deep):
    import loop_oracle
    from proovread_amd import correct
    d = deep
    lrs = [(f"lr_{i}", ACGT[np.minimum(d.lr_seq[d.lr_off[i]:d.lr_off[i + 1]], 3)].tobytes(), None) for i in range(d.n_lr)]
    sr = io.BytesIO()
    for i in range(d.n_sr):
        s = ACGT[np.minimum(d.sr_seq[d.sr_off[i]:d.sr_off[i + 1]], 3)].tobytes()
        sr.write(b"@sr%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    cfg = correct.LoopConfig(coverage=480.0, seed_threads=4, sampling=False,
                             tasks=("read-long", "bwa-sr-1", "bwa-sr-finish"))
    want = correct.run(lrs, sr.getvalue(), cfg, stages=loop_oracle.OracleStages(8))
    got = correct.run(lrs, sr.getvalue(), cfg)
    assert [e.task for e in got.log] == [e.task for e in want.log] == list(cfg.tasks)
    assert max(e.part_ms["big_reads"] for e in got.log[1:]) >= 1
    for g, w in zip(got.log, want.log):
        assert (g.n_sr, g.n_tasks, g.bpt, g.bpn, g.shortcut) == (w.n_sr, w.n_tasks, w.bpt, w.bpn, w.shortcut), g.task
    assert got.reads.seqs == want.reads.seqs
    assert got.reads.quals == want.reads.quals
    assert got.chim == want.chim


# ------------------------------------------------------------------ 5. refusal
def test_more_than_2_pow_20_tasks_on_one_read_is_refused():
    """task_lr_off claims 2^20 + 1 tasks on read 1: PR_ERR_CAPACITY naming it, before any upload."""
    from proovread_amd import iteration, synth
    d = synth.simulate(3, 4000, 2, 1500, 2)
    n = (1 << 20) + 1
    z = np.zeros(n, np.int32)
    e = dataclasses.replace(d, t_sr=z, t_lr=np.ones(n, np.int32), t_strand=np.zeros(n, np.uint8), t_qbeg=z, t_rbeg=z,
                            t_slen=z + 12)
    with pytest.raises(RuntimeError, match=r"PR_ERR_CAPACITY: long read 1 has 1048577 tasks"):
        iteration.Iteration(e)

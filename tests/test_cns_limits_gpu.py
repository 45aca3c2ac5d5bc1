"""The consensus kernel at every per-read limit of DESIGN.md §7 and on alignments that span
several pileup windows (tests/cns_limit_cases.py builds the inputs).

Each limit has an input one unit inside it, which must equal the C oracle byte for byte (FASTQ,
trace, chimera lines, kept flags), and one just outside, which must be refused with
PR_ERR_CAPACITY while the reads launched with it, and the next batch on the same context, stay
exact.  The limits are written here as literals: they are product contract, and a change of the
kernel's geometry has to fail this file and update DESIGN.md.

The unmarked tests check on the CPU that every input is what it claims to be (oracle rc 0, the
intended alignments kept, state and pair counts by a plain Python walk over the CIGARs)."""
import dataclasses
import functools
from pathlib import Path

import numpy as np
import pytest

import casefmt
import cns_limit_cases as lc
import oracle_bind as ob
from cns_case_util import case_inputs

PR_ERR_CAPACITY = -9

# the limits (GeoL = CnsGeo<2048, 1024, 8192, 1, false>, GeoM = CnsGeo<256, 1024, 512, 4, true>)
MAX_BINS = 17616           # L <= 352,319 at bin 20
BINS_IN, BINS_OUT = 352319, 352320
BINS_RETRY = 120000        # 6,001 bins: more than a 4-per-CU geometry holds, through the retry
WIN_IN, WIN_OUT = 1571840, 1571841   # nwin 1,535 | 1,536 of 1,024 columns, at bin 100
WIN_BIN = 100.0
KEPT_IN, KEPT_OUT = 65535, 65536
SPAN_IN, SPAN_OUT = 4095, 4096
TCAP_L, TCAP_M = 2048, 256
WCAP_L = 8192
CHIM_TCAP, CHIM_CL = 256, 8

GOLD = Path(__file__).resolve().parent / "golden"


@functools.lru_cache(maxsize=None)
def neighbours_src():
    """Two short golden cases to stand on either side of a refused read."""
    cases = casefmt.read_cases(GOLD / "cns_cases.txt")
    expect = casefmt.read_expect(GOLD / "cns_expected.txt")
    ok = [c for c in cases if c.name.startswith("rnd") and c.p("qual_weighted") == "0" and c.p("noref") == "0"
          and not expect[c.name].error and len(c.ref[1]) < 1000 and len(c.sam) > 20]
    return ok[0], ok[1]


@functools.lru_cache(maxsize=None)
def build(name):
    kind, _, arg = name.partition("_")
    if kind == "bins":
        return lc.spread_case(name, int(arg), 205, 21)
    if kind == "win":
        return lc.spread_case(name, int(arg), 200, 22)
    if kind == "stack":
        return lc.stack_case(int(arg))
    if kind == "span":
        return lc.span_case(int(arg))
    if kind == "states":
        return lc.states_case(int(arg))
    return {"qoff_over": lc.qoff_case, "pairs_over": lc.pairs_case, "chim_scan": lambda: lc.chim_case(False),
            "chim_over": lambda: lc.chim_case(True), "spans": lambda: lc.spans_case(False),
            "spans_chim": lambda: lc.spans_case(True)}[name]()


def bin_of(name):
    return WIN_BIN if name.startswith("win_") else 20.0


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The oracle's result of a case: computed once per module, never changed."""
    return ob.run_case(build(name), bin_size=bin_of(name))


@functools.lru_cache(maxsize=None)
def neighbour(which, like):
    """Golden neighbour `which` with the parameters of case `like`, and its oracle result."""
    c = dataclasses.replace(neighbours_src()[which], params={k: build(like).p(k) for k in casefmt.DEFAULT_PARAMS})
    want = ob.run_case(c, bin_size=bin_of(like))
    assert want["rc"] == 0, (c.name, like)
    return c, want


INSIDE = [f"bins_{BINS_IN}", f"bins_{BINS_RETRY}", f"win_{WIN_IN}", f"stack_{KEPT_IN}", f"span_{SPAN_IN}",
          f"states_{TCAP_L}", f"states_{TCAP_M}", f"states_{TCAP_M + 1}", "chim_scan", "spans", "spans_chim"]
OUTSIDE = [f"bins_{BINS_OUT}", f"win_{WIN_OUT}", f"stack_{KEPT_OUT}", f"span_{SPAN_OUT}", "qoff_over",
           f"states_{TCAP_L + 1}", "pairs_over", "chim_over"]
LARGE_TOO = [f"span_{SPAN_IN}", f"states_{TCAP_L}", f"states_{TCAP_M}", f"states_{TCAP_M + 1}", f"stack_{KEPT_IN}"]


# ------------------------------------------------------------------------------------------
# CPU: the inputs are what they claim to be
@pytest.mark.parametrize("name", INSIDE)
def test_inside_input_is_accepted_by_the_oracle(name):
    c, want = build(name), oracle(name)
    assert want["rc"] == 0
    assert want["kept"] == "1" * len(c.sam)   # exactly the alignments the case intends


def test_bin_and_window_counts_sit_on_their_limits():
    for L, nb in ((BINS_IN, MAX_BINS), (BINS_OUT, MAX_BINS + 1), (BINS_RETRY, 6001)):
        assert len(build(f"bins_{L}").ref[1]) == L and int(L / 20.0) + 1 == nb
    for L, nwin in ((WIN_IN, 1535), (WIN_OUT, 1536)):
        assert len(build(f"win_{L}").ref[1]) == L and -(-L // lc.W) == nwin
        assert int(L / WIN_BIN) + 1 <= MAX_BINS   # the bins do not bind first
    assert 2 * (1535 + 1) == 3 * lc.W and 2 * (1536 + 1) > 3 * lc.W
    assert len(oracle(f"bins_{BINS_IN}")["bin_bases"]) == MAX_BINS
    # both ends of the read are covered: the last window and the last bins are worked on
    for name in (f"bins_{BINS_IN}", f"win_{WIN_IN}"):
        starts = [lc.fields(l)[0] for l in build(name).sam]
        assert starts[0] == 0 and starts[-1] + 150 == len(build(name).ref[1])


def test_stack_puts_every_alignment_on_the_same_columns():
    for n in (KEPT_IN, KEPT_OUT):
        c = build(f"stack_{n}")
        assert len(c.sam) == n and len(set(c.sam)) == 1 and lc.fields(c.sam[0])[1] == [(60, "M")]
    want = oracle(f"stack_{KEPT_IN}")
    assert want["kept"] == "1" * KEPT_IN and KEPT_IN == 0xFFFF
    assert ob.run_case(build(f"stack_{KEPT_OUT}"))["kept"] == "1" * KEPT_OUT


def _states_of(ops):
    return sum(n for n, op in ops if op in "MD")


def test_span_alignment_is_kept_whole():
    for ns in (SPAN_IN, SPAN_OUT):
        c = build(f"span_{ns}")
        i = [k for k, l in enumerate(c.sam) if l.startswith("long\t")][0]
        start0, ops, seq = lc.fields(c.sam[i])
        assert start0 == lc.SPAN_RP and _states_of(ops) == ns and len(seq) > 160
        # the last op is an M longer than the taboo length: no trim at the 3' end; the insertion
        # lies 8 read bases or more from it, on the state of index 4080
        assert ops[-1][1] == "M" and ops[-1][0] > 7 and ops[-2] == (4, "I") and ops[-1][0] >= 8
        assert _states_of(ops[:-2]) - 1 == 4080
        want = ob.run_case(c) if ns == SPAN_OUT else oracle(f"span_{ns}")
        assert want["rc"] == 0 and want["kept"][i] == "1"
        # the long alignment alone covers its insertion: the consensus carries the four bases
        assert want["trace"].count("D") == 4 and "TGCA" in want["fastq"].split("\n")[1]


def test_query_offset_case_reaches_the_walk():
    c = build("qoff_over")
    i = [k for k, l in enumerate(c.sam) if l.startswith("clip\t")][0]
    start0, ops, seq = lc.fields(c.sam[i])
    assert ops[0] == (65536, "S") and _states_of(ops) < SPAN_IN
    assert all(n <= 0xFFFF for n, op in ops if op == "I")         # no insertion too long by itself
    assert (len(seq) - 65536) / len(seq) >= 0.7                    # (the trim would skip it below)
    want = ob.run_case(c)
    assert want["rc"] == 0 and want["kept"][i] == "1"


@pytest.mark.parametrize("n", [TCAP_M, TCAP_M + 1, TCAP_L, TCAP_L + 1])
def test_state_counts(n):
    c = build(f"states_{n}")
    want = oracle(f"states_{n}") if n != TCAP_L + 1 else ob.run_case(c)
    assert want["rc"] == 0
    kept = lc.kept_lines(c, want["kept"])
    assert len(kept) == len(c.sam) and lc.n_states(kept) == n
    # every insertion follows a reference 'A' and is a 6-mer: n states of 7 characters
    assert {len(s) for l in kept for _, s in lc.ins_states(l)} == {7}
    assert {s[0] for l in kept for _, s in lc.ins_states(l)} == {"A"}
    assert max(lc.window_pairs(kept).values()) <= WCAP_L


def test_pair_count_is_well_over_the_window_table():
    c = build("pairs_over")
    want = ob.run_case(c)
    assert want["rc"] == 0
    kept = lc.kept_lines(c, want["kept"])
    assert lc.window_pairs(kept)[0] >= 1.5 * WCAP_L
    assert lc.n_states(kept) <= 256   # (the state table is not what overflows)


def _chim_side_pairs(c, kept, lo, hi):
    """distinct (column, state) pairs of the compared columns among the kept alignments whose bin
    is in [lo, hi], and the states per column"""
    pairs = {cs for l in lc.kept_lines(c, kept) if lo <= lc.center_bin(l) <= hi for cs in lc.ins_states(l)
             if lc.CHIM_MF <= cs[0] <= lc.CHIM_MT}
    return pairs


@pytest.mark.parametrize("name", ["chim_scan", "chim_over"])
def test_chimera_cases_fill_their_tables(name):
    c = build(name)
    want = oracle(name) if name == "chim_scan" else ob.run_case(c)
    assert want["rc"] == 0
    # the candidate: bins 30 and 31 at or below bin_max_bases / 5 + 1, every other scanned bin above
    thr = 20 * 25 / 5 + 1
    bb = want["bin_bases"]
    assert [b for b in range(5, len(bb) - 5) if bb[b] <= thr] == list(lc.CHIM_LOW)
    left = _chim_side_pairs(c, want["kept"], *lc.CHIM_LEFT)
    right = _chim_side_pairs(c, want["kept"], *lc.CHIM_RIGHT)
    if name == "chim_over":
        assert len(left) >= 2 * CHIM_TCAP
        return
    assert want["chim"].strip() != ""
    assert len(left) <= CHIM_TCAP and len(right) <= CHIM_TCAP
    per_col = {}
    for col, _ in list(left) + list(right):
        per_col[col] = per_col.get(col, 0) + 1
    assert max(per_col.values()) > CHIM_CL and min(per_col.values()) <= CHIM_CL   # both paths
    assert {s for _, s in left} & {s for _, s in right}                          # a state on both sides


@pytest.mark.parametrize("name", ["spans", "spans_chim"])
def test_spans_case_shape(name):
    c, want = build(name), oracle(name)
    assert want["rc"] == 0 and want["kept"] == "1" * len(c.sam)
    ends = {}
    for l in c.sam:
        start0, ops, seq = lc.fields(l)
        ns = _states_of(ops)
        if ns >= 1100:
            ends.setdefault(ns, set()).add((start0 + ns) % lc.W)
            assert len(seq) > 1000
    assert ends == {1100: {0, lc.W - 1, 1}, 2100: {0, lc.W - 1, 1}, 3100: {0, lc.W - 1, 1}, 4095: {0, lc.W - 1, 1}}
    lseq = sorted(len(lc.fields(l)[2]) for l in c.sam)
    assert sum(1 for x in lseq if 160 < x < 1100) >= 8   # the slow SEQ path, short of a window too
    # indels on the window boundaries, and they reach the consensus
    cols = {col % lc.W for l in c.sam for col, _ in lc.ins_states(l)}
    assert cols == {lc.W - 1, 0}
    assert want["trace"].count("D") > 0 and want["trace"].count("I") > 0
    if name == "spans_chim":
        assert len(want["chim"].strip().split("\n")) >= 2


# ------------------------------------------------------------------------------------------
# GPU
def gpu_run(cases, bin_size=20.0):
    """One pr_cns_run launch of the cases on the default context -> (results, raw output arrays)."""
    import ctypes as C
    from proovread_amd import _abi, cns
    ins = [case_inputs(c, bin_size) for c in cases]
    assert all(p == ins[0][2] for _, _, p in ins)
    reads = [x[0] for x in ins]
    d = cns.pack_chunk(reads, [x[1] for x in ins])
    cb = cns.make_c_batch(d)
    out = cns.OutBuffers(d, cb, bin_size)
    pc = ins[0][2].to_c()
    _abi.check(_abi.lib().pr_cns_run(_abi.default_context().h, C.byref(pc), C.byref(cb), C.byref(out.c)), "pr_cns_run")
    return out.results([r.id for r in reads], d), out.a


def assert_exact(r, want, what):
    assert want["rc"] == 0 and r.status == 0, (what, want["rc"], r.status)
    assert r.fastq == want["fastq"], what
    assert r.trace == want["trace"], what
    assert "".join(l + "\n" for l in r.chim_lines()) == want["chim"], what
    assert "".join(map(str, r.kept.tolist())) == want["kept"], what


@pytest.mark.gpu
@pytest.mark.parametrize("name", INSIDE)
def test_gpu_inside_limit_matches_oracle(name):
    res, _ = gpu_run([build(name)], bin_of(name))
    assert_exact(res[0], oracle(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", LARGE_TOO)
def test_gpu_inside_limit_large_geometry(name, monkeypatch):
    monkeypatch.setenv("PRGPU_CNS_LARGE", "1")
    res, _ = gpu_run([build(name)], bin_of(name))
    assert_exact(res[0], oracle(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", OUTSIDE)
def test_gpu_outside_limit_is_refused_alone(name):
    """The refused read between two ordinary ones in one launch: PR_ERR_CAPACITY and no output
    for it, its neighbours exact; then an ordinary batch on the same context, exact again (the
    retry list, the K pool and the work counter survive the refusal)."""
    (c0, w0), (c1, w1) = neighbour(0, name), neighbour(1, name)
    res, a = gpu_run([c0, build(name), c1], bin_of(name))
    assert res[1].status == PR_ERR_CAPACITY, (name, res[1].status)
    assert (int(a["seq_len"][1]), int(a["trace_len"][1])) == (0, 0), name
    assert_exact(res[0], w0, (name, "before"))
    assert_exact(res[2], w1, (name, "after"))
    res, _ = gpu_run([c1, c0], bin_of(name))
    assert_exact(res[0], w1, (name, "next batch"))
    assert_exact(res[1], w0, (name, "next batch"))


@pytest.mark.gpu
def test_gpu_chimera_bin_size_is_bounded():
    """A chimera candidate compares 6 bins of columns in tables of 128: refused before the launch."""
    from proovread_amd import cns
    lr, alns, params = case_inputs(neighbours_src()[0], 22.0)
    params = dataclasses.replace(params, detect_chimera=True)
    with pytest.raises(RuntimeError, match="bin_size"):
        cns.run_chunk([lr], [alns], params)
    r = cns.run_chunk([lr], [alns], dataclasses.replace(params, bin_size=21.0))[0]
    assert r.status == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["spans", "spans_chim"])
def test_gpu_spans_through_bam_records(name):
    """The multi-window case as it arrives from an external aligner: BAM records decoded and
    grouped on the device (cns.run_bam_records)."""
    import bam_cases
    from proovread_amd import bamio, cns
    c = build(name)
    lr, _, params = case_inputs(c)
    body = bamio._native_sort(bam_cases.encode(c.sam, [c.ref_id]))
    r = cns.run_bam_records([lr], [c.ref_id], body, params)[0]
    want = oracle(name)
    assert r.status == 0 and len(r.kept) == len(c.sam)
    assert (r.fastq, r.trace) == (want["fastq"], want["trace"])
    assert "".join(l + "\n" for l in r.chim_lines()) == want["chim"]
    assert "".join(map(str, r.kept.tolist())) == want["kept"]


@pytest.mark.gpu
def test_gpu_iteration_refuses_the_long_read_only():
    """One iteration (SW -> hand-off -> consensus) over four 2.5 kb reads and one of 352,320 bp with a
    few hundred tasks: the long one comes back with PR_ERR_CAPACITY, the others equal the CPU chain."""
    from pipeline_oracle import consensus_cases, sam_for_tasks
    from proovread_amd import cns, iteration, sw, synth
    from test_sw_edge_gpu import merge
    small = synth.simulate(61, 40000, 4, 2500, 15, sr_frac=1.0)
    big = synth.simulate(62, 400000, 1, BINS_OUT, 0.15, sr_frac=1.0)
    # (the simulated read carries insertions: cut it to the length, with the tasks that end in it)
    assert int(big.lr_off[1]) > BINS_OUT
    keep = big.t_rbeg + big.t_slen + 200 <= BINS_OUT
    big = dataclasses.replace(big, lr_seq=big.lr_seq[:BINS_OUT].copy(), lr_off=np.array([0, BINS_OUT], np.int64),
                              **{k: getattr(big, k)[keep] for k in ("t_sr", "t_lr", "t_strand", "t_qbeg", "t_rbeg",
                                                                   "t_slen")})
    assert 200 <= len(big.t_sr) <= 1000
    d = merge([small, big])
    it = iteration.Iteration(d)
    it.launch(sw.default_opts(finish=False), cns.CnsParams(coverage=11.25))
    got = it.results()
    assert got[4].status == PR_ERR_CAPACITY
    params = {"coverage": "11.25", "use_ref_qual": "1", "detect_chimera": "0"}
    cases = consensus_cases(small, sam_for_tasks(small, "bwa-sr"), params)
    for c, g in zip(cases, got[:4]):
        want = ob.run_case(c)
        assert want["rc"] == 0 and g.status == 0, (c.name, g.status)
        assert (g.fastq, g.trace) == (want["fastq"], want["trace"]), c.name

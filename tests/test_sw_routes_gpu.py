"""Every route of the SW launcher (pr_sw_launch: sw_launch_extend / sw_launch_global in
csrc/sw_kernels.hip) and every option edge against the SW oracle, in single-seed mode.

Each case is a mixed batch of tests/sw_route_cases.py (directed reads + ~200 synthetic tasks,
7 + 3 long reads of 3 kb and more).  EVERY task is compared with ob.osw_task: bit-exact qb/qe/rb/re,
AS, truesc, POS, CIGAR and the -T pass flag.  Then the per-task route byte (sw.task_flags) is
held against what the oracle's results imply (retries, N hand-offs, CIGAR class), and the
routing rule (sw_route_cases.route) must show at least MIN_COUNT tasks in every kernel the row
names: a route that silently received nothing fails.  tests/test_sw_route_cases.py shows on
the CPU that the inputs can do that.

What the route byte can and cannot tell: it holds the retries, the N hand-offs and the CIGAR
class, so which rung of the ladder a task took is read back from the device.  Which kernel a
switch puts on that rung is not in the byte: under PRGPU_EXT80_LANE, PRGPU_PK_WIN,
PRGPU_PK_SPLIT / PRGPU_PK_BT_WIN and PRGPU_RING80_SIDE the kernel name in the asserted set is
inferred from the switch being set (the launcher reads each on every call, sw_api.cpp
pk_prepare / ring_side_z, sw_kernels.hip sw_launch_extend); what those tests read back is that
the rung received its tasks, and what they compare is every task's result."""
import ctypes as C

import numpy as np
import pytest

import sw_route_cases as rc
from sw_util import gpu_tuple

pytestmark = pytest.mark.gpu


CTX = []


@pytest.fixture(scope="module", autouse=True)
def own_context():
    """A context of the module's own, released at its end: the wide bands size the direction
    slabs by 4 w rows (15 GB at w = 100), which the suite's shared context would keep."""
    from proovread_amd import _abi
    CTX.append(_abi.Context())
    yield
    CTX.pop().close()


def launch(d, o, ctx=None):
    from proovread_amd import sw
    ctx = ctx or CTX[0]
    res = sw.run(d.sw_input(), rc.gpu_opts(o), ctx=ctx)
    return res, sw.task_flags(ctx)


def compare(d, tags, orc, res):
    assert res.n == len(orc) and (res["status"] == 0).all()
    bad = [(t, tags[t], tuple(w[0]), gpu_tuple(res, t)) for t, w in enumerate(orc) if tuple(w[0]) != gpu_tuple(res, t)]
    assert not bad, (len(bad), bad[:3])


def run_case(c, nopk=False, **kw):
    """Launch, compare every task, check the route bytes and the row's kernels."""
    res, flags = launch(c["d"], c["o"])
    compare(c["d"], c["tags"], c["orc"], res)
    pred = rc.predict_flags(c, nopk=nopk)
    off = np.nonzero((flags ^ pred) & rc.PREDICTED)[0]
    assert not len(off), [(int(t), c["tags"][t], hex(flags[t]), hex(pred[t])) for t in off[:5]]
    assert ((pred & 4) <= (flags & 4)).all()
    n = rc.route_counts(c, flags, nopk=nopk, **kw)
    want = rc.row_kernels(c["o"], c["qmax"], nopk=nopk, **kw)
    print(n)
    short = {k: n.get(k, 0) for k in want if n.get(k, 0) < rc.MIN_COUNT}
    assert not short, (short, n)
    if not rc.packed_on(c["o"], nopk):
        assert not [k for k in n if "_pk_" in k]
    return res, flags, n


IDS = ["%s-w%d%s" % (n, w, "-650bp" if lg else "") for n, w, lg in rc.SETS]


@pytest.mark.parametrize("name,w,long_reads", rc.SETS, ids=IDS)
def test_routes_by_band_and_scoring(name, w, long_reads):
    """The matrix: bands 8 .. 100 at the bwa-sr preset (packed extension and the <32>, <40>, <64>
    lane kernels, ext_wave, the wide kernel as retry and as first try, in LDS and in HBM form with
    650 bp reads, the ring-40 / ring-80 / general CIGAR kernels), and the scoring sets at w = 8,
    40 and 100 (bwa's defaults with the one-accumulator packed extension, a = 15 b = 16, a
    penalty of 32 against 33 -- packed against no packed route --, pen_clip 0 and 200, zdrop 0
    and 10)."""
    run_case(rc.case(name, w, long_reads))


def test_band_1000_is_accepted():
    from proovread_amd import _abi
    c = rc.case("sr", 1000)
    ctx = _abi.Context()   # (its slabs, sized by 4 w rows, go with it)
    try:
        res, flags = launch(c["d"], c["o"], ctx)
    finally:
        ctx.close()
    compare(c["d"], c["tags"], c["orc"], res)
    n = rc.route_counts(c, flags)
    assert n.get("sw_ext_wide_kernel<false>@0", 0) >= rc.MIN_COUNT, n


@pytest.mark.parametrize("name,w", rc.TWINS)
def test_zdrop0_twin(name, w):
    """The same reads under zdrop 0: the ones that stop on z-drop in the set's own run (asserted
    there) go on to the read end here (test_sw_route_cases.test_zdrop0_twin_changes_the_stopped_reads)."""
    tw = rc.zdrop0_twin(rc.case(name, w))
    res, flags = launch(tw["d"], tw["o"])
    compare(tw["d"], tw["tags"], tw["orc"], res)


@pytest.mark.parametrize("w", [33, 40])
def test_ext80_lane_switch(w, monkeypatch):
    """PRGPU_EXT80_LANE=1: the second band (66, 80) one task per lane, sw_ext_phase_kernel<80>."""
    monkeypatch.setenv("PRGPU_EXT80_LANE", "1")
    res, flags, n = run_case(rc.case("sr", w), ext80_lane=True)
    assert "sw_ext_wave_kernel@1" not in n


PRESETS = [("sr", 40), ("finish", 30)]


@pytest.mark.parametrize("name,w", PRESETS)
@pytest.mark.parametrize("bt", [4, 8, 16])
def test_split_cigar_path(name, w, bt, monkeypatch):
    """PRGPU_PK_SPLIT=1: sw_global_pk_kernel<40,16> DP launches, then sw_global_pk_bt_kernel<4|8|16>."""
    monkeypatch.setenv("PRGPU_PK_SPLIT", "1")
    monkeypatch.setenv("PRGPU_PK_BT_WIN", str(bt))
    run_case(rc.case(name, w), split=True, bt_win=bt)


def test_split_cigar_path_in_several_chunks(monkeypatch):
    """A slab budget of 1 MB: chunks of 64 segments, and the batch has more than 64 keys
    (test_sw_route_cases.test_split_chunks_batch_has_more_than_64_keys), so several chunks."""
    monkeypatch.setenv("PRGPU_PK_SPLIT", "1")
    monkeypatch.setenv("PRGPU_PK_SLAB_GB", "0.001")
    run_case(rc.case("sr", 40), split=True, bt_win=8)


@pytest.mark.parametrize("name,w", PRESETS)
def test_fused_window_16(name, w, monkeypatch):
    monkeypatch.setenv("PRGPU_PK_WIN", "16")
    run_case(rc.case(name, w), pk_win=16)


@pytest.mark.parametrize("name,w", PRESETS)
def test_ring80_on_the_main_stream(name, w, monkeypatch):
    monkeypatch.setenv("PRGPU_RING80_SIDE", "0")
    res, flags, n = run_case(rc.case(name, w))
    assert n["sw_global_ring_kernel<80>"] >= rc.MIN_COUNT


@pytest.mark.parametrize("name,w", PRESETS)
def test_no_packed_kernels_switch(name, w, monkeypatch):
    """PRGPU_SW_NOPK=1: everything through the ring and the general kernels."""
    monkeypatch.setenv("PRGPU_SW_NOPK", "1")
    run_case(rc.case(name, w), nopk=True)


@pytest.mark.parametrize("which", rc.FRAME_EDGES)
def test_frame_edges(which):
    """Perfect-match reads whose score fills a frame: 511 under the one-accumulator packed
    extension, 2040 / 2043 inside and 2052 outside the packed frame in one batch, 8190 under
    the 13-bit DP words; the scores asserted exactly."""
    o, d, tags, scores = rc.frame_edge(which)
    orc = rc.oracle_all(d, o)
    res, flags = launch(d, o)
    compare(d, tags, orc, res)
    lq = np.diff(d.sr_off)
    for t, g in enumerate(tags):
        if g in scores:
            assert int(res["score"][t]) == scores[g] and int(res["truesc"][t]) == scores[g]
            assert (int(res["qb"][t]), int(res["qe"][t])) == (0, int(lq[d.t_sr[t]]))
    c = dict(o=o, d=d, tags=tags, orc=orc, qmax=int(lq.max()))
    n = rc.route_counts(c, flags)
    print(n)
    pk_t, pk_f = n.get("sw_ext_pk_kernel<40,true>", 0), n.get("sw_ext_pk_kernel<40,false>", 0)
    if which.startswith("smallh"):
        assert pk_t >= rc.MIN_COUNT and not pk_f
    elif which == "w8190":
        assert not pk_t and n["sw_ext_phase_kernel<40>@0"] >= rc.MIN_COUNT
    else:
        assert pk_f >= rc.MIN_COUNT and not pk_t
    if which == "pk2047":   # the 228 bp reads (2052) leave the packed extension, their neighbours do not
        for t, g in enumerate(tags):
            r = rc.route(int(flags[t]), o, c["qmax"], int(lq[d.t_sr[t]]), int(d.t_qbeg[t]), int(d.t_slen[t]), res=orc[t][0],
                         wreg=orc[t][1])
            if g == "perfect_228":
                assert not [k for k in r if k.startswith("sw_ext_pk")]
            if g == "perfect_227":
                assert not [k for k in r if k.startswith("sw_ext_phase")]
        assert n["sw_ext_phase_kernel<40>@0"] >= rc.MIN_COUNT


def test_refusals_leave_the_context_usable():
    from proovread_amd import sw
    c = rc.case("sr", 40)

    def good():
        res, flags = launch(c["d"], c["o"])
        compare(c["d"], c["tags"], c["orc"], res)

    def refused(d, o, msg):
        good()
        with pytest.raises(RuntimeError, match=msg):
            sw.run(d.sw_input(), rc.gpu_opts(o), ctx=CTX[0])
        good()

    d547, _ = rc.perfect(16, [(547, None, None)] * 2 + [(100, None, None)] * 4)
    d546, t546 = rc.perfect(16, [(546, None, None)] * 2 + [(100, None, None)] * 4)
    refused(d547, rc.scoring("a15", 40), "below 8192")            # 15 * 547 = 8205
    o = rc.scoring("a15", 40)
    res, _ = launch(d546, o)                                       # 15 * 546 = 8190 is accepted
    compare(d546, t546, rc.oracle_all(d546, o), res)
    refused(c["d"], rc.make_opts(a=16, b=16), "match score > 15")
    refused(c["d"], rc.make_opts(a=5, b=17), "mismatch penalty > 16")
    refused(c["d"], rc.make_opts(w=1001), "w > 1000")
    refused(c["d"], rc.make_opts(w=0), "bad scoring options")


def test_task_flags_needs_a_single_seed_launch():
    from proovread_amd import _abi, seed, sw, synth
    ctx = CTX[0]
    L = _abi.lib()
    c = rc.case("sr", 40)
    inp = c["d"].sw_input()
    b = inp.c_batch()
    _abi.check(L.pr_sw_upload(ctx.h, C.byref(b)), "pr_sw_upload")
    with pytest.raises(RuntimeError, match="launch"):
        sw.task_flags(ctx)                                         # uploaded, not launched
    sw.run(inp, rc.gpu_opts(c["o"]), ctx=ctx)
    n = len(c["d"].t_sr)
    buf = np.zeros(n, np.uint8)
    assert L.pr_sw_task_flags(ctx.h, _abi.ptr(buf, C.c_uint8), n - 1) == -1   # PR_ERR_ARG: not the task count
    assert len(sw.task_flags(ctx)) == n
    d = synth.simulate(21, 20000, 6, 2000, 4)
    ix = seed.SeedIndex(d.lr_seq, d.lr_off)
    db = synth.with_seeds(d, ix.map(d.sr_seq, d.sr_off, seed.default_opts(False), threads=4))
    ix.close()
    sw.run(db.sw_input(), sw.default_opts(finish=False), ctx=ctx)
    with pytest.raises(RuntimeError, match="bwa mode"):
        sw.task_flags(ctx)                                         # bwa mode refills the byte per round

"""CPU: the directed SW route cases (tests/sw_route_cases.py) against the oracle alone.

Conditions on the inputs, so that no GPU comparison passes by having nothing to compare:
every set shows what it exists for at least MIN_COUNT times in the oracle's own results
(retries on the left, the right and both; a last CIGAR band <= 40, 41 to 80, > 80; clipped
and to-end outcomes on both ends; the tie gscore == score - pen_clip; a z-drop stop; -T pass
0 and 1), and the flags those results imply send MIN_COUNT tasks to every kernel the set's
row names.  Also the routing rule itself on hand-made flag bytes."""
import numpy as np
import pytest

import sw_route_cases as rc

IDS = ["%s-w%d%s" % (n, w, "-650bp" if lg else "") for n, w, lg in rc.SETS]


@pytest.mark.parametrize("name,w,long_reads", rc.SETS, ids=IDS)
def test_set_shows_what_it_exists_for(name, w, long_reads):
    c = rc.case(name, w, long_reads)
    tr = rc.case_trace(c)
    # the per-side trace restates mem_chain2aln: it must land on osw_task's region
    bad = [t for t, ((sd, reg), (res, wreg, w2)) in enumerate(zip(tr, c["orc"])) if reg != (res[0], res[1], res[4])]
    assert not bad, bad[:5]
    n = rc.count_features(tr, c["orc"])
    want = rc.features(name, w)
    print(name, w, n)
    short = {k: n[k] for k in want if n[k] < rc.MIN_COUNT}
    assert not short, (short, n)
    if long_reads:
        assert c["qmax"] == 650


@pytest.mark.parametrize("name,w,long_reads", rc.SETS, ids=IDS)
def test_set_reaches_every_kernel_of_its_row(name, w, long_reads):
    c = rc.case(name, w, long_reads)
    n = rc.route_counts(c, rc.predict_flags(c))
    want = rc.row_kernels(c["o"], c["qmax"])
    print(name, w, n)
    short = {k: n.get(k, 0) for k in want if n.get(k, 0) < rc.MIN_COUNT}
    assert not short, (short, n)
    if not rc.packed_on(c["o"]):
        assert not [k for k in n if "_pk_" in k]


@pytest.mark.parametrize("name,w", rc.TWINS)
def test_zdrop0_twin_changes_the_stopped_reads(name, w):
    """The z-drop reads of a set, run again with zdrop 0, come out differently (they reach the
    read end): a kernel that ignored zdrop, or always applied it, fails one of the two runs."""
    c = rc.case(name, w)
    tw = rc.zdrop0_twin(c)
    diff = [t for t, (x, y) in enumerate(zip(c["orc"], tw["orc"])) if x[0] != y[0]]
    assert len([t for t in diff if c["tags"][t].startswith("zdrop")]) >= rc.MIN_COUNT, len(diff)
    for t in diff:   # with zdrop 0 the read goes further
        assert tw["orc"][t][0][1] - tw["orc"][t][0][0] >= c["orc"][t][0][1] - c["orc"][t][0][0]


def test_no_draw_is_left_unmet():
    """Hardly any directed read is dead weight: at most 3 per set carry the builder's '?' (no
    draw met its condition; the counts of test_set_shows_what_it_exists_for hold without them),
    except for a feature the set's options rule out (rc.features)."""
    why = {"lowscore": "pass0", "indel": "retry_LR"}
    for name, w, lg in rc.SETS:
        f = rc.features(name, w)
        unmet = [g for g in rc.case(name, w, lg)["tags"] if g.endswith("?") and why[g.split("_")[0].rstrip("?")] in f]
        assert len(unmet) <= 3, (name, w, lg, unmet)


def test_rows_name_every_kernel_instantiation():
    """Every instantiation sw_launch_extend / sw_launch_global can launch is in some row's set
    (the switch-selected ones with their switch)."""
    got = set()
    for name, w, lg in rc.SETS:
        c = rc.case(name, w, lg)
        got |= {k.split("@")[0] for k in rc.row_kernels(c["o"], c["qmax"])}
    c = rc.case("sr", 40)
    got |= {k.split("@")[0] for k in rc.row_kernels(c["o"], c["qmax"], ext80_lane=True)}
    got |= rc.row_kernels(c["o"], c["qmax"], pk_win=16)
    for bt in (4, 8, 16):
        got |= rc.row_kernels(c["o"], c["qmax"], split=True, bt_win=bt)
    want = {"sw_ext_pk_kernel<40,true>", "sw_ext_pk_kernel<40,false>", "sw_ext_phase_kernel<32>",
            "sw_ext_phase_kernel<40>", "sw_ext_phase_kernel<64>", "sw_ext_phase_kernel<80>", "sw_ext_wave_kernel",
            "sw_ext_wide_kernel<false>", "sw_ext_wide_kernel<true>", "sw_global_pk_kernel<40,8>",
            "sw_global_pk_kernel<40,16>", "sw_global_pk_bt_kernel<4>", "sw_global_pk_bt_kernel<8>",
            "sw_global_pk_bt_kernel<16>", "sw_global_ring_kernel<40>", "sw_global_ring_kernel<80>",
            "sw_global_kernel<false>", "sw_global_kernel<true>"}
    assert want <= got, want - got


def test_route_rule_on_hand_made_flags():
    o = rc.scoring("sr", 40)
    pk, ring = "sw_ext_pk_kernel<40,false>", "sw_ext_phase_kernel<40>@0"
    assert rc.route(0, o, 150, 150, 60, 20) == [pk, pk, "sw_global_pk_kernel<40,8>"]
    assert rc.route(0, o, 150, 150, 0, 150) == ["sw_global_pk_kernel<40,8>"]            # all seed
    assert rc.route(0x40, o, 150, 150, 0, 20) == [pk, "sw_global_ring_kernel<40>"]       # left side empty
    assert rc.route(0x08 | 0x02 | 0x80, o, 150, 150, 60, 20) == [pk, ring, pk, "sw_ext_wave_kernel@1",
                                                                  "sw_global_ring_kernel<80>"]
    assert rc.route(0x02, o, 150, 150, 60, 20, ext80_lane=True)[2] == "sw_ext_phase_kernel<80>@1"
    # a * lq > 2047 (lq 410) or a side longer than 255 leaves the packed extension
    assert rc.route(0, o, 410, 410, 100, 20)[:2] == [ring, ring]
    assert rc.route(0, o, 400, 400, 300, 20)[:2] == [ring, pk]
    # one-accumulator row maximum while a * qmax <= 511
    assert rc.route(0, rc.scoring("bwa", 40), 511, 100, 40, 20)[0] == "sw_ext_pk_kernel<40,true>"
    assert rc.route(0, rc.scoring("bwa", 40), 512, 100, 40, 20)[0] == "sw_ext_pk_kernel<40,false>"
    # bands: 41 has no packed extension; 65 .. 80 one task per wave; above 80 the wide kernel,
    # its row in HBM once the general kernel's (qmax >= 510) or its own (qmax >= 638) outgrows the LDS
    assert rc.route(0x01, rc.scoring("sr", 41), 150, 150, 60, 20)[:3] == [
        "sw_ext_phase_kernel<64>@0", "sw_ext_wide_kernel<false>@1", "sw_ext_phase_kernel<64>@0"]
    assert rc.route(0, rc.scoring("sr", 65), 150, 150, 60, 20)[0] == "sw_ext_wave_kernel@0"
    assert rc.route(0, rc.scoring("sr", 81), 509, 150, 60, 20)[0] == "sw_ext_wide_kernel<false>@0"
    assert rc.route(0, rc.scoring("sr", 81), 510, 150, 60, 20)[0] == "sw_ext_wide_kernel<true>@0"
    assert not rc.eh_hbm(509, 40) and rc.eh_hbm(510, 40) and rc.eh_hbm(638, 41)
    # a penalty of 33 switches the packed kernels off; the class then comes from the region
    o33 = rc.scoring("pen33", 40)
    res = (0, 150, 100, 250, 750, 750, 100, "150M", 1)
    assert rc.route(0, o33, 150, 150, 60, 20, res=res, wreg=40) == [ring, ring, "sw_global_ring_kernel<40>"]
    assert rc.route(0x24, o, 150, 150, 0, 150)[-2:] == ["sw_global_kernel<false>", "sw_global_kernel<false>@overflow"]


@pytest.mark.parametrize("which", rc.FRAME_EDGES)
def test_frame_edge_batches(which):
    o, d, tags, scores = rc.frame_edge(which)
    lq = np.diff(d.sr_off)
    for tag, sc in scores.items():
        ts = [t for t, g in enumerate(tags) if g == tag]
        assert len(ts) >= rc.MIN_COUNT
        assert all(o.a * int(lq[d.t_sr[t]]) == sc for t in ts)
    orc = rc.oracle_all(d, o)
    for t, g in enumerate(tags):
        if g in scores:   # a perfect match scores a * lq, end to end
            assert orc[t][0][4] == scores[g] and orc[t][0][:2] == (0, int(lq[d.t_sr[t]]))
    qmax = int(lq.max())
    if which.startswith("smallh"):
        assert o.a * qmax == 511
    if which == "smallh1":   # both sides of the 511 bp reads inside the packed extension
        assert all(max(int(d.t_qbeg[t]), 511 - int(d.t_qbeg[t]) - int(d.t_slen[t])) <= 255
                   for t, g in enumerate(tags) if g == "perfect_511")
    if which == "w8190":
        assert o.a * qmax == 8190 < 8192


def test_split_chunks_batch_has_more_than_64_keys():
    """PRGPU_PK_SLAB_GB=0.001 splits the packed CIGAR pass into chunks of 64 segments at the
    least, and every key (band, qe - qb) has a segment of its own: the preset case has more
    than 64 distinct qe - qb among the tasks the packed kernel takes, in the oracle's results."""
    c = rc.case("sr", 40)
    keys = {rc.pk_cigar_key(c["o"], res, wreg) for res, wreg, w2 in c["orc"]} - {-1}
    assert len({k & 255 for k in keys}) > 64, len(keys)


def test_pool_edge_seeds_sit_at_the_pool_ends():
    """Seeds within 12 bases of the first base of the pool's first long read and of the last
    base of its last long read, on both strands, with the read hanging over the edge."""
    c = rc.case("sr", 40)
    d = c["d"]
    L = np.diff(d.lr_off)
    for lr, tag in ((0, "edge_lo"), (d.n_lr - 1, "edge_hi")):
        for st in (0, 1):   # (a reverse-strand seed near the strand's other end is near the same forward base)
            ts = [t for t, g in enumerate(c["tags"]) if g.startswith("edge") and d.t_lr[t] == lr and d.t_strand[t] == st]
            near_first = [t for t in ts if (d.t_rbeg[t] if st == 0 else L[lr] - d.t_rbeg[t] - d.t_slen[t]) < 12]
            near_last = [t for t in ts if (L[lr] - d.t_rbeg[t] - d.t_slen[t] if st == 0 else d.t_rbeg[t]) < 12]
            assert len(near_first if lr == 0 else near_last) >= 3, (lr, st)

"""bwa mode (extension rounds, mem_patch_reg, the CIGAR pass over the reported alignments) on
the launcher's non-preset routes and under its switches, against oracle/aln_oracle.c read by
read (tests/test_aln_gpu.py's comparison with an explicit option tuple): -w 8 (the <32> lane
kernel in both tries under the packed extension), -w 100 (sw_ext_wide_kernel in every round),
a gap penalty of 33 (no packed kernel), PRGPU_ALN_NO_HPREV, PRGPU_BWA_NO_EARLY_FINAL, and
PRGPU_ALN_LANE=1 (every read on the lane kernels), which the library reads once per process:
a child process runs it (tests/sw_bwa_child.py) and the parent compares its arrays."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "oracle"))


@functools.lru_cache(maxsize=None)
def bwa_data(finish):
    from proovread_amd import seed, synth
    f = 0.02 / 0.15 if finish else 1.0   # finish's -T 4 per base needs long reads corrected to ~2 % error
    d = synth.simulate(141 + int(finish), 20000, 12, 2000, 8, p_ins=0.09 * f, p_del=0.045 * f, p_sub=0.015 * f)
    rng = np.random.default_rng(9)
    lr = d.lr_seq.copy()
    for i in range(d.n_lr):   # N windows: colinear regions for mem_patch_reg
        for x in range(int(d.lr_off[i]) + 100, int(d.lr_off[i + 1]) - 200, 300):
            x += int(rng.integers(0, 100))
            lr[x:x + int(rng.integers(10, 111))] = 4
    d.lr_seq = lr
    ix = seed.SeedIndex(d.lr_seq, d.lr_off)
    d = synth.with_seeds(d, ix.map(d.sr_seq, d.sr_off, seed.default_opts(finish), threads=4))
    ix.close()
    return d


def by_read(a, n, d):
    out = {}
    for i in range(n):
        t = int(a["task"][i])
        assert a["status"][i] == 0
        cg = a["cigar"][int(a["cigar_off"][i]):int(a["cigar_off"][i + 1])]
        out.setdefault(int(d.t_sr[t]), []).append(
            (int(d.t_lr[t]), int(d.t_strand[t]), int(a["pos"][i]), [int(x) for x in cg], int(a["score"][i]),
             int(a["flag"][i]), int(a["qb"][i]), int(a["qe"][i]), int(a["rb"][i]), int(a["re"][i]), int(a["truesc"][i]), t))
    return out


@functools.lru_cache(maxsize=None)
def oracle(finish, swt):
    import cpu_chain
    from proovread_amd import sw
    return cpu_chain.bwa_alignments(bwa_data(finish), swt, drop_ratio=sw.default_opts(finish).drop_ratio)


def tuple_of(o):
    return (o.a, o.b, o.o_del, o.o_ins, o.e_del, o.e_ins, o.w, o.pen_clip5, o.pen_clip3, o.zdrop, o.min_score_per_base)


def check(a, n, d, want):
    got = by_read(a, n, d)
    bad = [r for r in range(d.n_sr) if got.get(r, []) != want[r]]
    assert not bad, (len(bad), bad[:3], got.get(bad[0]), want[bad[0]])
    assert n == sum(len(v) for v in want) > 5 * d.n_lr


def run_here(finish, **over):
    from proovread_amd import _abi, sw
    d = bwa_data(finish)
    o = sw.default_opts(finish)
    for k, v in over.items():
        setattr(o, k, v)
    ctx = _abi.default_context()
    res = sw.run(d.sw_input(), o, ctx=ctx)
    rounds, n_ext, n_patch = sw.bwa_stats(ctx)
    print(f"rounds {rounds} extended {n_ext} patches {n_patch}")
    check(res.a, res.n, d, oracle(finish, tuple_of(o)))
    assert rounds >= 1 and n_ext > 0
    return rounds, n_ext, n_patch


@pytest.mark.gpu
@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("over", [dict(w=8), dict(w=100), dict(o_del=33)], ids=["w8", "w100", "pen33"])
def test_bwa_mode_off_preset_routes(finish, over):
    run_here(finish, **over)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["PRGPU_ALN_NO_HPREV", "PRGPU_BWA_NO_EARLY_FINAL"])
def test_bwa_mode_switches(switch, monkeypatch):
    monkeypatch.setenv(switch, "1")
    run_here(False)


CHILD_DOWN = []   # why the child-based tests stopped starting GPU processes


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"PRGPU_ALN_LANE": "1"}, {"PRGPU_ALN_LANE": "1", "PRGPU_ALN_NO_HPREV": "1"}],
                         ids=["lane", "lane-no-hprev"])
def test_bwa_mode_lane_kernels_in_a_fresh_process(env, tmp_path):
    if CHILD_DOWN:
        pytest.skip("an earlier child process " + CHILD_DOWN[0])
    out = tmp_path / "r.npz"
    try:
        p = subprocess.run([sys.executable, str(HERE / "sw_bwa_child.py"), str(out)], env={**os.environ, **env},
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        CHILD_DOWN.append("ran into its timeout")
        raise
    if p.returncode < 0:
        CHILD_DOWN.append("ended on signal %d" % -p.returncode)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    a = np.load(out)
    d = bwa_data(False)
    check(a, int(a["n"]), d, oracle(False, tuple_of(__import__("oracle_bind").sw_opts("bwa-sr"))))
    assert a["stats"][1] > 0

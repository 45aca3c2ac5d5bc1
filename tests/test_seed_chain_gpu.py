"""seed_chain_kernel on the GPU: pr_seed_gpu_map with the lane phase stopping after the SMEMs and the
reads chained on chip (the default) = the same map with every read chained by its lane
(PRGPU_SEED_CHAIN=lane) = the host path pr_seed_map, array-equal and no read flagged, on
seed_chain_cases' text: reads at cap - 1, cap and cap + 1 of the seeds and the ranges of both of
the kernel's geometries (the first geometry's cap + 1 reads come back through the second, the
second's through pass 2: the pass counters show it), more than 64 ranges in one read, one range with every occurrence,
chains of equal pos, tied weights, an N, reads below 12 bases, no SMEM, an empty read, one read of
mr length in the batch (the lane path) and a last wave that is partly filled."""
import numpy as np
import pytest

import seed_chain_cases as cases
from proovread_amd import seed

pytestmark = pytest.mark.gpu

# the kernel's geometries (seed_chain.h ChainLdsSmall / ChainLdsLarge): seeds, ranges
GEOMETRIES = [(512, 256), (1536, 1024)]


@pytest.fixture(scope="module")
def setup():
    from proovread_amd import _abi
    data = cases.build(GEOMETRIES)
    ix = seed.SeedIndex(data[0], data[1])
    ix.to_gpu(_abi.default_context())
    return ix, data


def run(ix, data, o, monkeypatch, lane):
    # the families' reads have ~500 hits for every start: pass 1's slices hold them (the hook's
    # hits, intervals, SMEMs, seeds, chains), so that they reach the chaining kernel
    monkeypatch.setenv("PRGPU_SEED_SMALL", "65536,64,512,2048,2048")
    if lane:
        monkeypatch.setenv("PRGPU_SEED_CHAIN", "lane")
    else:
        monkeypatch.delenv("PRGPU_SEED_CHAIN", raising=False)
    got, st = ix.map_gpu(data[2], data[3], o, allow_flagged=True)
    passes = ix.phase_ms()["pass_reads"]   # reads mapped again by pass 1b / pass 2 / the later passes
    monkeypatch.delenv("PRGPU_SEED_CHAIN", raising=False)
    return got, st, passes


@pytest.mark.parametrize("which", ["bwa-sr", "finish", "c20"])
def test_chain_kernel_equals_lane_path_and_host_path(setup, monkeypatch, which):
    ix, data = setup
    o = seed.default_opts(which == "finish")
    if which == "c20":
        o.max_occ = 20   # every 3rd occurrence of the repeated segments' SMEMs
    want = ix.map(data[2], data[3], o, threads=8)
    new, nst, new_passes = run(ix, data, o, monkeypatch, lane=False)
    old, ost, old_passes = run(ix, data, o, monkeypatch, lane=True)
    assert not nst.any() and not ost.any()
    assert np.array_equal(new, old)
    assert np.array_equal(new, want)
    assert len(want) > 3000
    labels = data[4]
    n_by_read = np.bincount(new["sr"], minlength=len(data[3]) - 1)
    if which == "bwa-sr":
        for ci, (sc, rc) in enumerate(GEOMETRIES):
            for k in (-1, 0, 1):   # every seed of the edge reads is a task (-D 0, weights >= -W)
                assert n_by_read[labels[f"seeds{k:+d}.{ci}"]] == sc + k
                assert n_by_read[labels[f"ranges{k:+d}.{ci}"]] == rc + k   # (one seed a range)
        # the second geometry's cap + 1 reads (1,537 seeds; 1,025 ranges) left the chaining kernel
        # and came back through pass 2; the lane path's slices (the hook's 2,048) hold them
        assert new_passes["pass2"] >= old_passes["pass2"] + 2, (new_passes, old_passes)
        assert n_by_read[labels["mr_length"]] > 0
        for name in ("short", "short11", "no_smem", "empty", "all_n"):
            assert n_by_read[labels[name]] == 0

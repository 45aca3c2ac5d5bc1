"""seed_chain_kernel's -D pass on the GPU with kept lists beyond one and two steps of 64: the finish
options with mask_level 0.99 on seed_chain_cases' text, where a read of one repeated 24-mer keeps a
chain for every copy (255 to 257 of them in the first geometry, 1,023 to 1,025 in the second: the
kept list's first 64 entries in registers, the later ones in LDS) and the noisy reads over the
repeated unit drop chains.  pr_seed_gpu_map with the reads chained on chip (the default) = the
same with every read chained by its lane (PRGPU_SEED_CHAIN=lane) = the host path pr_seed_map,
array-equal, no read flagged.  The batch's last wave is partly filled, and two reads of 18 and 20
exact bases hand over a single position."""
import numpy as np
import pytest

import seed_chain_cases as cases
from proovread_amd import seed

pytestmark = pytest.mark.gpu

GEOMETRIES = [(512, 256), (1536, 1024)]


@pytest.fixture(scope="module")
def setup():
    from proovread_amd import _abi
    lr_seq, lr_off, sr_seq, sr_off, labels = cases.build(GEOMETRIES)
    # two short exact reads from the first (random) long read: one SMEM, one position
    extra = [lr_seq[500:518], lr_seq[900:920]]
    labels = dict(labels, single18=len(sr_off) - 1, single20=len(sr_off))
    sr_seq = np.concatenate([sr_seq] + extra).astype(np.uint8)
    sr_off = np.concatenate([sr_off, sr_off[-1] + np.cumsum([len(x) for x in extra])]).astype(np.int64)
    ix = seed.SeedIndex(lr_seq, lr_off)
    ix.to_gpu(_abi.default_context())
    o = seed.default_opts(True)
    assert o.drop_ratio == 0.75
    o.mask_level = 0.99
    want = ix.map(sr_seq, sr_off, o, threads=8)
    o0 = seed.default_opts(True)   # the same without -D: every chain past -W kept
    o0.mask_level = 0.99
    o0.drop_ratio = 0.0
    all_chains = ix.map(sr_seq, sr_off, o0, threads=8)
    return ix, (sr_seq, sr_off, labels), o, want, all_chains


def run(ix, sr, o, monkeypatch, lane):
    monkeypatch.setenv("PRGPU_SEED_SMALL", "65536,64,512,2048,2048")   # (as test_seed_chain_gpu.py)
    if lane:
        monkeypatch.setenv("PRGPU_SEED_CHAIN", "lane")
    else:
        monkeypatch.delenv("PRGPU_SEED_CHAIN", raising=False)
    got, st = ix.map_gpu(sr[0], sr[1], o, allow_flagged=True)
    monkeypatch.delenv("PRGPU_SEED_CHAIN", raising=False)
    return got, st


def chains_by_read(tasks, n):
    out = np.zeros(n, np.int64)
    np.maximum.at(out, tasks["sr"], tasks["chain"] + 1)
    return out


def test_long_kept_lists_equal_lane_path_and_host_path(setup, monkeypatch):
    ix, sr, o, want, all_chains = setup
    n = len(sr[1]) - 1
    labels = sr[2]
    assert n % 64 not in (0, 63)   # the last wave partly filled
    kept = chains_by_read(want, n)
    every = chains_by_read(all_chains, n)
    # the cases are there, by the host path: kept lists past 64 and past 128 entries within the
    # first geometry and past 1,000 in the second, reads that lost chains to -D, single positions
    first = kept[[labels[f"ranges{k:+d}.0"] for k in (-1, 0)]]
    assert (first > 128).all() and (first <= 256).all(), first
    assert (kept > 64).sum() >= 6 and (kept > 128).sum() >= 6, np.sort(kept)[-12:]
    assert kept[labels["ranges+0.1"]] > 1000
    assert ((kept < every) & (kept > 0)).sum() >= 5, (kept < every).sum()
    assert kept[labels["single18"]] == 1 and kept[labels["single20"]] == 1
    new, nst = run(ix, sr, o, monkeypatch, lane=False)
    old, ost = run(ix, sr, o, monkeypatch, lane=True)
    assert not nst.any() and not ost.any()
    assert np.array_equal(new, want)
    assert np.array_equal(old, want)

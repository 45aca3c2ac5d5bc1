"""The task sample gathered on the device (seed_api.cpp gather_ranges: the record ranges' bytes,
adjacent ranges merged, copied by one kernel): pr_seed_gpu_map_sampled over record ranges of the
resident short reads gives the seeds of pr_seed_gpu_map over the same reads gathered on the host
(ShortReads.gather).  Reads of 149 / 150 / 151 bases, so the ranges' byte offsets are odd and the
source and destination alignments differ from range to range."""
import ctypes as C
import functools

import numpy as np
import pytest

from proovread_amd import seed, synth


@functools.lru_cache(maxsize=1)
def _case():
    d = synth.simulate(31, 120_000, 120, 5000, 12.0)
    n = 6000
    assert d.n_sr >= n
    sr = d.sr_seq[:d.sr_off[n]].reshape(n, 150)
    lens = 149 + (np.arange(n) * 7 + 3) % 3   # 149, 150, 151 mixed
    lens[:3] = (149, 151, 149)
    pool = np.concatenate([np.concatenate([r, r[:1]])[:l] for r, l in zip(sr, lens)]).astype(np.uint8)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return d, pool, off


CASES = {
    "single range": [(100, 1700)],
    "whole set": [(0, 6000)],
    "adjacent ranges": [(10, 300), (300, 301), (301, 1500), (2000, 2600), (2600, 3111)],
    "an empty range in the middle": [(5, 700), (900, 900), (1501, 2202)],
    "ranges of one read": [(0, 1), (1, 2), (7, 8), (4000, 4001), (5998, 5999)],
    "odd byte offsets": [(1, 650), (651, 1302), (1303, 1304), (3001, 3653)],
    "the last read of the set": [(3, 404), (5999, 6000)],
    "many ranges": [(k * 40, k * 40 + 1 + k % 29) for k in range(150)],
}


@pytest.mark.gpu
def test_sampled_map_equals_map_of_host_gathered_reads():
    from proovread_amd import _abi, correct, iteration
    d, pool, off = _case()
    ctx = _abi.default_context()
    L = _abi.lib()
    iteration._setup(L)
    seed._setup(L)
    L.pr_seed_gpu_seeds.argtypes = [C.c_void_p, C.POINTER(seed.SeedTasks)]
    srs = correct.ShortReads.from_pool(pool, off)
    _abi.check(L.pr_srset_load(ctx.h, len(off) - 1, _abi.ptr(off, C.c_int64), _abi.ptr(pool, C.c_uint8)), "pr_srset_load")
    ix = seed.DeviceSeedIndex(ctx, d.lr_seq, d.lr_off)
    o = seed.default_opts(False)
    for name, ranges in CASES.items():
        rg = np.ascontiguousarray(ranges, np.int64).reshape(-1, 2)
        lens = np.concatenate([off[a + 1:b + 1] - off[a:b] for a, b in rg])
        so = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=so[1:])
        ss = srs.gather(rg)
        assert len(ss) == so[-1], name
        want, wst = ix.map(ss, so, o)
        st = np.full(len(lens), -1, np.int32)
        _abi.check(L.pr_seed_gpu_map_sampled(ctx.h, C.byref(o), _abi.ptr(rg, C.c_int64), len(rg), _abi.ptr(st, C.c_int32)),
                   "pr_seed_gpu_map_sampled")
        out = seed.SeedTasks()
        _abi.check(L.pr_seed_gpu_seeds(ctx.h, C.byref(out)), "pr_seed_gpu_seeds")
        got = seed._take(L, out)
        assert not wst.any() and np.array_equal(st, wst), name
        assert len(want) > 0, name
        assert np.array_equal(got, want), name


@pytest.mark.gpu
def test_sampled_map_refuses_ranges_outside_the_set():
    from proovread_amd import _abi, iteration
    d, pool, off = _case()
    ctx = _abi.default_context()
    L = _abi.lib()
    iteration._setup(L)
    seed._setup(L)
    _abi.check(L.pr_srset_load(ctx.h, len(off) - 1, _abi.ptr(off, C.c_int64), _abi.ptr(pool, C.c_uint8)), "pr_srset_load")
    seed.DeviceSeedIndex(ctx, d.lr_seq, d.lr_off)
    o = seed.default_opts(False)
    st = np.zeros(16, np.int32)
    for bad in ([(0, 6001)], [(-1, 4)], [(9, 3)]):
        rg = np.ascontiguousarray(bad, np.int64)
        assert L.pr_seed_gpu_map_sampled(ctx.h, C.byref(o), _abi.ptr(rg, C.c_int64), len(rg), _abi.ptr(st, C.c_int32)) != 0

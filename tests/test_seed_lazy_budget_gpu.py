"""Pass 1's hit budget and pass 1b's batch size on the GPU (seed_batch_kernel<true>, seed_plan.h
pass1b_batch): the near-exact setting of test_seed_gpu.py's pass-1b cases with the finish
options (the lazy occurrence table) and a mixed read set, 24,000 reads of which 20,000 carry
10 % substitutions.  With a budget of 512 hits pass 1 flags most of the noisy reads (more than
the 16,384 a lane-per-read pass 1b needs), pass 1b maps them with slices sized from the need
they report, and nothing is left for a later pass."""
import functools

import numpy as np
import pytest

from proovread_amd import seed, synth

BUDGET = 512


@functools.lru_cache(maxsize=1)
def _case():
    """-> the index, reads, the host path's seeds, the reads pass 1 flags at BUDGET (host emulation)."""
    d = synth.simulate(17, 150_000, 1400, 5000, 40.0, p_ins=0.002, p_del=0.002, p_sub=0.002, sr_frac=0.6)
    n = 24000
    assert d.n_sr >= n
    sr = d.sr_seq[:d.sr_off[n]].reshape(n, 150).copy()
    rng = np.random.default_rng(5)
    noisy = np.arange(n) % 6 != 0
    sub = (rng.random(sr.shape) < 0.10) & noisy[:, None]
    sr[sub] = (sr[sub] + rng.integers(1, 4, int(sub.sum())).astype(np.uint8)) % 4
    ix = seed.SeedIndex(d.lr_seq, d.lr_off)
    o = seed.default_opts(True)
    _, st, _ = ix.map_device_pass1(sr.reshape(-1), np.arange(n + 1, dtype=np.int64) * 150, o, budget=BUDGET)
    # a flagged count that no tested batch size above 1 divides: the last dequeue is a partial one
    flagged = np.cumsum(st != 0)
    while flagged[n - 1] % 16 == 0 or flagged[n - 1] % 63 == 0:
        n -= 1
    ss, so = sr[:n].reshape(-1), np.arange(n + 1, dtype=np.int64) * 150
    want = ix.map(ss, so, o, threads=8)
    return ix, ss, so, o, want, int(flagged[n - 1]), int((noisy[:n] & (st[:n] != 0)).sum())


def _map(monkeypatch, batch=None):
    from proovread_amd import _abi
    ix, ss, so, o, want, n_flag, n_noisy_flag = _case()
    ix.to_gpu(_abi.default_context())
    monkeypatch.setenv("PRGPU_SEED_BUDGET", str(BUDGET))
    if batch is not None:
        monkeypatch.setenv("PRGPU_SEED_1B_BATCH", str(batch))
    got, st = ix.map_gpu(ss, so, o, allow_flagged=True)
    reads = ix.phase_ms()["pass_reads"]
    print(f"budget {BUDGET}, batch {batch}: {len(so) - 1} reads, {n_flag} flagged by pass 1 on the host "
          f"({n_noisy_flag} noisy), handed to the passes: {reads}, flagged at the end: {int((st != 0).sum())}")
    return got, st, reads


@pytest.mark.gpu
def test_gpu_budget_hands_the_noisy_reads_to_pass1b(monkeypatch):
    _, _, _, _, want, n_flag, n_noisy_flag = _case()
    got, st, reads = _map(monkeypatch)
    assert n_noisy_flag > 16384
    assert reads["pass1b_lane"] == n_flag and reads["pass1b_wave"] == 0
    assert reads["later"] == 0
    assert not st.any()
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 16, 63])
def test_gpu_pass1b_batch_sizes_give_the_same_seeds(monkeypatch, batch):
    _, _, _, _, want, n_flag, _ = _case()
    assert batch == 1 or n_flag % batch
    got, st, reads = _map(monkeypatch, batch)
    assert reads["pass1b_lane"] == n_flag and reads["later"] == 0
    assert not st.any()
    assert np.array_equal(got, want)

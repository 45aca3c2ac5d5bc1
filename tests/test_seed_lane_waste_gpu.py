"""The device's lane phase after its dropped accesses (seed_kernels.hip seed_batch_kernel: the
lazy kernel's range tables cleared once per launch and reused from read to read; mem_chain_flt
without the kept-list scan at -D 0, the chain weight in one walk, in both kernels) on 50,000
short reads with the edge reads of test_seed_lane_waste.py among them: the seeds of the host path
and the flags of the host run of the device path, for the eager (bwa-sr) and the lazy
(bwa-sr-finish) kernels.

With PRGPU_SEED_WAVES_PER_CU=1 a wave's 64 slices serve several 64-read batches each, so reads
follow reads in one slice; reads that overflow pass 1's 384 chains (a 17-mer planted in 450 long
reads: one chain per long read, all below the chain weight minimum, so nothing else overflows)
sit at fixed lanes of early batches, and the read at that lane of whichever batch the wave takes
next is an ordinary one."""
import numpy as np
import pytest

from proovread_amd import seed

N = 4
WAVES = 256   # pass 1's waves at one wave per CU


def _rc(r):
    r = np.asarray(r, np.uint8)[::-1]
    return np.where(r < 4, 3 - r, 4).astype(np.uint8)


def _build():
    rng = np.random.default_rng(20261021)
    G = rng.integers(0, 4, 250_000).astype(np.uint8)
    k17 = rng.integers(0, 4, 17).astype(np.uint8)
    lrs = []
    for i in range(2000):
        s = int(rng.integers(0, len(G) - 500))
        lr = G[s:s + 500].copy()
        sub = rng.random(500) < 0.03
        lr[sub] = rng.integers(0, 4, int(sub.sum()))
        if i % 4 == 0 and i < 1800:   # 450 long reads hold the 17-mer
            p = int(rng.integers(20, 460))
            lr[p:p + 17] = k17
        lrs.append(lr)
    n = 50_000
    lens = rng.integers(100, 151, n)
    starts = rng.integers(0, len(G) - 150, n)
    reads = []
    for i in range(n):
        r = G[starts[i]:starts[i] + lens[i]].copy()
        if i % 3 == 0:
            r[int(rng.integers(0, len(r)))] = rng.integers(0, 4)
        reads.append(_rc(r) if i % 2 else r)
    base = G[5000:5192].copy()

    def with_n(pos):
        r = base.copy()
        r[list(pos)] = N
        return r
    special = [with_n([0]), with_n([191]), with_n([63]), with_n([64]), with_n([127]), with_n([128]),
               with_n([63, 64, 127, 128, 191]), with_n(range(60, 69)), with_n(range(124, 132)),
               np.full(150, N, np.uint8), G[7000:7011].copy(), G[7000:7012].copy(), G[7000:7192].copy(),
               G[7000:7193].copy()]
    over = np.concatenate([np.full(40, N, np.uint8), k17, np.full(43, N, np.uint8)])
    # the 17-mer between mapped flanks: many chains, but its SMEMs reach into the flanks and have
    # fewer occurrences than pass 1's chains (no overflow)
    over2 = np.concatenate([G[9000:9050], k17, G[9100:9150]])
    over_at = [0, 1, 31, 63, 64 * 5 + 17, 64 * 40 + 63, 64 * 130, 64 * 200 + 5, 64 * 255 + 62, 64 * 300 + 9]
    for k, i in enumerate(over_at):
        reads[i] = over2 if k % 3 == 2 else over
        # the suggested follower one sweep of the waves later, and the batch after the overflow
        reads[i + 64 * WAVES] = special[k % len(special)]
    for k, s in enumerate(special):
        reads[1000 + 37 * k] = s
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    lr_off = np.concatenate([[0], np.cumsum([len(x) for x in lrs])]).astype(np.int64)
    ix = seed.SeedIndex(np.concatenate(lrs), lr_off)
    n_over = sum(1 for k in range(len(over_at)) if k % 3 != 2)
    return {"ix": ix, "seq": np.concatenate(reads), "off": off, "n_over": n_over, "G": G, "ref": {}}


@pytest.fixture(scope="module")
def data():
    from proovread_amd import _abi
    d = _build()
    d["ix"].to_gpu(_abi.default_context())
    yield d
    d["ix"].close()


def _reference(data, finish):
    """The host path's seeds and the device path's flags on the host, once per option set."""
    if finish not in data["ref"]:
        o = seed.default_opts(finish)
        host = data["ix"].map(data["seq"], data["off"], o, threads=16)
        dev, wst = data["ix"].map_device_caps(data["seq"], data["off"], o, threads=16)
        data["ref"][finish] = (host, dev, wst)
    return data["ref"][finish]


def _check(data, finish):
    host, dev, wst = _reference(data, finish)
    got, st = data["ix"].map_gpu(data["seq"], data["off"], seed.default_opts(finish), allow_flagged=True)
    assert np.array_equal(st, wst)
    assert np.array_equal(got, dev)
    ok = wst == 0
    assert ok.mean() > 0.999
    assert np.array_equal(got, host[ok[host["sr"]]])
    assert len(got) > 2 * (len(data["off"]) - 1)
    return data["ix"].phase_ms()["pass_reads"]


@pytest.mark.gpu
@pytest.mark.parametrize("finish", [False, True])
def test_slices_reused_over_batches(data, finish, monkeypatch):
    monkeypatch.setenv("PRGPU_SEED_WAVES_PER_CU", "1")
    reads = _check(data, finish)
    # the overflowing reads went on to pass 2: the 17-mer is a seed under either option set (-k 12 /
    # -k 17), and its 450 chains outgrow pass 1's 384 in the eager and in the lazy kernel, whose
    # slices are the reused ones
    assert reads["pass2"] + reads["pass1b_wave"] + reads["pass1b_lane"] >= data["n_over"]


@pytest.mark.gpu
@pytest.mark.parametrize("finish", [False, True])
def test_default_waves(data, finish):
    _check(data, finish)


@pytest.mark.gpu
def test_long_read_among_short_reads(data):
    """One 600-base read with N bases (the slices grow with the longest read: range tables of
    2,048 entries) among 4,000 of the short reads."""
    n = 4000
    long_read = data["G"][20_000:20_600].copy()
    long_read[[70, 200, 599]] = N
    seq = np.concatenate([data["seq"][:data["off"][n]], long_read])
    off = np.concatenate([data["off"][:n + 1], [data["off"][n] + 600]]).astype(np.int64)
    for finish in (False, True):
        o = seed.default_opts(finish)
        want, wst = data["ix"].map_device_caps(seq, off, o, threads=16)
        host = data["ix"].map(seq, off, o, threads=16)
        got, st = data["ix"].map_gpu(seq, off, o, allow_flagged=True)
        assert np.array_equal(st, wst) and np.array_equal(got, want)
        assert np.array_equal(got, host[(wst == 0)[host["sr"]]])
        assert (got["sr"] == n).any()

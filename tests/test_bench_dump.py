"""bench.py --dump-outputs: the files dump_outputs writes for a small long-read set (host only:
the set is a stand-in with the download() of iteration.LongReadSet)."""
import numpy as np

import bench


class _Set:
    def __init__(self, off, sq, ql):
        self.pools = (off, sq, ql, None)

    def download(self, seq=True, qual=True):
        return self.pools


def _set(seed=7, n=2500):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 60, n)
    lens[[0, 5, 1023, 1024, n - 1]] = 0   # empty reads: first, last, either side of a block boundary
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return _Set(off, rng.integers(33, 127, off[-1]).astype(np.uint8), rng.integers(33, 127, off[-1]).astype(np.uint8))


def test_dump_outputs_files_and_checksums(tmp_path):
    s = _set()
    off, sq, ql, _ = s.pools
    chim = ["lr1\t10\t20\t0.5", "lr7\t1\t2\t0.25"]
    bench.dump_outputs(tmp_path / "d", s, chim)
    got = {p.stem: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert sorted(got) == ["chimera_lines", "read_checksums", "read_offsets", "sample_bases", "sample_quals",
                           "sample_reads"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert np.array_equal(got["read_offsets"], off)
    n = len(off) - 1
    want = np.zeros((n, 4))
    for i in range(n):
        w = np.arange(off[i + 1] - off[i]) % 251 + 1
        for c, pool in ((0, sq), (2, ql)):
            v = pool[off[i]:off[i + 1]].astype(np.int64)
            want[i, c], want[i, c + 1] = v.sum(), (v * w).sum()
    assert np.array_equal(got["read_checksums"], want)
    pick = got["sample_reads"].astype(np.int64)
    assert len(pick) == bench.DUMP_SAMPLE_READS and np.all(np.diff(pick) > 0) and pick[-1] < n
    assert np.array_equal(got["sample_bases"], np.concatenate([sq[off[i]:off[i + 1]] for i in pick]))
    assert np.array_equal(got["sample_quals"], np.concatenate([ql[off[i]:off[i + 1]] for i in pick]))
    assert bytes(got["chimera_lines"].astype(np.uint8)).decode() == "\n".join(chim)


def test_dump_outputs_same_sample_every_time(tmp_path):
    s = _set()
    bench.dump_outputs(tmp_path / "a", s, [])
    bench.dump_outputs(tmp_path / "b", s, [])
    for p in (tmp_path / "a").iterdir():
        assert np.array_equal(np.load(p), np.load(tmp_path / "b" / p.name)), p.name
    assert np.load(tmp_path / "a" / "chimera_lines.npy").shape == (0,)

"""The resident consensus batch's buffer sizes and a pipeline batch's output capacities
(proovread_amd/csrc/cns_plan.h), compiled for the host (tests/native/cns_plan_host.cpp).  The byte
counts below are literals worked out by hand from the ensure chains the table replaced: (count + 1)
elements of the array's type, (n_lr + 16) ints of retry list, 64 bytes of work counters, 24 phase
clocks of 8 bytes."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

# every buffer the table sizes, by group
GROUPS = {
    "aln_off": ["CB_ALN_OFF"],
    "aln_in": ["CB_POS", "CB_SCORE", "CB_AFLAGS", "CB_SEQ_OFF", "CB_LSEQ", "CB_CIG_OFF", "CB_NCIG"],
    "aln_scratch": ["CB_A_ST", "CB_A_LEN", "CB_A_NC", "CB_A_BIN", "CB_A_CB", "CB_A_CE", "CB_A_SB", "CB_A_RPOS", "CB_A_END",
                    "CB_SORTED", "CB_LST_SCORE", "CB_LST_ALN", "CB_KEPT"],
    "read_out": ["CB_STATUS", "CB_SEQ_LEN", "CB_TRACE_LEN", "CB_NCIGAR", "CB_NCHIM", "CB_O_SEQ", "CB_O_QUAL", "CB_O_TRACE",
                 "CB_O_CIG", "CB_O_CHIM", "CB_WORK", "CB_PROF", "CB_RETRY"],
}

# (read lengths, alignments) -> out_off, chim_off, and the bytes asked for each buffer
CASES = {
    "empty": dict(
        lens=[], n_aln=0, out_off=[0], chim_off=[0],
        bytes=dict(CB_ALN_OFF=8,
                   CB_POS=4, CB_SCORE=8, CB_AFLAGS=1, CB_SEQ_OFF=8, CB_LSEQ=4, CB_CIG_OFF=8, CB_NCIG=4,
                   CB_A_ST=4, CB_A_LEN=4, CB_A_NC=8, CB_A_BIN=4, CB_A_CB=4, CB_A_CE=4, CB_A_SB=4, CB_A_RPOS=4, CB_A_END=4,
                   CB_SORTED=4, CB_LST_SCORE=8, CB_LST_ALN=4, CB_KEPT=1,
                   CB_STATUS=4, CB_SEQ_LEN=4, CB_TRACE_LEN=4, CB_NCIGAR=4, CB_NCHIM=4,
                   CB_O_SEQ=1, CB_O_QUAL=1, CB_O_TRACE=1, CB_O_CIG=4, CB_O_CHIM=16,
                   CB_WORK=64, CB_PROF=192, CB_RETRY=64)),
    "one-base": dict(
        # 2 * 1 + 1024 output bytes; int(1 / 20) + 1 = 1 bin -> 1 // 2 + 2 = 2 chimera records
        lens=[1], n_aln=1, out_off=[0, 1026], chim_off=[0, 2],
        bytes=dict(CB_ALN_OFF=16,
                   CB_POS=8, CB_SCORE=16, CB_AFLAGS=2, CB_SEQ_OFF=16, CB_LSEQ=8, CB_CIG_OFF=16, CB_NCIG=8,
                   CB_A_ST=8, CB_A_LEN=8, CB_A_NC=16, CB_A_BIN=8, CB_A_CB=8, CB_A_CE=8, CB_A_SB=8, CB_A_RPOS=8, CB_A_END=8,
                   CB_SORTED=8, CB_LST_SCORE=16, CB_LST_ALN=8, CB_KEPT=2,
                   CB_STATUS=8, CB_SEQ_LEN=8, CB_TRACE_LEN=8, CB_NCIGAR=8, CB_NCHIM=8,
                   CB_O_SEQ=1027, CB_O_QUAL=1027, CB_O_TRACE=1027, CB_O_CIG=4108, CB_O_CHIM=48,
                   CB_WORK=64, CB_PROF=192, CB_RETRY=68)),
    "three-reads": dict(
        # 19 -> 1062 bytes, 1 bin, 2 records; 20 -> 1064 bytes, 2 bins, 3 records;
        # 4097 -> 9218 bytes, 205 bins, 104 records
        lens=[19, 20, 4097], n_aln=5, out_off=[0, 1062, 2126, 11344], chim_off=[0, 2, 5, 109],
        bytes=dict(CB_ALN_OFF=32,
                   CB_POS=24, CB_SCORE=48, CB_AFLAGS=6, CB_SEQ_OFF=48, CB_LSEQ=24, CB_CIG_OFF=48, CB_NCIG=24,
                   CB_A_ST=24, CB_A_LEN=24, CB_A_NC=48, CB_A_BIN=24, CB_A_CB=24, CB_A_CE=24, CB_A_SB=24, CB_A_RPOS=24,
                   CB_A_END=24, CB_SORTED=24, CB_LST_SCORE=48, CB_LST_ALN=24, CB_KEPT=6,
                   CB_STATUS=16, CB_SEQ_LEN=16, CB_TRACE_LEN=16, CB_NCIGAR=16, CB_NCHIM=16,
                   CB_O_SEQ=11345, CB_O_QUAL=11345, CB_O_TRACE=11345, CB_O_CIG=45380, CB_O_CHIM=1760,
                   CB_WORK=64, CB_PROF=192, CB_RETRY=76)),
}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("cns_plan") / "libcns_plan_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", str(out),
                    str(ROOT / "tests" / "native" / "cns_plan_host.cpp")], check=True)
    L = C.CDLL(str(out))
    L.cns_plan_id.argtypes = [C.c_char_p]
    L.cns_plan_group.argtypes = [C.c_char_p]
    L.cns_plan_group.restype = C.c_uint
    L.cns_plan_all.restype = C.c_uint
    L.cns_plan_sizes.argtypes = [C.c_uint, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    L.cns_plan_pipe_caps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.cns_plan_pipe_caps.restype = None
    return L


def buf_id(lib, name):
    i = lib.cns_plan_id(name.encode())
    assert i >= 0, name
    return i


def sizes(lib, mask, n_lr, n_aln, seq_cap, chim_cap):
    """[(id, bytes)] of the groups in `mask`, in table order."""
    ids, by = np.full(128, -1, np.int32), np.full(128, -1, np.int64)
    n = lib.cns_plan_sizes(mask, n_lr, n_aln, seq_cap, chim_cap, ids.ctypes.data, by.ctypes.data, 128)
    assert 0 <= n <= 128
    return [(int(ids[k]), int(by[k])) for k in range(n)]


def pipe_caps(lib, lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    oo, co = np.full(len(lens) + 1, -1, np.int64), np.full(len(lens) + 1, -1, np.int64)
    lib.cns_plan_pipe_caps(off.ctypes.data, len(lens), oo.ctypes.data, co.ctypes.data)
    return [int(v) for v in oo], [int(v) for v in co]


@pytest.mark.parametrize("case", list(CASES))
def test_output_capacities(lib, case):
    c = CASES[case]
    assert pipe_caps(lib, c["lens"]) == (c["out_off"], c["chim_off"])


@pytest.mark.parametrize("case", list(CASES))
def test_bytes_per_buffer(lib, case):
    c = CASES[case]
    got = dict(sizes(lib, lib.cns_plan_all(), len(c["lens"]), c["n_aln"], c["out_off"][-1], c["chim_off"][-1]))
    want = {buf_id(lib, name): b for name, b in c["bytes"].items()}
    assert got == want, {k: (want.get(k), got.get(k)) for k in set(want) | set(got) if want.get(k) != got.get(k)}


def test_groups(lib):
    """Each group lists each buffer at most once, holds exactly its buffers, and the groups together
    are exactly the buffers the upload paths size from the batch's counts."""
    union = []
    for g, names in GROUPS.items():
        mask = lib.cns_plan_group(g.encode())
        assert mask and mask & (mask - 1) == 0, g
        ids = [i for i, _ in sizes(lib, mask, 3, 5, 100, 10)]
        assert len(ids) == len(set(ids)), g
        assert sorted(ids) == sorted(buf_id(lib, n) for n in names), g
        union += ids
    assert len(union) == len(set(union)) == 34
    every = [i for i, _ in sizes(lib, lib.cns_plan_all(), 3, 5, 100, 10)]
    assert sorted(every) == sorted(union)
    assert {n for c in CASES.values() for n in c["bytes"]} == {n for names in GROUPS.values() for n in names}

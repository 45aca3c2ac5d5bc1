"""The occurrence pool's sizing (seed_plan.h occ_pool_words) and the counts the lane phase reserves
from it (seed_chain.h occ_words, occ_taken), compiled for the host
(tests/native/seed_chain_plan_host.cpp)."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
GB = 1 << 30


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("seed_chain_plan") / "libchainplan.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", str(out),
                    str(ROOT / "tests" / "native" / "seed_chain_plan_host.cpp")], check=True)
    L = C.CDLL(str(out))
    L.occ_pool_words_case.restype = C.c_int64
    L.occ_pool_words_case.argtypes = [C.c_int64, C.c_int, C.c_int64, C.c_int64]
    L.occ_one_list_words.restype = C.c_int64
    L.occ_words_case.restype = C.c_int64
    L.occ_taken_case.argtypes = [C.c_int, C.c_int64]
    return L


def test_pool_follows_the_reads_within_its_limits(lib):
    one = lib.occ_one_list_words()
    # an empty card: the reads' share, one pool for the task
    assert lib.occ_pool_words_case(200_000, 0, 280 * GB, 0) == 200_000 * 3072 + one
    assert lib.occ_pool_words_case(460_000, 0, 280 * GB, 0) == 8 * GB // 8   # (configs[1]: the 8 GB ceiling)
    assert lib.occ_pool_words_case(914_000, 1, 280 * GB, 0) == 914_000 * 384 + one
    # never beyond 8 GB, however many reads and however much memory
    assert lib.occ_pool_words_case(3_000_000, 0, 280 * GB, 0) == 8 * GB // 8
    # a crowded device: a sixteenth of what is free (the pool's own bytes count as free)
    assert lib.occ_pool_words_case(460_000, 0, 32 * GB, 0) == 2 * GB // 8
    assert lib.occ_pool_words_case(460_000, 0, 16 * GB, 16 * GB) == 2 * GB // 8
    # and always one read's largest list
    assert lib.occ_pool_words_case(0, 0, 0, 0) == one
    assert lib.occ_pool_words_case(460_000, 0, 1 << 20, 0) == one


def test_a_list_of_n_occurrences_takes_n_and_a_half_words(lib):
    assert [lib.occ_words_case(n) for n in (0, 1, 2, 3, 16384)] == [0, 2, 3, 5, 24576]


@pytest.mark.parametrize("max_occ", [1, 20, 500])
def test_reserved_count_equals_the_selection_loop(lib, max_occ):
    """chain_seq's selection: of np qualifying hits every step-th, at most max_occ"""
    for np_ in list(range(0, 3 * max_occ + 3)) + [10 * max_occ - 1, 10 * max_occ, 10 * max_occ + 1, 7919]:
        step = np_ // max_occ if np_ > max_occ else 1
        count, take = 0, 0
        for f in range(np_):
            if count >= max_occ:
                break
            if f == take:
                take += step
                count += 1
        assert lib.occ_taken_case(max_occ, np_) == count, (max_occ, np_)

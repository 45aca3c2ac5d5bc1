"""csrc/ccs_core.h compiled alone for the host (tests/native/ccs_core_host.cpp), under
AddressSanitizer and UBSan: the header is HIP-free, and a stand-alone program over it writes the
alignments and the consensus the library's host path writes."""
import random
import subprocess
from pathlib import Path

import pytest

import ccs_ref
from proovread_amd import ccseq

SRC = Path(__file__).resolve().parent / "native" / "ccs_core_host.cpp"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("ccs_core") / "ccs_core_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(out), str(SRC)], check=True)
    return out


@pytest.mark.parametrize("w,seed", [(8, 1), (300, 2), (8, 3)])
def test_program_under_sanitizers_equals_the_library(exe, tmp_path, w, seed):
    rng = random.Random(seed)
    _, recs = ccs_ref.sim_zmw(rng, "m1", 1, rng.randrange(150, 320), rng.randrange(2, 7))
    ids = [r[0] for r in recs]
    role, _, _ = ccseq.group(ids, [len(r[1]) for r in recs])
    ref = list(role).index(ccseq.PRIMARY)
    f = tmp_path / "group.txt"
    f.write_text(f"9 {w} {ref}\n" + "".join(f"{r[1]} {r[2]}\n" for r in recs))
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    grp = ([x[1].encode() for x in recs], [x[2].encode() for x in recs], ref)
    (res,), (ga,), _ = ccseq.run_groups([grp], ccseq.default_params(w=w), device=False)
    want = [f"aln 1 {a[0]} {a[1]} {a[2]} {a[3]}" if a else "aln 0 0 0 0 " for t, a in enumerate(ga) if t != ref]
    want += [f"seq {res[1].decode()}", f"qual {res[2].decode()}", f"trace {res[3].decode()}", "groups 1 roles 0 1 0"]
    assert r.stdout.split("\n")[:-1] == want

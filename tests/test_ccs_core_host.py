"""csrc/ccs_core.h compiled alone for the host (tests/native/ccs_core_host.cpp), under
AddressSanitizer and UBSan: the header is HIP-free, and a stand-alone program over it writes the
alignments and the consensus the library's host path writes.  The program also holds the slab
of per-column states against the same states found by bisection over the ops, entry by entry
and vote by vote, and exits non-zero at the first difference."""
import random
import subprocess
from pathlib import Path

import pytest

import ccs_cases
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


def _hand_groups():
    """name -> (trim, reference, [(aligned SEQ, QUAL, pos0, CIGAR, strand)]): 70-base references
    with alignments of about 60 bases that hold the corners of Seq.pm:396-459."""
    rng = random.Random(31)
    ref = ccs_cases.rand_seq(rng, 70)

    def aln(pos, cigar, ins=None, strand=0, low=False):   # phred 25-40 (weights >= 5.21), low: 5-12 (<= 1.2)
        s = ccs_cases.query_of(ref, pos, cigar, rng, ins)
        return s, "".join(chr(33 + (rng.randint(5, 12) if low else rng.randint(25, 40))) for _ in s), pos, cigar, strand

    return {
        # D+I is one replaced state; the second alignment carries the same bytes from the other strand
        "del_ins_pair": (1, ref, [aln(2, "30M2D3I33M", ["TGA"]), aln(4, "28M2D3I31M", ["TGA"], strand=1), aln(0, "66M", low=True)]),
        # a leading insertion is a column of its own (Trim 0 keeps it), and so is a trailing one's state
        "leading_ins": (0, ref, [aln(4, "3I20M2D40M", ["GGG"]), aln(2, "2M1D58M4I", ["ACAC"], low=True)]),
        # insertions behind the last column of an M op: two states in one column, and one carried twice
        "ins_behind_m": (1, ref, [aln(3, "40M2I22M", ["CA"]), aln(1, "42M2I24M", ["TG"], strand=1), aln(0, "43M2I25M", ["TG"])]),
        # a deletion at window position 1 takes the quality at position 1 on both sides ($qpos > 1)
        "del_at_1": (1, ref, [aln(3, "1M2D62M"), aln(5, "1M1D30M1D31M", strand=1)]),
    }


@pytest.mark.parametrize("name", ["del_ins_pair", "leading_ins", "ins_behind_m", "del_at_1"])
def test_slab_and_bisection_agree_on_hand_groups(exe, tmp_path, name):
    """The program exits non-zero where an entry of the slab or a vote over it differs from the
    same state found by bisection; its consensus is the library's from the same alignments."""
    trim, ref, alns = _hand_groups()[name]
    assert all(55 <= len(a[0]) <= 70 for a in alns)
    stored = [(ccs_ref.revcomp(s), ql[::-1]) if strand else (s, ql) for s, ql, _, _, strand in alns]
    f = tmp_path / "group.txt"
    f.write_text(f"9 8 0 {trim}\n{ref} {'#' * len(ref)}\n" +
                 "".join(f"{s} {ql} {a[4]} {a[2]} {a[3]}\n" for (s, ql), a in zip(stored, alns)))
    r = subprocess.run([str(exe), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    grp = ([ref.encode()] + [s.encode() for s, _ in stored], [b"#" * len(ref)] + [ql.encode() for _, ql in stored], 0)
    ga = [None] + [(a[4], a[2], 0, a[3]) for a in alns]
    (res,) = ccseq.consensus_groups([grp], [ga], ccseq.default_params(trim=trim), device=False)
    assert res[0] == 0
    want = [f"aln 1 {a[4]} {a[2]} 0 {a[3]}" for a in alns]
    want += [f"seq {res[1].decode()}", f"qual {res[2].decode()}", f"trace {res[3].decode()}", "groups 1 roles 0 1 0"]
    assert r.stdout.split("\n")[:-1] == want
    # the corner is in the consensus: the two strong alignments outweigh the weak one and the
    # reference ('#': 0.03), so their states of several bases (D) and their gaps (I) are written
    assert ("D" in res[3].decode()) == (name != "del_at_1") and ("I" in res[3].decode()) == (name != "ins_behind_m")

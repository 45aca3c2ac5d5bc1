"""Deterministic generator of the ccs-1 consensus cases: about ten small groups (a reference
subread and the alignments of the other subreads of its ZMW, SAM lines in arrival order) --
the hand-made corner cases of tests/ccs_cases.py and simulated ZMWs mapped by the host path.

    python make_ccs_cases.py out_cases.txt
"""
import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE.parent), str(HERE.parent.parent)]
import casefmt  # noqa: E402
import ccs_cases  # noqa: E402
import ccs_ref  # noqa: E402
from proovread_amd import ccseq  # noqa: E402


def main(out):
    # rev_ins_wins came after the Perl records were written; the C oracle holds it
    cases = [ccs_cases.to_case(name, *c) for name, c in ccs_cases.hand_cases().items() if name != "rev_ins_wins"]
    rng = random.Random(31)
    for z, w in enumerate((8, 300, 8, 300)):
        _, recs = ccs_ref.sim_zmw(rng, "m150101_1_s1_p0", 100 + z, rng.randrange(150, 260), rng.randrange(3, 7))
        ids = [r[0] for r in recs]
        role, _, _ = ccseq.group(ids, [len(r[1]) for r in recs])
        grp = ([r[1].encode() for r in recs], [r[2].encode() for r in recs], list(role).index(ccseq.PRIMARY))
        (ga,) = ccseq.map_groups([grp], ccseq.default_params(w=w), device=False)
        cases.append(casefmt.Case(f"sim{z}_w{w}", {"qual_weighted": "1", "use_ref_qual": "1"},
                                  ["@" + ids[grp[2]], recs[grp[2]][1], "+", recs[grp[2]][2]], ccseq.sam_lines(ids, grp, ga)))
    casefmt.write_cases(out, cases)


if __name__ == "__main__":
    main(sys.argv[1])

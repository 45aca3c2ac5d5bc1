"""One timing of the ccs-1 stage: pr_ccs_run on the device (wall and kernel time, after a
warm-up call) against the host path at 16 threads, on one synthetic set of ZMWs under the CLR
error model.  Prints and writes one JSON record.

    python tools/time_ccs.py [--zmws 400] [--out profiles/ccs_timing.json]
"""
import argparse
import json
import random
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import ccs_ref  # noqa: E402
from proovread_amd import _abi, ccseq  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--zmws", type=int, default=400)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ccs_timing.json"))
    a = ap.parse_args()
    rng = random.Random(1)
    groups = []
    for z in range(a.zmws):
        _, recs = ccs_ref.sim_zmw(rng, "m1", z, rng.randrange(800, 2500), rng.randrange(3, 9))
        groups.append(([r[1].encode() for r in recs], [r[2].encode() for r in recs], 1))
    n_sub = sum(len(g[0]) for g in groups)
    bases = sum(len(s) for g in groups for s in g[0])
    ctx = _abi.default_context()
    ccseq.run_groups(groups[:8], ctx=ctx)   # warm-up
    t = time.perf_counter()
    dev = ccseq.run_groups(groups, ctx=ctx)
    dev_s = time.perf_counter() - t
    t = time.perf_counter()
    host = ccseq.run_groups(groups, device=False, threads=16)
    host_s = time.perf_counter() - t
    rec = {"zmws": a.zmws, "subreads": n_sub, "bases": bases, "w": 300, "device_wall_s": round(dev_s, 3),
           "device_kernel_ms": round(dev[2], 1), "host_16_threads_s": round(host_s, 3),
           "equal": dev[0] == host[0] and dev[1] == host[1]}
    print(json.dumps(rec))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")
    return 0 if rec["equal"] and dev_s < host_s else 1


if __name__ == "__main__":
    sys.exit(main())

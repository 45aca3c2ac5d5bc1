#!/usr/bin/env python3
"""One timing of the unitig consensus (pr_utg_run): device against the host path at 16 threads
on the same machine, on synthetic data shaped like a blasr-utg task -- long reads of 5-30 kb at
CLR error rates, unitig hits of 1-20 kb at about 3x, repeat stacks of 10-30 short hits, and
proovread's flags (--qual-weighted --fallback-phred 30 --rep-coverage 7 --min-ncscore 3.3
--invert-scores).  One run after a warm-up call; the results must be identical.

    python tools/time_utg.py [--reads 2000] [--threads 16] [--out profiles/utg_timing.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from proovread_amd import _abi, cns, utgcns  # noqa: E402

BASES = np.frombuffer(b"ACGT", np.uint8)


def hit(rng, name, rid, ref, start, span, score, noisy=True):
    """A unitig hit over ref[start, start + span): the read's errors show as mismatches,
    deletions and single-base insertions; QUAL '*' as blasr writes it for FASTA unitigs."""
    cols = ref[start:start + span]
    u = rng.random(span)
    dele = (u < 0.04) & noisy
    mism = (u > 0.98) & noisy
    ins = (rng.random(span) < 0.08) & noisy
    dele[0] = dele[-1] = ins[-1] = False
    base = np.where(mism, BASES[(np.searchsorted(BASES, cols) + 1 + rng.integers(0, 3, span)) % 4], cols)
    ops = np.empty(2 * span, np.uint8)
    ops[0::2] = np.where(dele, 2, 0)
    ops[1::2] = np.where(ins, 1, 255)
    seq = np.empty(2 * span, np.uint8)
    seq[0::2] = base
    seq[1::2] = BASES[rng.integers(0, 4, span)]
    take = np.empty(2 * span, bool)
    take[0::2] = ~dele
    take[1::2] = ins
    ops = ops[ops != 255]
    edge = np.flatnonzero(np.diff(ops)) + 1
    starts = np.concatenate(([0], edge))
    lens = np.diff(np.concatenate((starts, [len(ops)])))
    cigar = [int(n) << 4 | int(ops[s]) for s, n in zip(starts, lens)]
    return cns.SamRecord(rid, start + 1, cigar, seq[take].tobytes().decode(), "*", float(score))


def make(n_reads, seed):
    rng = np.random.default_rng(seed)
    reads, alns = [], []
    for r in range(n_reads):
        L = int(rng.integers(5000, 30001))
        ref = BASES[rng.integers(0, 4, L)]
        rid = f"lr{r}"
        reads.append(cns.LongRead(rid, ref.tobytes().decode(), (rng.integers(2, 20, L) + 33).astype(np.uint8).tobytes().decode(), ""))
        a = []
        covered = 0
        while covered < 3 * L:
            span = int(min(L, rng.integers(1000, 20001)))
            start = int(rng.integers(0, L - span + 1))
            a.append(hit(rng, f"u{len(a)}", rid, ref, start, span, -4.5 * span))
            covered += span
        at = int(rng.integers(0, L - 400))
        for _ in range(int(rng.integers(10, 31))):
            span = int(rng.integers(60, 300))
            a.append(hit(rng, f"s{len(a)}", rid, ref, at + int(rng.integers(0, 80)), span, -4.0 * span))
        order = rng.permutation(len(a))
        alns.append([a[i] for i in order])
    return reads, alns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    p = utgcns.UtgParams(qual_weighted=True, fallback_phred=30, rep_coverage=7, min_ncscore=3.3, invert_scores=True)
    reads, alns = make(a.reads, a.seed)
    ctx = _abi.default_context()
    utgcns.run(reads[:8], alns[:8], p, device=True, ctx=ctx)           # warm-up
    utgcns.run(reads[:8], alns[:8], p, device=False, threads=a.threads)
    A = utgcns.Packed(reads, alns)
    timing = {}
    t0 = time.perf_counter()
    dev = utgcns.run_packed(reads, A, p, device=True, ctx=ctx, timing=timing)
    t_dev = time.perf_counter() - t0
    B = utgcns.Packed(reads, alns)
    t0 = time.perf_counter()
    host = utgcns.run_packed(reads, B, p, device=False, threads=a.threads)
    t_host = time.perf_counter() - t0
    same = all((d.status, d.seq, d.qual, d.trace, d.windows) == (h.status, h.seq, h.qual, h.trace, h.windows) and (d.kept == h.kept).all()
               for d, h in zip(dev, host))
    res = {"reads": len(reads), "read_bases": int(sum(len(r.seq) for r in reads)), "alignments": int(A.n_alns),
           "aligned_bases": int(A.seq_off[-1]), "cigar_ops": int(A.cig_off[-1]), "kept": int(sum(int(h.kept.sum()) for h in host)),
           "windows": int(sum(len(h.windows) for h in host)), "status_nonzero": int(sum(h.status != 0 for h in host)),
           "device_wall_s": round(t_dev, 4), "device_kernel_ms": round(timing["kernel_ms"], 3),
           "device_kernel_split_ms": {k: round(v, 3) for k, v in timing["split_ms"].items()},
           "host_threads": a.threads, "host_wall_s": round(t_host, 4), "identical": bool(same),
           "device_faster": bool(t_dev < t_host)}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

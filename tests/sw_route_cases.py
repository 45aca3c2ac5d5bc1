"""Directed inputs for the SW stage's launcher routes, the routing rule restated for tests,
and a per-side trace of the oracle's extension -- TEST INFRASTRUCTURE, CPU only.

`synth.simulate` plants single-base errors only, so at the preset bands almost no task asks
for the second band and none ends its CIGAR pass above band 40.  The builders here make
small batches by hand: long reads are random sequences, short reads are cut from them around
one exact seed of 19 to 30 bases, and each side of the seed carries one planted feature
(block indel sized from the band, N, a tail that ties the clip decision, a z-drop run, a
read edge).  `route()` is the one place where the `if` ladder of sw_launch_extend /
sw_launch_global / pk_ext_key (csrc/sw_kernels.hip, sw_api.cpp) is written down for tests.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

import oracle_bind as ob

PK_QMAX, PK_TMAX = 255, 320          # csrc/sw_pk.h
LDS_BYTES = 160 * 1024


# ---------------------------------------------------------------------------
# options
def make_opts(a=5, b=11, o_del=2, o_ins=1, e_del=4, e_ins=3, w=40, clip=30, zdrop=100, per_base=2.5):
    o = ob.OswOpts()
    o.a, o.b, o.o_del, o.o_ins, o.e_del, o.e_ins, o.w = a, b, o_del, o_ins, e_del, e_ins, w
    o.pen_clip5 = o.pen_clip3 = clip
    o.zdrop = zdrop
    o.min_score_per_base = per_base
    return o


SCORING = {   # name -> make_opts keywords (without w)
    "sr": dict(a=5, b=11, o_del=2, o_ins=1, e_del=4, e_ins=3, per_base=2.5),          # proovread.cfg bwa-sr
    "finish": dict(a=5, b=13, o_del=15, o_ins=19, e_del=3, e_ins=3, per_base=4.0),    # bwa-sr-finish
    "bwa": dict(a=1, b=4, o_del=6, o_ins=6, e_del=1, e_ins=1, clip=5, per_base=0.9),  # bwa mem's defaults
    "a15": dict(a=15, b=16, o_del=6, o_ins=6, e_del=2, e_ins=2, per_base=9.0),
    "pen32": dict(a=5, b=11, o_del=32, o_ins=6, e_del=2, e_ins=2),
    "pen33": dict(a=5, b=11, o_del=33, o_ins=6, e_del=2, e_ins=2),
    "clip0": dict(a=5, b=11, o_del=2, o_ins=1, e_del=4, e_ins=3, clip=0),
    "clip200": dict(a=5, b=11, o_del=2, o_ins=1, e_del=4, e_ins=3, clip=200),
    "zdrop0": dict(a=5, b=11, o_del=2, o_ins=1, e_del=4, e_ins=3, zdrop=0),
    "zdrop10": dict(a=5, b=11, o_del=2, o_ins=1, e_del=4, e_ins=3, zdrop=10),
}


def scoring(name, w):
    return make_opts(w=w, **SCORING[name])


def gpu_opts(o):
    """The same options as the library's pr_sw_opts."""
    from proovread_amd import sw
    g = sw.default_opts(finish=False)
    g.a, g.b, g.o_del, g.e_del, g.o_ins, g.e_ins, g.w = o.a, o.b, o.o_del, o.e_del, o.o_ins, o.e_ins, o.w
    g.pen_clip5, g.pen_clip3, g.zdrop, g.min_score_per_base = o.pen_clip5, o.pen_clip3, o.zdrop, o.min_score_per_base
    return g


# ---------------------------------------------------------------------------
# batches
def strand_seq(lr, strand):
    if not strand:
        return lr
    r = lr[::-1].copy()
    r[r < 4] = 3 - r[r < 4]
    return r


def dataset(lrs, srs, tasks):
    from proovread_amd import synth
    z = np.zeros(0, np.int64)
    t = np.asarray(tasks, np.int64).reshape(-1, 6)
    lr_off = np.zeros(len(lrs) + 1, np.int64)
    np.cumsum([len(x) for x in lrs], out=lr_off[1:])
    sr_off = np.zeros(len(srs) + 1, np.int64)
    np.cumsum([len(x) for x in srs], out=sr_off[1:])
    return synth.Dataset(np.zeros(0, np.uint8), np.concatenate(lrs).astype(np.uint8), lr_off, z,
                         np.concatenate(srs).astype(np.uint8), sr_off, z, np.zeros(0, np.uint8),
                         t[:, 0].astype(np.int32), t[:, 1].astype(np.int32), t[:, 2].astype(np.uint8),
                         t[:, 3].astype(np.int32), t[:, 4].astype(np.int32), t[:, 5].astype(np.int32))


def merge(parts):
    """One batch from several Datasets (long / short read ids shifted)."""
    lrs, srs, tasks = [], [], []
    for p in parts:
        nl, ns = len(lrs), len(srs)
        lrs += [p.lr_seq[p.lr_off[i]:p.lr_off[i + 1]] for i in range(p.n_lr)]
        srs += [p.sr_seq[p.sr_off[i]:p.sr_off[i + 1]] for i in range(p.n_sr)]
        tasks += [(int(p.t_sr[t]) + ns, int(p.t_lr[t]) + nl, int(p.t_strand[t]), int(p.t_qbeg[t]), int(p.t_rbeg[t]),
                   int(p.t_slen[t])) for t in range(len(p.t_sr))]
    return dataset(lrs, srs, tasks)


def reorder_lrs(d, order):
    """The same batch with its long reads in the order given (old indices)."""
    new = np.empty(d.n_lr, np.int64)
    new[np.asarray(order)] = np.arange(d.n_lr)
    lrs = [d.lr_seq[d.lr_off[i]:d.lr_off[i + 1]] for i in order]
    srs = [d.sr_seq[d.sr_off[i]:d.sr_off[i + 1]] for i in range(d.n_sr)]
    tasks = [(int(d.t_sr[t]), int(new[d.t_lr[t]]), int(d.t_strand[t]), int(d.t_qbeg[t]), int(d.t_rbeg[t]), int(d.t_slen[t]))
             for t in range(len(d.t_sr))]
    return dataset(lrs, srs, tasks)


def gap_tail(o, B):
    """Matches after a block indel of B bases that pay for it with 20 to spare."""
    cost = max(o.o_del + o.e_del * B, o.o_ins + o.e_ins * B)
    return cost // o.a + 20


def retry_block(w):
    """Block length that the band w holds and that asks for the band 2w: the stop rule is
    max_off < w/2 + w/4, so 0.85 w (0.78 w .. 0.9 w all do; below 0.75 w none retries)."""
    return max((w >> 1) + (w >> 2), int(round(0.85 * w)))


def zdrop_plan(o, h0_bases, k):
    """(prefix, run, recover) of a z-drop stop: `prefix` matching bases, a run of `run` query As
    against reference Cs (planted: nothing in it can match by chance), `recover` matches that
    win the run back, so that with zdrop 0 the extension goes on to the read end.  The run is
    longer than the band: zdrop forgives a gap its extensions, so the row maximum falls only
    once a plain deletion from the maximum has left the band.  The prefix keeps the score
    above zero through the run (the extension would otherwise end on an all-zero row before
    any z-drop test, with or without zdrop): a * (h0_bases + prefix) > zdrop + the cheapest way
    through the run, on the diagonal or by an insertion and a deletion of it.  k (the draw)
    lengthens the run."""
    zd = o.zdrop if o.zdrop > 0 else 100
    run = o.w + 10 + 6 * k
    gapped = min(o.o_del + o.o_ins + (o.e_del + o.e_ins) * run + o.b, run * o.b)   # the cheapest way through
    prefix = max(25, -(-(gapped + zd + 30) // o.a) - h0_bases)
    return prefix, run, gapped // o.a + 20


class Builder:
    """Long reads of random bases; add() cuts one short read around an exact seed and plants a
    feature list on each side.  A side is a list of ops walked outwards from the seed:
    ("m", n) n reference bases, ("x", n) n mismatches, ("i", n) n inserted bases, ("d", n) n
    reference bases skipped, ("n", 1) an N in the query.  Past the long read's edge the query
    goes on with random bases."""

    def __init__(self, seed, n_lr=6, lr_len=3000, o=None, lens=None):
        self.o = o
        self.rng = np.random.default_rng(seed)
        self.lrs = [self.rng.integers(0, 4, (lens or {}).get(i, lr_len + 13 * i), dtype=np.uint8) for i in range(n_lr)]
        self.srs, self.tasks, self.tags, self.ref_n = [], [], [], []

    def _walk(self, S, pos, step, spec):
        out = []
        for op, n in spec:
            for _ in range(n):
                inside = 0 <= pos < len(S)
                if op == "i" or (not inside and op != "d"):
                    out.append(int(self.rng.integers(0, 4)))
                    if op != "i":
                        pos += step
                    continue
                if op == "m":
                    out.append(int(S[pos]) if S[pos] < 4 else 0)
                elif op == "x":
                    out.append((int(S[pos]) + int(self.rng.integers(1, 4))) % 4)
                elif op == "n":
                    out.append(4)
                pos += step
        return out

    def span(self, spec):
        return sum(n for op, n in spec if op != "i")

    def place(self, lr, strand, left, right, slen, margin=260):
        L = len(self.lrs[lr])
        lo, hi = self.span(left) + margin, L - slen - self.span(right) - margin
        return int(self.rng.integers(lo, hi))

    def add(self, tag, lr, strand, left=(), right=(), slen=None, rbeg=None, ref_n=None, ok=None, tries=60):
        """ok(sides, region): what the oracle's trace of the read must show (trace_task).  The
        read is drawn again, at another place, until it does -- chance matches in random
        sequence let gaps stand in for planted mismatches -- and tagged "<tag>?" if no draw
        does."""
        for k in range(tries if ok else 1):
            sl = slen or int(self.rng.integers(19, 31))
            lspec = left(k) if callable(left) else left
            rspec = right(k) if callable(right) else right
            rb = self.place(lr, strand, lspec, rspec, sl) if rbeg is None else rbeg
            S = strand_seq(self.lrs[lr], strand)
            lq = self._walk(S, rb - 1, -1, lspec)
            rq = self._walk(S, rb + sl, 1, rspec)
            q = np.array(lq[::-1] + [int(x) for x in S[rb:rb + sl]] + rq, np.uint8)
            if ok is None or ok(*trace_task(self.o, q, self.lrs[lr], strand, len(lq), rb, sl)):
                break
        else:
            tag += "?"
        self.add_raw(tag, lr, strand, q, len(lq), rb, sl)
        if ref_n is not None:   # an N in the reference window only, ref_n bases outwards of the seed's end
            x = rb + sl + ref_n if ref_n >= 0 else rb + ref_n
            self.ref_n.append((lr, x if not strand else len(S) - 1 - x))
        return dict(q=q, qbeg=len(lq), rbeg=rb, slen=sl, lspan=self.span(lspec), rspan=self.span(rspec))

    def add_raw(self, tag, lr, strand, q, qbeg, rbeg, slen):
        self.tasks.append((len(self.srs), lr, strand, qbeg, rbeg, slen))
        self.srs.append(np.asarray(q, np.uint8))
        self.tags.append(tag)

    def plant_n(self, lr, strand, xs):
        """Ns at strand positions xs of long read lr, at once (reads cut later see them)."""
        L = len(self.lrs[lr])
        for x in xs:
            self.lrs[lr][x if not strand else L - 1 - x] = 4

    def plant(self, lr, strand, x0, bases):
        """Strand bases `bases` at strand position x0 of long read lr, at once."""
        L = len(self.lrs[lr])
        for i, c in enumerate(bases):
            self.lrs[lr][x0 + i if not strand else L - 1 - x0 - i] = c if not strand or c > 3 else 3 - c

    def dataset(self):
        lrs = [x.copy() for x in self.lrs]
        for lr, x in self.ref_n:
            lrs[lr][x] = 4
        return dataset(lrs, self.srs, self.tasks)


def directed(o, seed=1, reps=12, long_reads=False, n_lr=7):
    """The directed set for options o: (Dataset, tags).  Long read n_lr - 2 takes the reference
    Ns, n_lr - 3 the tie tails, n_lr - 4 the z-drop runs, the first and the last the pool-edge seeds.  long_reads: plain
    sides of up to 310 bases, so reads reach 650 bp (the HBM forms of the wide and the general
    kernel)."""
    zslot = 120 + 31 + 40 + sum(zdrop_plan(o, 19, 15))   # a z-drop task's stretch of its long read
    bd = Builder(seed, n_lr=n_lr, o=o, lens={n_lr - 3: 600 + 600 * reps, n_lr - 4: 200 + zslot * 2 * reps})
    rng = bd.rng
    w = o.w
    B = retry_block(w)
    tail = gap_tail(o, B)
    # 25 to 35 bases from the seed, or as many as keep the score above zero through the gap
    cost = max(o.o_del + o.e_del * B, o.o_ins + o.e_ins * B)
    near = lambda: max(int(rng.integers(25, 36)), (cost - 19 * o.a) // o.a + 10)
    plain = (lambda: int(rng.integers(250, 311))) if long_reads else (lambda: int(rng.integers(20, 90)))
    free = [i for i in range(n_lr) if i not in (n_lr - 2, n_lr - 3, n_lr - 4)]
    pick = lambda: (free[int(rng.integers(0, len(free)))], int(rng.integers(0, 2)))

    def fits(*sides):   # reads stay within proovread's 1000 bp, a * lq below the 13-bit DP words
        lq = 30 + sum(sum(n for op, n in s if op != "d") for s in sides)
        return lq <= 1000 and o.a * lq < 8192

    # block indels, 25 to 35 bases from the seed, on one side or both
    for kind in ("i", "d"):
        blk = lambda: [("m", near()), (kind, B), ("m", tail)]
        for k in range(reps + 3):
            for where in ("L", "R", "LR"):
                left = blk() if "L" in where else [("m", plain() if where == "R" and long_reads else int(rng.integers(0, 40)))]
                right = blk() if "R" in where else [("m", plain() if where == "L" and long_reads else int(rng.integers(0, 40)))]
                if not fits(left, right):
                    continue
                lr, st = pick()
                bd.add(f"indel_{kind}_{where}", lr, st, left, right,
                       ok=lambda sd, reg, where=where: [x["retry"] for x in sd] == ["L" in where, "R" in where])
    # N in the query side / in the reference window only
    for k in range(reps + 2):
        for side in ("L", "R"):
            feat = [("m", int(rng.integers(8, 40))), ("n", 1), ("m", int(rng.integers(10, 60)))]
            other = [("m", plain())]
            lr, st = pick()
            bd.add(f"qn_{side}", lr, st, feat if side == "L" else other, other if side == "L" else feat)
            d = int(rng.integers(5, 40))
            bd.add(f"rn_{side}", n_lr - 2, int(rng.integers(0, 2)), [("m", plain())], [("m", plain())],
                   ref_n=-1 - d if side == "L" else d)
    # seeds flush with the read start / end, reads that are all seed
    for k in range(reps):
        lr, st = pick()
        bd.add("flush_L", lr, st, (), [("m", plain())])
        lr, st = pick()
        bd.add("flush_R", lr, st, [("m", plain())], ())
        lr, st = pick()
        bd.add("all_seed", lr, st, (), ())
    # seeds next to the pool's first and last base, both strands: truncated windows
    for lr in (0, n_lr - 1):
        L = len(bd.lrs[lr])
        for st in (0, 1):
            for k in range(3):
                slen, over = int(rng.integers(19, 31)), int(rng.integers(10, 60))
                bd.add("edge_lo", lr, st, [("m", int(rng.integers(0, 12)) + over)], [("m", plain())], slen=slen,
                       rbeg=int(rng.integers(0, 12)))
                bd.add("edge_hi", lr, st, [("m", plain())], [("m", int(rng.integers(0, 12)) + over)], slen=slen,
                       rbeg=L - slen - int(rng.integers(0, 12)))
    # tails with gscore == score - pen_clip exactly, and one base fewer / more: the read ends in
    # reference Ns (-1 each whatever the scoring set; with a = 5, b = 11 the (mismatch, match)
    # pairs that also sum to -30 lose to gaps of 4 and 6), pen_clip of them tie, one fewer goes
    # to the read end, one more clips.  Each task has its own stretch of the tie long read.
    tie_lr, slot = n_lr - 3, 0
    for k in range(reps):
        for side, clip in (("L", o.pen_clip5), ("R", o.pen_clip3)):
            if clip > 40 or (0 < o.zdrop < clip + o.b):
                continue
            st, sl, d = int(rng.integers(0, 2)), int(rng.integers(19, 31)), int(rng.integers(20, 50))
            rb = 300 + 300 * slot + int(rng.integers(0, 20))
            slot += 1
            xs = range(rb + sl + d, rb + sl + d + clip + 1) if side == "R" else range(rb - d - clip - 1, rb - d)
            bd.plant_n(tie_lr, st, xs)
            for dp in (-1, 0, 1):
                if clip + dp < 0:
                    continue
                feat, other = [("m", d + clip + dp)], [("m", int(rng.integers(5, 40)))]
                bd.add(f"tie_{side}{dp:+d}", tie_lr, st, feat if side == "L" else other, other if side == "L" else feat,
                       slen=sl, rbeg=rb)
    # a z-drop stop before the read end (zdrop_plan), each task on its own stretch of the z-drop
    # long read; drawn again with another run length until the oracle's trace shows the stop
    zd_lr = n_lr - 4
    for slot in range(2 * reps):
        side = "LR"[slot & 1]
        st, sl, other = int(rng.integers(0, 2)), int(rng.integers(19, 31)), int(rng.integers(5, 40))
        x0 = 100 + zslot * slot
        S = strand_seq(bd.lrs[zd_lr], st)
        saved = S[x0:x0 + zslot].copy()
        for k in range(16):
            pre, run, rec = zdrop_plan(o, sl + (other if side == "R" else 0), k)
            if not fits([("m", pre + run + rec)], [("m", other)]):
                break
            bd.plant(zd_lr, st, x0, saved)
            S = strand_seq(bd.lrs[zd_lr], st)
            # strand layout of the stretch: [other | seed | prefix run recover] or mirrored
            rb = x0 + 40 + (other if side == "R" else pre + run + rec)
            far = [int(x) for x in (S[rb + sl:rb + sl + pre + run + rec] if side == "R"
                                    else S[rb - pre - run - rec:rb][::-1])]
            far[pre:pre + run] = [0] * run
            r0 = rb + sl + pre if side == "R" else rb - pre - run
            bd.plant(zd_lr, st, r0, [1] * run)
            S = strand_seq(bd.lrs[zd_lr], st)
            near_ = [int(x) for x in (S[rb - other:rb] if side == "R" else S[rb + sl:rb + sl + other])]
            q = np.array((near_ + [int(x) for x in S[rb:rb + sl]] + far) if side == "R"
                         else (far[::-1] + [int(x) for x in S[rb:rb + sl]] + near_), np.uint8)
            qbeg = other if side == "R" else len(far)
            sd, reg = trace_task(o, q, bd.lrs[zd_lr], st, qbeg, rb, sl)
            if o.zdrop <= 0 or sd[1 if side == "R" else 0]["zstop"]:
                bd.add_raw(f"zdrop_{side}", zd_lr, st, q, qbeg, rb, sl)
                break
    # just enough matches to pay for the next mismatch, over and over: reaches the read end,
    # fails -T's score per base
    for k in range(2 * reps):
        lr, st = pick()
        n = int(rng.integers(12, 18))
        bd.add("lowscore", lr, st, [("m", o.b // o.a + 1), ("x", 1)] * n, [("m", o.b // o.a + 1), ("x", 1)] * n,
               ok=lambda sd, reg: reg[2] < o.min_score_per_base * (reg[1] - reg[0]), tries=20)
    if long_reads:   # one read of exactly 650 bp pins qmax
        lr, st = pick()
        bd.add("len650", lr, st, [("m", 310)], [("m", 310)], slen=30)
    return bd.dataset(), bd.tags


def mixed(o, seed=1, n_synth=200, long_reads=False, reps=12):
    """directed() plus about n_synth synth.simulate tasks (three more long reads), so that the
    length buckets are not uniform: (Dataset, tags); synthetic tasks are tagged "synth"."""
    from proovread_amd import synth
    d, tags = directed(o, seed, reps=reps, long_reads=long_reads)
    if not n_synth:
        return d, tags
    s = synth.simulate(100 + seed, 12000, 3, 3000, 5.0 if not long_reads else 9.0, sr_len=650 if long_reads else 150)
    rng = np.random.default_rng(seed)
    keep = np.sort(rng.choice(len(s.t_sr), size=min(n_synth, len(s.t_sr)), replace=False))
    s = dataclasses.replace(s, **{k: getattr(s, k)[keep] for k in ("t_sr", "t_lr", "t_strand", "t_qbeg", "t_rbeg",
                                                                   "t_slen")})
    used = np.unique(s.t_sr)   # only the short reads that have a task
    remap = np.full(s.n_sr, -1, np.int64)
    remap[used] = np.arange(len(used))
    srs = [s.sr_seq[s.sr_off[i]:s.sr_off[i + 1]] for i in used]
    tasks = [(int(remap[s.t_sr[t]]), int(s.t_lr[t]), int(s.t_strand[t]), int(s.t_qbeg[t]), int(s.t_rbeg[t]),
              int(s.t_slen[t])) for t in range(len(s.t_sr))]
    s2 = dataset([s.lr_seq[s.lr_off[i]:s.lr_off[i + 1]] for i in range(s.n_lr)], srs, tasks)
    # the synthetic long reads go between the directed ones, whose first and last stay the
    # pool's first and last (the pool-edge seeds)
    m = merge([d, s2])
    order = [0] + list(range(d.n_lr, m.n_lr)) + list(range(1, d.n_lr))
    return reorder_lrs(m, order), tags + ["synth"] * len(tasks)


def perfect(seed, specs, n_lr=3, filler=0, filler_max=60):
    """Perfect-match reads, specs = [(lq, qbeg, slen), ...]; qbeg None: a random seed place.
    `filler` more reads of up to filler_max bases with two mismatches each."""
    bd = Builder(seed, n_lr=n_lr)
    rng = bd.rng
    for lq, qbeg, slen in specs:
        slen = slen or int(rng.integers(19, 31))
        qbeg = int(rng.integers(0, lq - slen + 1)) if qbeg is None else qbeg
        bd.add(f"perfect_{lq}", int(rng.integers(0, n_lr)), int(rng.integers(0, 2)), [("m", qbeg)],
               [("m", lq - qbeg - slen)], slen=slen)
    for k in range(filler):
        n = int(rng.integers(10, (filler_max - 30) // 2))
        bd.add("filler", int(rng.integers(0, n_lr)), int(rng.integers(0, 2)), [("m", n - 5), ("x", 1), ("m", 4)],
               [("m", 4), ("x", 1), ("m", n - 5)])
    return bd.dataset(), bd.tags


def features(name, w):
    """What the directed set of scoring set `name` at band w exists for: each feature occurs
    at least MIN_COUNT times in the oracle's own results (tests/test_sw_route_cases.py).
    Left out only where the options rule the feature out: pen_clip 0 never goes to the read
    end (gscore <= score always) and pen_clip 200 hardly ever clips; zdrop 10 stops at the
    first mismatch, before any tie or low-score tail; a = 15 lets random sequence align
    through the N tails, the clipped sides and the low-score reads; zdrop 0 has no z-drop."""
    f = {"retry_L", "retry_R", "band<=40", "pass1"}
    if name != "zdrop10":   # (a stop on one side undoes a planted retry on both)
        f.add("retry_LR")
    if 24 <= w <= 81:
        f.add("band41-80")
    if w >= 64:
        f.add("band>80")
    if name != "clip0":
        f |= {"toend_L", "toend_R"}
    if name not in ("clip200", "a15"):
        f |= {"clip_L", "clip_R"}
    if name not in ("clip200", "zdrop10", "a15"):
        f.add("tie")
    if name not in ("clip0", "zdrop10", "a15"):
        f.add("pass0")
    if name != "zdrop0":
        f.add("zstop")
    return f


MIN_COUNT = 20


def count_features(tr, orc):
    """Occurrences of each feature in trace_all / oracle_all results."""
    c = {k: 0 for k in ("retry_L", "retry_R", "retry_LR", "band<=40", "band41-80", "band>80", "toend_L", "toend_R",
                        "clip_L", "clip_R", "tie", "zstop", "pass0", "pass1")}
    for (sd, reg), (res, wreg, w2) in zip(tr, orc):
        rl, rr = sd[0]["retry"], sd[1]["retry"]
        c["retry_L"] += rl and not rr
        c["retry_R"] += rr and not rl
        c["retry_LR"] += rl and rr
        c["band<=40" if w2 <= 40 else ("band41-80" if w2 <= 80 else "band>80")] += 1
        for i, n in ((0, "L"), (1, "R")):
            c["toend_" + n] += sd[i]["end"] == "toend"
            c["clip_" + n] += sd[i]["end"] == "clip"
            c["tie"] += sd[i]["tie"]
            c["zstop"] += sd[i]["zstop"]
        c["pass%d" % res[8]] += 1
    return c


# ---------------------------------------------------------------------------
# the oracle, per task and per side
def _u8(a):
    a = np.ascontiguousarray(a, np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8))


def _extend(o, q, t, w, clip, h0, zdrop):
    L = ob.sw_lib()
    mat = (C.c_int8 * 25)()
    L.osw_fill_scmat(o.a, o.b, mat)
    outs = [C.c_int() for _ in range(5)]
    qa, qp = _u8(q if len(q) else np.zeros(1, np.uint8))
    ta, tp = _u8(t if len(t) else np.zeros(1, np.uint8))
    sc = L.osw_extend(len(q), qp, len(t), tp, 5, mat, o.o_del, o.e_del, o.o_ins, o.e_ins, w, clip, zdrop, h0,
                      *[C.byref(x) for x in outs])
    return (sc,) + tuple(x.value for x in outs)   # score, qle, tle, gtle, gscore, max_off


def cal_max_gap(o, qlen):
    l = max(int((qlen * o.a - o.o_del) / o.e_del + 1.), int((qlen * o.a - o.o_ins) / o.e_ins + 1.), 1)
    return min(l, o.w << 1)


def trace_task(o, q, lr, strand, qbeg, rbeg, slen):
    """mem_chain2aln's two band-try loops of one seed with the oracle's osw_extend, side by side
    with what each side decided: retry (asked for 2w), end ("none" no bases, "clip", "toend"),
    tie (gscore == score - pen_clip), zstop (the last try differs from its run with zdrop 0).
    Also the region (qb, qe, score), to be held against osw_task."""
    S = strand_seq(lr, strand)
    lq, L = len(q), len(S)
    rmax0 = max(0, rbeg - (qbeg + cal_max_gap(o, qbeg)))
    rmax1 = min(L, rbeg + slen + (lq - qbeg - slen) + cal_max_gap(o, lq - qbeg - slen))
    sides = []
    score = slen * o.a
    qb, qe = 0, lq
    for side in (0, 1):
        if side == 0:
            qs, ts, clip, h0 = q[:qbeg][::-1], S[rmax0:rbeg][::-1], o.pen_clip5, slen * o.a
        else:
            qs, ts, clip, h0 = q[qbeg + slen:], S[rbeg + slen:rmax1], o.pen_clip3, score
        if len(qs) == 0:
            sides.append(dict(retry=False, end="none", tie=False, zstop=False))
            continue
        prev, r, aw, retry = (-1 if side == 0 else h0), None, o.w, False
        for i in range(2):
            aw = o.w << i
            r = _extend(o, qs, ts, aw, clip, h0, o.zdrop)
            if r[0] == prev or r[5] < (aw >> 1) + (aw >> 2):
                break
            prev = r[0]
            retry = retry or i == 0
        sc, qle, tle, gtle, gscore, max_off = r
        clipped = gscore <= 0 or gscore <= sc - clip
        zstop = o.zdrop > 0 and _extend(o, qs, ts, aw, clip, h0, 0) != r
        sides.append(dict(retry=retry, end="clip" if clipped else "toend", tie=gscore > 0 and gscore == sc - clip,
                          zstop=zstop))
        score = sc
        if side == 0:
            qb = qbeg - qle if clipped else 0
        else:
            qe = qbeg + slen + qle if clipped else lq
    return sides, (qb, qe, score)


def trace_all(d, o):
    out = []
    for t in range(len(d.t_sr)):
        s, l = int(d.t_sr[t]), int(d.t_lr[t])
        out.append(trace_task(o, d.sr_seq[d.sr_off[s]:d.sr_off[s + 1]], d.lr_seq[d.lr_off[l]:d.lr_off[l + 1]],
                              int(d.t_strand[t]), int(d.t_qbeg[t]), int(d.t_rbeg[t]), int(d.t_slen[t])))
    return out


def oracle_all(d, o):
    """osw_task over every task: (comparison tuple as sw_util.oracle_results, region w, last band w2)."""
    L = ob.sw_lib()
    out = []
    r = ob.OswResult()
    for t in range(len(d.t_sr)):
        s, l = int(d.t_sr[t]), int(d.t_lr[t])
        qa, qp = _u8(d.sr_seq[d.sr_off[s]:d.sr_off[s + 1]])
        la, lp = _u8(d.lr_seq[d.lr_off[l]:d.lr_off[l + 1]])
        rc = L.osw_task(C.byref(o), qp, len(qa), lp, len(la), int(d.t_strand[t]), int(d.t_qbeg[t]), int(d.t_rbeg[t]),
                        int(d.t_slen[t]), C.byref(r))
        assert rc == 0
        cg = "".join(f"{x >> 4}{'MIDNSHP=X'[x & 15]}" for x in r.cigar[:r.n_cigar])
        out.append(((r.qb, r.qe, r.rb, r.re, r.score, r.truesc, r.pos, cg, int(getattr(r, "pass"))), r.w, r.w2))
    return out


# ---------------------------------------------------------------------------
# the routing rule
def ext_kernel(wb, qmax, w, ext80_lane=False):
    """sw_launch_extend's ladder for one band try of width wb."""
    if wb <= 32:
        return "sw_ext_phase_kernel<32>"
    if wb <= 40:
        return "sw_ext_phase_kernel<40>"
    if wb <= 64:
        return "sw_ext_phase_kernel<64>"
    if wb <= 80:
        return "sw_ext_phase_kernel<80>" if ext80_lane else "sw_ext_wave_kernel"
    return "sw_ext_wide_kernel<true>" if eh_hbm(qmax, w) else "sw_ext_wide_kernel<false>"


def eh_hbm(qmax, w):
    """pr_sw_launch: the general CIGAR kernel's row ((qmax+1) words + padded query per lane) or
    the wide extension kernel's ((qmax+2) words per lane) does not fit the LDS; either moves both
    kernels' rows to HBM."""
    lds_glob = (qmax + 1) * 64 * 4 + 64 * ((qmax + 8) & ~3)
    lds_wide = (qmax + 2) * 64 * 4
    return lds_glob + 256 > LDS_BYTES or ((w << 1) > 80 and lds_wide + 256 > LDS_BYTES)


def packed_on(o, nopk=False):
    return max(o.o_del, o.o_ins, o.e_del, o.e_ins) <= 32 and not nopk


def infer_bw(l1, l2, score, a, q, r):
    if l1 == l2 and l1 * a - score < (q + r - a) << 1:
        return 0
    w = int((min(l1, l2) * a - score - q) / r + 2.)
    return max(w, abs(l1 - l2))


def first_cigar_band(o, res, wreg):
    """(band of the first ksw_global2 pass, no-DP flag) from a task's region: glob_w2 / glob_pass_w."""
    qb, qe, rb, re, truesc = res[0], res[1], res[2], res[3], res[5]
    lqq, rlen = qe - qb, re - rb
    w2 = max(infer_bw(lqq, rlen, truesc, o.a, o.o_del, o.e_del), infer_bw(lqq, rlen, truesc, o.a, o.o_ins, o.e_ins))
    if w2 > o.w:
        w2 = min(w2, wreg)
    w2 = min(w2, o.w << 2)
    if lqq <= 0 or rlen <= 0:
        return -1, False
    if lqq == rlen and w2 == 0:
        return 0, True
    mn = min(lqq, rlen)
    max_gap = max(int((mn * o.a - o.o_ins) / o.e_ins + 1.), int((mn * o.a - o.o_del) / o.e_del + 1.), 1)
    dl = abs(rlen - lqq)
    return max(min((max_gap + dl + 1) >> 1, w2), dl + 3), False


def route(flags, o, qmax, lq, qbeg, slen, res=None, wreg=None, nopk=False, ext80_lane=False, split=False,
          pk_win=8, bt_win=8):
    """Names of the kernels one single-seed task went through, from its pr_sw_task_flags byte.
    res / wreg (the task's result tuple and region band) are needed only without the packed
    kernel, where the CIGAR class is not left in the byte."""
    pk = packed_on(o, nopk)
    names = []
    for side, ql in ((0, qbeg), (1, lq - qbeg - slen)):
        if ql <= 0:
            continue
        pk_ext = pk and o.w <= 40 and ql <= PK_QMAX and o.a * lq <= 2047   # pk_ext_key
        if pk_ext:
            names.append("sw_ext_pk_kernel<40,%s>" % ("true" if o.a * qmax <= 511 else "false"))
        if not pk_ext or flags & (8 << side):
            names.append(ext_kernel(o.w, qmax, o.w, ext80_lane) + "@0")
        if flags & (1 << side):
            names.append(ext_kernel(o.w << 1, qmax, o.w, ext80_lane) + "@1")
    gen = "sw_global_kernel<%s>" % ("true" if eh_hbm(qmax, o.w) else "false")
    if pk:
        if flags & 0x40:
            names.append("sw_global_ring_kernel<40>")
        elif flags & 0x80:
            names.append("sw_global_ring_kernel<80>")
        elif res is not None and pk_cigar_key(o, res, wreg) < 0:
            pass   # classed general by the ordering pass (bit 4 below): no packed run
        else:
            if split:
                names += ["sw_global_pk_kernel<40,16>", "sw_global_pk_bt_kernel<%d>" % bt_win]
            else:
                names.append("sw_global_pk_kernel<40,%d>" % pk_win)
        if flags & 4:
            names.append(gen)
    else:
        c = _class(o, res, wreg)
        names.append(("sw_global_ring_kernel<40>", "sw_global_ring_kernel<80>", gen)[c])
        if c < 2 and flags & 4:
            names.append(gen)
    if flags & 0x20:
        names.append(gen + "@overflow")
    return names


def _class(o, res, wreg):
    ww, _ = first_cigar_band(o, res, wreg)
    return 0 if ww <= 40 else (1 if ww <= 80 else 2)


def pk_cigar_key(o, res, wreg):
    """pk_key: band * 256 + query length of a task the packed CIGAR kernel takes, else -1."""
    lqq, rlen = res[1] - res[0], res[3] - res[2]
    if lqq > PK_QMAX or rlen > PK_TMAX:
        return -1
    ww, nogap = first_cigar_band(o, res, wreg)
    return -1 if ww <= 0 or nogap or ww > 40 else ww * 256 + lqq


# ---------------------------------------------------------------------------
# the case sets of tests/test_sw_route_cases.py (oracle alone) and tests/test_sw_routes_gpu.py
W_ROWS = (8, 24, 33, 40, 41, 64, 65, 80, 81, 100)
SETS = ([("sr", w, False) for w in W_ROWS] + [("finish", 30, False)] +
        [(n, w, False) for n in SCORING if n != "sr" for w in (8, 40, 100)] +
        [("sr", 41, True), ("sr", 100, True)])

_cache = {}


def case(name, w, long_reads=False):
    """The mixed batch of one set with the oracle's results, built once per process:
    dict(o, d, tags, orc, qmax)."""
    key = (name, w, long_reads)
    if key not in _cache:
        o = scoring(name, w)
        small = w > 200   # the w = 1000 row: one small case
        d, tags = mixed(o, seed=1, long_reads=long_reads, reps=1 if small else 12, n_synth=20 if small else 200)
        _cache[key] = dict(o=o, d=d, tags=tags, orc=oracle_all(d, o), qmax=int(np.diff(d.sr_off).max()))
    return _cache[key]


def zdrop0_twin(c):
    """The same batch under the same options but zdrop 0, with the oracle's results for them:
    the reads that stop on z-drop in c go on to the read end here."""
    if "twin" not in c:
        o = ob.OswOpts.from_buffer_copy(c["o"])
        o.zdrop = 0
        c["twin"] = dict(o=o, d=c["d"], tags=c["tags"], orc=oracle_all(c["d"], o), qmax=c["qmax"])
    return c["twin"]


TWINS = [("sr", 8), ("sr", 40), ("sr", 100), ("finish", 30), ("bwa", 40), ("pen32", 40)]


def case_trace(c):
    if "tr" not in c:
        c["tr"] = trace_all(c["d"], c["o"])
    return c["tr"]


def predict_flags(c, nopk=False):
    """The pr_sw_task_flags byte the oracle's results imply for every task: retries (1, 2), a
    query N under the packed extension (8, 16), the CIGAR class of tasks outside the packed
    kernel (0x40, 0x80, 4).  Hand-ons to the general kernel (4) and the overflow pass (0x20)
    depend on the kernels' own limits and are not predicted."""
    o, d = c["o"], c["d"]
    pk = packed_on(o, nopk)
    lqs = np.diff(d.sr_off)
    out = np.zeros(len(d.t_sr), np.uint8)
    for t, ((sd, reg), (res, wreg, w2)) in enumerate(zip(case_trace(c), c["orc"])):
        s = int(d.t_sr[t])
        q = d.sr_seq[d.sr_off[s]:d.sr_off[s + 1]]
        lq, qbeg, slen = int(lqs[s]), int(d.t_qbeg[t]), int(d.t_slen[t])
        f = 0
        for side, (ql, part) in enumerate(((qbeg, q[:qbeg]), (lq - qbeg - slen, q[qbeg + slen:]))):
            if sd[side]["retry"]:
                f |= 1 << side
            if pk and o.w <= 40 and 0 < ql <= PK_QMAX and o.a * lq <= 2047 and (part == 4).any():
                f |= 8 << side
        if pk and pk_cigar_key(o, res, wreg) < 0:
            f |= (0x40, 0x80, 4)[_class(o, res, wreg)]
        out[t] = f
    return out


PREDICTED = 0x01 | 0x02 | 0x08 | 0x10 | 0x40 | 0x80


def route_counts(c, flags, **kw):
    """Tasks per kernel name over the whole case (route() of every task)."""
    d, o = c["d"], c["o"]
    lqs = np.diff(d.sr_off)
    n = {}
    for t, (res, wreg, w2) in enumerate(c["orc"]):
        for k in route(int(flags[t]), o, c["qmax"], int(lqs[d.t_sr[t]]), int(d.t_qbeg[t]), int(d.t_slen[t]), res=res,
                       wreg=wreg, **kw):
            n[k] = n.get(k, 0) + 1
    return n


def row_kernels(o, qmax, nopk=False, ext80_lane=False, split=False, pk_win=8, bt_win=8):
    """The kernels a mixed case at these options must reach with MIN_COUNT tasks each: the
    launcher's ladder by band (sw_launch_extend / sw_launch_global)."""
    pk = packed_on(o, nopk)
    names = {ext_kernel(o.w, qmax, o.w, ext80_lane) + "@0", ext_kernel(o.w << 1, qmax, o.w, ext80_lane) + "@1"}
    # with the packed CIGAR kernel on, the band <= 40 ring kernel is left the tasks without a DP
    # (equal lengths and an inferred band of 0: needs o + e > a for both gap kinds) and the
    # regions longer than 255 bp
    if not pk or min(o.o_del + o.e_del, o.o_ins + o.e_ins) > o.a or qmax >= 600:
        names.add("sw_global_ring_kernel<40>")
    if pk and o.w <= 40:
        names.add("sw_ext_pk_kernel<40,%s>" % ("true" if o.a * qmax <= 511 else "false"))
    if pk and o.w <= 81:   # (at w = 100 the directed reads mostly outgrow its 255 bp)
        names |= ({"sw_global_pk_kernel<40,16>", "sw_global_pk_bt_kernel<%d>" % bt_win} if split
                  else {"sw_global_pk_kernel<40,%d>" % pk_win})
    if 24 <= o.w <= 81:
        names.add("sw_global_ring_kernel<80>")
    if o.w >= 64:
        names.add("sw_global_kernel<%s>" % ("true" if eh_hbm(qmax, o.w) else "false"))
    return names


# frame-edge batches: perfect-match reads whose score is the largest a frame holds
def frame_edge(which):
    """(o, Dataset, tags, {tag: score}) of one frame-edge batch.  "smallh7" / "smallh1": a * lq =
    511 = 511 * 128 + 127 >> 7, the packed extension's one-accumulator row maximum (a = 7 with
    73 bp reads; a = 1 with a 511 bp read, qbeg 200, slen 56, both sides <= 255).  "pk2047":
    a * lq either side of the packed frame's 2047: a = 8 x 255 = 2040 and a = 9 x 227 = 2043
    inside, a = 9 x 228 = 2052 outside, neighbours in one batch (2047 = 23 x 89 itself cannot be
    reached with a <= 15 and reads <= 1000 bp).  "w8190": a = 15 x 546 = 8190 under the 13-bit
    DP words."""
    rng = np.random.default_rng(7)
    if which == "smallh7":
        o = make_opts(a=7, b=11, o_del=6, o_ins=6, e_del=2, e_ins=2, w=40, per_base=3.0)
        specs = [(73, None, None)] * 24 + [(73, 0, 25), (73, 48, 25), (73, 0, 73)]
        d, tags = perfect(11, specs, filler=40, filler_max=73)
        return o, d, tags, {"perfect_73": 511}
    if which == "smallh1":
        o = scoring("bwa", 40)
        specs = [(511, 200, 56)] * 16 + [(511, 255, 19), (511, 236, 20)] * 2 + [(int(x), None, None) for x in rng.integers(60, 300, 40)]
        d, tags = perfect(12, specs)
        return o, d, tags, {"perfect_511": 511}
    if which == "pk2047":
        o = make_opts(a=9, b=11, o_del=6, o_ins=6, e_del=2, e_ins=2, w=40, per_base=4.0)
        specs = [(227, None, None), (228, None, None)] * 24 + [(int(x), None, None) for x in rng.integers(40, 227, 30)]
        d, tags = perfect(13, specs)
        return o, d, tags, {"perfect_227": 2043, "perfect_228": 2052}
    if which == "pk2040":
        o = make_opts(a=8, b=11, o_del=6, o_ins=6, e_del=2, e_ins=2, w=40, per_base=4.0)
        specs = [(255, None, None)] * 24 + [(255, 0, 20), (255, 235, 20)] + [(int(x), None, None) for x in rng.integers(40, 255, 30)]
        d, tags = perfect(14, specs)
        return o, d, tags, {"perfect_255": 2040}
    if which == "w8190":
        o = scoring("a15", 40)
        specs = [(546, None, None)] * 22 + [(546, 0, 30), (546, 516, 30)] + [(int(x), None, None) for x in rng.integers(40, 546, 30)]
        d, tags = perfect(15, specs)
        return o, d, tags, {"perfect_546": 8190}
    raise KeyError(which)


FRAME_EDGES = ("smallh7", "smallh1", "pk2040", "pk2047", "w8190")

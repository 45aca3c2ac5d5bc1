"""Reads and long reads built for the on-chip chaining (seed_chain.h), shared by
test_seed_chain_host.py and test_seed_chain_gpu.py.

`family(seg, n0, ...)` plants copies of a segment's prefix so that the exact read seg[:24] has
n0 + 1 occurrences, seg[:25] n0 and seg[:26] n0 - 1 (one copy ends after 24 bases, one after
25, the rest after 30; every copy is followed by a base that differs from the segment's next
one).  With every copy in one long read the occurrences are one range's; with `spread` every
copy lies in its own (long read, strand), so the same three reads have n0 + 1, n0 and n0 - 1 ranges.
"""
import numpy as np

COMP = np.array([3, 2, 1, 0, 4], np.uint8)


def rc(a):
    return COMP[np.asarray(a, np.uint8)[::-1]]


def _unit(seg, p, rng, avoid=()):
    """seg[:p], a terminator that differs from seg[p] (and from `avoid`), three random bases"""
    bad = {int(seg[p]), *avoid}
    t = next(b for b in range(4) if b not in bad)
    return np.concatenate([seg[:p], [t], rng.integers(0, 4, 3)]).astype(np.uint8)


def family(seg, n0, rng, spread=False, pre_avoid=(), term_avoid=()):
    """-> list of long reads (uint8 arrays)"""
    plens = [24, 25] + [30] * (n0 - 1)
    units = []
    for p in plens:
        pre = next(b for b in range(4) if b not in set(pre_avoid))
        units.append(np.concatenate([[pre], _unit(seg, p, rng, term_avoid)]).astype(np.uint8))
    if not spread:
        out, cur = [], []
        for u in units:   # long reads of 2 to 2.5 kb
            cur.append(u)
            if sum(len(x) for x in cur) > 2500:
                out.append(np.concatenate(cur))
                cur = []
        if cur:
            out.append(np.concatenate(cur))
        return out
    out = []
    for k in range(0, len(units), 2):   # a long read holds one copy per strand
        parts = [rng.integers(0, 4, 20).astype(np.uint8), units[k], rng.integers(0, 4, 20).astype(np.uint8)]
        if k + 1 < len(units):
            parts += [rc(units[k + 1]), rng.integers(0, 4, 20).astype(np.uint8)]
        out.append(np.concatenate(parts))
    return out


def chained_families(total, spread, rng):
    """Families whose three reads have total - 1, total and total + 1 occurrences (spread: as many
    ranges).  One SMEM takes at most -c 500 occurrences, so beyond 400 further segments add 400
    each and a read is the first segment's prefix followed by theirs.  No match runs across a
    junction: a copy's terminator differs from the next segment's first base, the base before a
    copy from the previous segment's last bases, and the next segment's first base from the bases
    that follow the prefix in the longer copies.  -> long reads, {-1, 0, 1: read}"""
    nb = (total - 1) // 400
    segs = [rng.integers(0, 4, 40).astype(np.uint8)]
    for k in range(nb):
        prev = segs[-1]
        follow = {int(prev[24]), int(prev[25]), int(prev[26])} if k == 0 else {int(prev[30])}
        while True:
            sg = rng.integers(0, 4, 40).astype(np.uint8)
            if int(sg[0]) not in follow:
                break
        segs.append(sg)
    lrs = []
    for k, sg in enumerate(segs):
        last = {int(segs[k - 1][x]) for x in ((23, 24, 25) if k == 1 else (29,))} if k else set()
        pre_avoid = tuple(last) if len(last) < 4 else ()
        term_avoid = (int(segs[k + 1][0]),) if k + 1 < len(segs) else ()
        lrs += family(sg, total - 400 * nb if k == 0 else 401, rng, spread=spread, pre_avoid=pre_avoid, term_avoid=term_avoid)
    reads = {d: np.concatenate([segs[0][:25 - d]] + [sg[:30] for sg in segs[1:]]) for d in (-1, 0, 1)}
    return lrs, reads


def build(caps, seed=7):
    """A text and reads around the capacities caps = [(seeds, ranges), ...] (chained_families for
    each).  -> lr_seq, lr_off, sr_seq, sr_off, labels (read index by name: seeds-1/+0/+1 and
    ranges-1/+0/+1 with the set's number appended)"""
    rng = np.random.default_rng(seed)
    lrs = [rng.integers(0, 4, 1500).astype(np.uint8) for _ in range(3)]
    # a 300-base unit repeated with 3 % differences: many chains per range, opened before the
    # head, between two chains and after the tail, weights that tie
    unit = rng.integers(0, 4, 300).astype(np.uint8)
    for _ in range(2):
        rep = np.tile(unit, 6)
        m = rng.random(len(rep)) < 0.03
        rep[m] = rng.integers(0, 4, int(m.sum()))
        lrs.append(rep.astype(np.uint8))
    # U + U with U of 45 bases once in the text: two chains of one range with equal pos and equal
    # weight that cannot merge (45 bases apart on the read, beyond -w 40 / 30), so only creation
    # order decides which comes first.  The bases around U in the text stop both SMEMs at U's ends
    # (before U: not U's last base, which precedes the read's second U; after: not U's first)
    U = rng.integers(0, 4, 45).astype(np.uint8)
    lrs.append(np.concatenate([rng.integers(0, 4, 400), [(int(U[44]) + 1) % 4], U, [(int(U[0]) + 1) % 4],
                               rng.integers(0, 4, 400)]).astype(np.uint8))
    # A + I + B with B = A[20:] + C and the text A + C: two seeds of one chain 40 apart on the read
    # and 20 on the text, so the chain's reference cover (50) is below its query cover (60); D (55
    # bases, another long read) sorts before that chain only by the smaller of the two covers
    rng2 = np.random.default_rng(seed + 1000)   # (its own stream: the families below keep theirs)
    A, C, D, ins = (rng2.integers(0, 4, k).astype(np.uint8) for k in (30, 20, 55, 10))
    ins[0] = (int(C[0]) + 1) % 4    # the first seed ends with A
    ins[9] = (int(A[19]) + 1) % 4   # the second starts with B
    lrs.append(np.concatenate([rng2.integers(0, 4, 300), A, C, [(int(D[0]) + 1) % 4], rng2.integers(0, 4, 300)]).astype(np.uint8))
    lrs.append(np.concatenate([rng2.integers(0, 4, 300), [(int(C[19]) + 1) % 4], D, rng2.integers(0, 4, 300)]).astype(np.uint8))
    wr_lt = np.concatenate([A, ins, A[20:], C, D])
    n_noisy_text = len(lrs) - 3
    edge = {}
    for ci, (sc, rcap) in enumerate(caps):
        for name, total, spread in (("seeds", sc, False), ("ranges", rcap, True)):
            fl, fr = chained_families(total, spread, rng)
            lrs += fl
            for k in (-1, 0, 1):
                edge[f"{name}{k:+d}.{ci}"] = fr[k]
    lr_off = np.zeros(len(lrs) + 1, np.int64)
    lr_off[1:] = np.cumsum([len(x) for x in lrs])
    lr_seq = np.concatenate(lrs).astype(np.uint8)

    reads, labels = [], {}

    def add(name, r):
        labels[name] = len(reads)
        reads.append(np.asarray(r, np.uint8))

    for name, r in edge.items():
        add(name, r)
    add("equal_pos", np.concatenate([U, U]))
    add("wr_lt", wr_lt)
    add("n_inside", np.concatenate([lrs[0][100:160], [4], lrs[0][161:230]]))
    add("short", lrs[0][10:19])
    add("short11", lrs[1][10:21])
    add("no_smem", rng.integers(0, 4, 11).astype(np.uint8))
    add("empty", np.zeros(0, np.uint8))
    add("all_n", np.full(40, 4, np.uint8))
    # >= 440 bases: mem_flt_chained_seeds, the lane path (800: the batch's reads get 1,600 output
    # slots each, enough for every seed of the largest edge read)
    add("mr_length", lrs[1][200:1000])
    text_len = int(lr_off[n_noisy_text])   # noisy reads over the random and the repeated long reads
    for k in range(90 - len(reads) % 64 + 64):   # (the batch's last wave partly filled: n % 64 = 26)
        p = int(rng.integers(0, text_len - 200))
        r = lr_seq[p:p + int(rng.integers(60, 180))].copy()
        if k % 3:
            m = rng.random(len(r)) < 0.06
            r[m] = rng.integers(0, 4, int(m.sum()))
        if k % 4 == 0:
            r = rc(r)
        add(f"noisy{k}", r)
    sr_off = np.zeros(len(reads) + 1, np.int64)
    sr_off[1:] = np.cumsum([len(x) for x in reads])
    sr_seq = np.concatenate(reads).astype(np.uint8) if sr_off[-1] else np.zeros(0, np.uint8)
    return lr_seq, lr_off, sr_seq, sr_off, labels

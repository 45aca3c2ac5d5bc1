"""Plain-Python restatement of the siamaera stage, TEST INFRASTRUCTURE ONLY.

Written from the stage's definition, not from csrc/siam_core.h: a brute-force
seed scan over every anti-diagonal and a row-by-row ksw_extend2 whose cells carry
(matches, cols).  The library's host path and the kernels are held equal to it.

Second half: the seeded inputs the host and GPU tests share (extension pairs, known-answer
reads, the mixed batch with planted siamaeras).
"""
from __future__ import annotations

import functools
import random

import numpy as np

PASS1 = dict(a=1, b=4, o=3, e=2, w=31, zdrop=25, word=28)
PASS2 = dict(a=1, b=2, o=0, e=3, w=31, zdrop=100, word=28)
MAX_SEEDS, MAX_HSPS, MAX_LEN = 1024, 64, 131072
SEED_OVERFLOW, HSP_OVERFLOW, TOO_LONG = 1, 2, 4
KEEP, TRIM, DROP = 0, 1, 2

_CODE = {c: k for k, c in enumerate("ACGT")}


def nt4(s):
    if isinstance(s, bytes):
        s = s.decode()
    return [_CODE.get(c.upper(), 4) for c in s]


def comp(c):
    return 3 - c if c < 4 else c


def rc(s: str) -> str:
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


# ---------------------------------------------------------------------------- seeds (§1a)
def seeds(S, word):
    """Every maximal run (i + t, p - t) of matching cells with len >= word, as (i, p, len) in
    (len desc, i asc, p asc) order.  Brute force: every anti-diagonal d = i + p."""
    L = len(S)
    s = np.asarray(S, np.int64)
    out = []
    for d in range(2 * L - 1):
        lo, hi = max(0, d - (L - 1)), min(L - 1, d)
        i = np.arange(lo, hi + 1)
        a, b = s[i], s[d - i]
        m = (a < 4) & (b < 4) & (a + b == 3)
        if not m.any():
            continue
        pad = np.concatenate(([0], m.astype(np.int8), [0]))
        edge = np.flatnonzero(np.diff(pad))
        for st, en in zip(edge[0::2], edge[1::2]):
            if en - st >= word:
                out.append((int(lo + st), int(d - (lo + st)), int(en - st)))
    out.sort(key=lambda x: (-x[2], x[0], x[1]))
    return out


# ---------------------------------------------------------------------------- extension (§1c, §1d)
def extend(q, t, h0, a, b, o, e, w, zdrop, word=None):
    """ksw_extend2 (o_del = o_ins = o, e_del = e_ins = e, end_bonus 0) over nt4 lists q, t ->
    (score, qle, tle, matches, cols)."""
    qlen, tlen = len(q), len(t)
    if qlen == 0 or tlen == 0:
        return h0, 0, 0, 0, 0
    oe = o + e

    def score(x, y):
        if x > 3 or y > 3:
            return -1
        return a if x == y else -b

    # eh[j] = (h, e) with each value a (value, matches, cols) triple
    Z = (0, 0, 0)
    H = [Z] * (qlen + 1)
    E = [Z] * (qlen + 1)
    H[0] = (h0, 0, 0)
    if h0 > oe:
        H[1] = (h0 - oe, 0, 1)
    j = 2
    while j <= qlen and H[j - 1][0] > e:
        H[j] = (H[j - 1][0] - e, 0, j)
        j += 1
    # the band cap: the longest gap the best possible score pays for
    mx = max(a, -b, -1, 0)
    cap = max(int((qlen * mx - o) / e + 1.0), 1)
    w = min(w, cap)
    best, best_i, best_j, best_cell = h0, -1, -1, (h0, 0, 0)
    beg, end = 0, qlen
    for i in range(tlen):
        f = Z
        mm, mj, mcell = 0, -1, Z
        beg = max(beg, i - w)
        end = min(end, i + w + 1, qlen)
        if beg == 0:
            v = h0 - (o + e * (i + 1))
            h1 = (v, 0, i + 1) if v > 0 else Z
        else:
            h1 = Z
        ti = t[i]
        for j in range(beg, end):
            M, ee = H[j], E[j]
            H[j] = h1
            if M[0]:
                qj = q[j]
                M = (M[0] + score(qj, ti), M[1] + (1 if qj < 4 and qj == ti else 0), M[2] + 1)
            else:
                M = Z
            h = ee if ee[0] >= M[0] else M            # h takes e when e >= M
            if f[0] >= h[0]:                          # then f when f >= max(M, e)
                h = f
            h1 = h
            if h[0] >= mm:                            # last column on ties
                mm, mj, mcell = h[0], j, h
            op = M[0] - oe
            if op < 0:
                op = 0
            if op >= ee[0] - e:                       # the opening from M wins ties
                E[j] = (op, M[1], M[2] + 1)
            else:
                E[j] = (ee[0] - e, ee[1], ee[2] + 1)
            if op >= f[0] - e:
                f = (op, M[1], M[2] + 1)
            else:
                f = (f[0] - e, f[1], f[2] + 1)
        H[end] = h1
        E[end] = Z
        if mm == 0:
            break
        if mm > best:                                 # strictly greater updates the maximum
            best, best_i, best_j, best_cell = mm, i, mj, mcell
        elif zdrop > 0:
            di, dj = i - best_i, mj - best_j
            if di > dj:
                if best - mm - (di - dj) * e > zdrop:
                    break
            elif best - mm - (dj - di) * e > zdrop:
                break
        j = beg
        while j < end and H[j][0] == 0 and E[j][0] == 0:
            j += 1
        beg = j
        j = end
        while j >= beg and H[j][0] == 0 and E[j][0] == 0:
            j -= 1
        end = min(j + 2, qlen)
    return best, best_j + 1, best_i + 1, best_cell[1], best_cell[2]


# ---------------------------------------------------------------------------- alignments (§1b-e, g)
def produce(S, prm):
    """Every alignment produced for read S (nt4 list), in order of production, as
    (qas, qae, sas, sae, length, matches, score); and the status flags."""
    L = len(S)
    if L > MAX_LEN:
        return [], TOO_LONG
    sd = seeds(S, prm["word"])
    if len(sd) > MAX_SEEDS:
        return [], SEED_OVERFLOW
    out = []
    al = {k: prm[k] for k in ("a", "b", "o", "e", "w", "zdrop")}
    for i, p, ln in sd:
        q0, q1, s0, s1 = i + 1, i + ln, p - ln + 2, p + 1   # the seed's box, 1-based
        if any(h[0] <= q0 and q1 <= h[1] and h[3] <= s0 and s1 <= h[2] for h in out):
            continue
        if len(out) == MAX_HSPS:
            return [], HSP_OVERFLOW
        lq = [S[i - 1 - k] for k in range(i)]
        lt = [comp(S[p + 1 + k]) for k in range(L - 1 - p)]
        ls, lqle, ltle, lm, lc = extend(lq, lt, ln * prm["a"], **al)
        rq = [S[i + ln + k] for k in range(L - i - ln)]
        rt = [comp(S[p - ln - k]) for k in range(p - ln + 1)]
        rs, rqle, rtle, rm, rcn = extend(rq, rt, ls, **al)
        out.append((i - lqle + 1, i + ln + rqle, p + ltle + 1, p - ln - rtle + 2, ln + lc + rcn, ln + lm + rm, rs))
    return out, 0


def select(hs, min_idy):
    """Identity threshold, then -culling_limit 1."""
    kept = [h for h in hs if 100.0 * h[5] >= min_idy * h[4]]
    out = []
    for x, h in enumerate(kept):
        culled = False
        for y, g in enumerate(kept):
            if y != x and g[0] <= h[0] and h[1] <= g[1] and (g[6] > h[6] or (g[6] == h[6] and y < x)):
                culled = True
        if not culled:
            out.append(h)
    return out


def hsps(S, prm=PASS1, min_idy=97.5):
    hs, status = produce(S, prm)
    return ([] if status else select(hs, min_idy)), status


# ---------------------------------------------------------------------------- decision (§1h)
def spurious(hs, L, seq_min_len=150):
    t = (int(0.05 * L + 0.5) or 1) + 1
    out = []
    for k, b in enumerate(hs):
        if b[0] == b[3] and b[1] == b[2]:
            if b[1] - b[0] > 0.7 * seq_min_len:
                out.append(b)
        else:
            for i, o in enumerate(hs):
                if i != k and abs(b[0] - o[3]) < t and abs(b[1] - o[2]) < t:
                    out.append(b)
    return out


def decide(L, pass1, pass2=(), seq_min_len=150, term_ignore_len=10, trim=5, filter_inconclusive=True):
    """siamaera:258-448 from pass 1's kept alignments and pass 2's (a list, or a callable that
    is asked only when pass 2 runs) -> (action, from, to, inconclusive)."""
    keep = (KEEP, 0, L, False)
    if L < seq_min_len or not pass1:
        return keep
    b = list(pass1)
    if len(b) > 2:
        b = spurious(b, L, seq_min_len)
    if len(b) > 2:
        re = list(pass2() if callable(pass2) else pass2)
        if re:
            b = re
    if len(b) > 2:
        b = spurious(b, L, seq_min_len)
    lim = term_ignore_len + 1
    clamp = lambda v: max(0, min(L, v))
    if len(b) == 1:
        qas, qae = b[0][0], b[0][1]
        if qas <= lim:
            return TRIM, clamp(int((qae - qas - 1) / 2 + qas + trim + 0.5)), L, False
        if qae > L - lim:
            return TRIM, 0, clamp(int((qae - qas - 1) / 2 + qas - trim + 0.5)), False
        return keep
    if len(b) == 2:
        for h in b:
            if h[0] <= lim:
                return TRIM, clamp(h[3] - 1 + trim), L, False
            if h[1] > L - lim:
                return TRIM, 0, clamp(h[2] - trim), False
        return keep
    if len(b) > 2:
        return (DROP if filter_inconclusive else KEEP), 0, L, True
    return keep


def run(S, aln_min_idy=97.5, **kw):
    """One read through both passes -> (action, from, to, inconclusive, status)."""
    L = len(S)
    if L < kw.get("seq_min_len", 150):
        return KEEP, 0, L, False, 0
    h1, st = hsps(S, PASS1, aln_min_idy)
    if st:
        return KEEP, 0, L, False, st
    st2 = [0]

    def second():
        h2, st2[0] = hsps(S, PASS2, aln_min_idy - 2)
        return h2
    d = decide(L, h1, second, **kw)
    if st2[0]:
        return KEEP, 0, L, False, st2[0]
    return (*d, 0)


# ============================================================================ shared test inputs
SEED_EDGE_LENGTHS = (27, 28, 29, 31, 32, 33, 64, 65, 150, 1000)


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, rate, n_frac=0.0):
    """Substitutions and indels at `rate` per base (half substitutions), N at n_frac."""
    out = []
    for c in s:
        x = rng.random()
        if x < rate / 2:
            out.append(rng.choice([b for b in "ACGT" if b != c]))
        elif x < rate * 3 / 4:
            pass                                    # deletion
        elif x < rate:
            out.append(c + rng.choice("ACGT"))      # insertion
        else:
            out.append(c)
        if n_frac and rng.random() < n_frac:
            out[-1] = "N"
    return "".join(out)


@functools.lru_cache(maxsize=None)
def extension_pairs():
    """About 200 seeded pairs: lengths 1 .. 600 (short ones more often: the first rows and the
    band cap), target a copy mutated 0-8 %, some with N, h0 in {28, 60}."""
    rng = random.Random(20240611)
    pairs = []
    for k in range(200):
        n = rng.randint(1, 40) if k % 4 == 0 else (rng.randint(1, 600) if k % 4 == 1 else rng.randint(40, 250))
        q = rand_seq(rng, n)
        t = mutate(rng, q, rng.choice([0.0, 0.01, 0.02, 0.04, 0.08]), 0.01 if k % 5 == 0 else 0.0)
        if k % 7 == 0:                              # a target that runs past / stops short of the query
            t = t + rand_seq(rng, rng.randint(1, 30)) if k % 2 else t[:max(1, len(t) - rng.randint(1, 30))]
        if not t:
            t = "A"
        pairs.append((q, t, 28 if k % 2 else 60))
    return pairs


@functools.lru_cache(maxsize=None)
def extension_ref():
    """extend() for every pair under both parameter sets (computed once per process)."""
    out = {}
    for name, prm in (("pass1", PASS1), ("pass2", PASS2)):
        al = {k: prm[k] for k in ("a", "b", "o", "e", "w", "zdrop")}
        out[name] = [extend(nt4(q), nt4(t), h0, **al) for q, t, h0 in extension_pairs()]
    return out


@functools.lru_cache(maxsize=None)
def known():
    """The known-answer reads: X random (400), J a 40-base joint with J[0] != comp(J[-1])."""
    rng = random.Random(424242)
    X = rand_seq(rng, 400)
    J = rand_seq(rng, 40)
    while J[0] == rc(J[-1]):
        J = rand_seq(rng, 40)
    pal70 = rand_seq(rng, 70)
    return {
        "X": X, "J": J,
        "joined": X + rc(X),
        "split": X + J + rc(X),
        "short_tail": X + J + rc(X)[:150],
        "short_head": X[-150:] + J + rc(X),
        "random": rand_seq(rng, 1000),
        "stubby": pal70 + rc(pal70),
    }


@functools.lru_cache(maxsize=None)
def seed_edge_reads():
    """Per length in SEED_EDGE_LENGTHS: a random read, X + rc(X), the same with N at the centre;
    and (AT)x100 + 50 random bases."""
    rng = random.Random(777)
    reads = []
    for L in SEED_EDGE_LENGTHS:
        reads.append(rand_seq(rng, L))
        x = rand_seq(rng, L // 2)
        pal = x + ("A" if L % 2 else "") + rc(x)
        reads.append(pal)
        c = len(pal) // 2
        reads.append(pal[:c] + "N" + pal[c + 1:])
    reads.append("AT" * 100 + rand_seq(rng, 50))
    return reads


@functools.lru_cache(maxsize=None)
def multi_arm_reads():
    """Reads with more than 2 alignments after the filter: `resolved` (A J rc(A) J A with short
    joints: pass 2 bridges them and the read is trimmed) and `inconclusive` (four arms, joints
    of 200: pass 2 returns the same four alignments)."""
    rng = random.Random(78)
    A = rand_seq(rng, 300)
    J = [rand_seq(rng, 200) for _ in range(3)]
    rng2 = random.Random(77)
    B = rand_seq(rng2, 300)
    return {"resolved": B + rand_seq(rng2, 30) + rc(B) + rand_seq(rng2, 35) + B,
            "inconclusive": A + J[0] + rc(A) + J[1] + A + J[2] + rc(A)}


def plant(rng, read: str, kind: int) -> str:
    """A siamaera made of `read`: 0 joined (R + rc(R)), 1 split by a joint, 2 split with a
    short second arm, 3 split with mutated second arm (1 %)."""
    j = rand_seq(rng, rng.randint(20, 60))
    if kind == 0:
        return read + rc(read)
    if kind == 1:
        return read + j + rc(read)
    if kind == 2:
        return read + j + rc(read)[:max(60, len(read) // 3)]
    return read + j + rc(mutate(rng, read, 0.01))


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """64 seeded reads of 150 .. 3000 bases (most of them short: the Python reference pays per
    base), every third one a planted siamaera."""
    rng = random.Random(9001)
    reads = []
    for k in range(64):
        n = rng.randint(1500, 3000) if k % 8 == 0 else rng.randint(150, 600)
        if k % 3 == 0:
            r = plant(rng, rand_seq(rng, max(75, n // 2 - 20)), (k // 3) % 4)[:3000]
        else:
            r = rand_seq(rng, n)
        reads.append(r)
    return reads


@functools.lru_cache(maxsize=None)
def mixed_ref():
    """hsps() of the mixed batch under pass 1 (computed once per process)."""
    return [hsps(nt4(r), PASS1, 97.5) for r in mixed_batch()]

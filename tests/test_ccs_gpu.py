"""ccs-1 on the device equals the host path: status, alignments and consensus bytes of every
group, at both bands, at each capacity and just beyond it."""
import random

import pytest

import ccs_ref
from proovread_amd import _abi, ccseq

pytestmark = pytest.mark.gpu


def _group(recs):
    ids = [r[0] for r in recs]
    role, _, ng = ccseq.group(ids, [len(r[1]) for r in recs])
    assert ng == 1
    return [r[1].encode() for r in recs], [r[2].encode() for r in recs], list(role).index(ccseq.PRIMARY)


def _zmws(seed, n, lo=200, hi=700, passes=(2, 8)):
    rng = random.Random(seed)
    return [_group(ccs_ref.sim_zmw(rng, "m150101_1_s1_p0", z, rng.randrange(lo, hi + 1), rng.randrange(passes[0], passes[1] + 1))[1])
            for z in range(n)]


@pytest.fixture(scope="module")
def ctx():
    return _abi.default_context()


def _same(groups, p, ctx):
    host = ccseq.run_groups(groups, p, device=False, threads=8)
    dev = ccseq.run_groups(groups, p, device=True, ctx=ctx)
    for g, (hr, ha, dr, da) in enumerate(zip(host[0], host[1], dev[0], dev[1])):
        assert ha == da, f"group {g}: alignments"
        assert hr == dr, f"group {g}: status / consensus"
    return host, dev


@pytest.mark.parametrize("w", [8, 300])
def test_device_equals_host(ctx, w):
    groups = _zmws(11 + w, 12)
    host, dev = _same(groups, ccseq.default_params(w=w), ctx)
    assert sum(a is not None for ga in host[1] for a in ga) >= 20
    assert any(a is not None and a[0] == 1 for ga in host[1] for a in ga)
    assert all(r[0] == 0 and len(r[1]) > 100 for r in host[0])
    assert dev[2] > 0.0


def test_hooks_on_the_device(ctx):
    groups = _zmws(5, 4, 200, 300)
    p = ccseq.default_params(w=8)
    alns = ccseq.map_groups(groups, p, device=True, ctx=ctx)
    assert alns == ccseq.map_groups(groups, p, device=False)
    assert ccseq.consensus_groups(groups, alns, p, device=True, ctx=ctx) == ccseq.consensus_groups(groups, alns, p, device=False)


def _exact_len(rng, n, passes):
    """A group whose subreads all have exactly n bases."""
    insert = "".join(rng.choice("ACGT") for _ in range(n + n // 4 + 200))
    recs, at = [], 0
    for k in range(passes):
        s = ccs_ref.noisy(rng, insert if k % 2 == 0 else ccs_ref.revcomp(insert), 0.02, 0.01, 0.005)
        s = s[:n] if k % 2 == 0 else s[-n:]
        assert len(s) == n
        recs.append((f"m2/{n}/{at}_{at + n}", s, "".join(chr(33 + rng.randint(5, 20)) for _ in s)))
        at += n + 40
    return _group(recs)


def test_capacities_and_the_calls_after(ctx):
    rng = random.Random(3)
    p = ccseq.default_params(w=8)
    small = _zmws(21, 3, 200, 300, (3, 4))
    at_len, over_len = _exact_len(rng, ccseq.MAX_LEN, 2), _exact_len(rng, ccseq.MAX_LEN + 1, 2)
    at_n, over_n = _exact_len(rng, 80, ccseq.MAX_SUBREADS), _exact_len(rng, 80, ccseq.MAX_SUBREADS + 1)
    groups = [small[0], at_len, over_len, small[1], at_n, over_n, small[2]]
    host, dev = _same(groups, p, ctx)
    assert [r[0] for r in dev[0]] == [0, 0, ccseq.TOO_LONG, 0, 0, ccseq.TOO_MANY, 0]
    assert dev[0][2][1] == b"" and dev[0][5][1] == b"" and all(a is None for a in dev[1][2] + dev[1][5])
    assert dev[1][1][0] is not None and len(dev[0][1][1]) > ccseq.MAX_LEN // 2
    assert sum(a is not None for a in dev[1][4]) == ccseq.MAX_SUBREADS - 1
    _same(small, p, ctx)   # the next call on the context

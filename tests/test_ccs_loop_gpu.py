"""The task ccs-1 in the correction loop (modes sr / mr): correct.run(mode="sr") equals ccseq on
the read-long output followed by the sr-noccs tasks on ccseq's reads and their masked copy; one
id that is no PacBio subread id makes the run the plain sr-noccs run (bin/proovread:1512-1517)."""
import random

import numpy as np
import pytest

import ccs_ref
from proovread_amd import _abi, ccseq, correct, mask, tasks as T

pytestmark = pytest.mark.gpu

CFG = dict(coverage=30.0, seed_threads=2)


@pytest.fixture(scope="module")
def inputs():
    """Six ZMWs of 3-6 passes and two single subreads (qualities 20-35, so that the consensus has
    regions the hcr mask covers), 100 bp short reads off the inserts."""
    rng = random.Random(17)
    lrs, inserts = [], []
    for z in range(8):
        insert, recs = ccs_ref.sim_zmw(rng, "m150101_1_s1_p0", 10 + z, rng.randrange(500, 700), 1 if z in (2, 6) else rng.randrange(3, 7),
                                       partial=z % 2 == 0, qual_range=(20, 35))
        inserts.append(insert)
        lrs += [(i, s.encode(), q.encode()) for i, s, q in recs]
    sr = []
    for k in range(1400):
        ins = inserts[k % 8]
        at = rng.randrange(0, len(ins) - 100)
        s = ins[at:at + 100]
        sr.append(b"@sr%d\n%s\n+\n%s\n" % (k, (ccs_ref.revcomp(s) if rng.random() < 0.5 else s).encode(), b"I" * 100))
    return lrs, b"".join(sr)


def _same_reads(a: correct.LongReads, b: correct.LongReads):
    assert a.ids == b.ids
    assert a.seqs == b.seqs and a.quals == b.quals


def test_mode_sr_equals_ccseq_then_sr_noccs(inputs, tmp_path):
    lrs, srd = inputs
    pre = str(tmp_path / "PRE")
    res = correct.run(lrs, srd, correct.LoopConfig(mode="sr", keep_temporary=pre, **CFG))
    tasks = [e.task for e in res.log]
    assert tasks[:3] == ["read-long", "ccs-1", "bwa-sr-1"] and tasks[-1] == "bwa-sr-finish"
    # step 1: ccseq on the read-long output
    reads, _ = correct.read_long(lrs, 200)
    out, stats = ccseq.ccs_records([(i, "", s, q) for i, s, q in zip(reads.ids, reads.seqs, reads.quals)])
    assert (stats["primary"], stats["single"]) == (6, 2) and stats["flagged"] == 0
    assert res.log[1].counters == {k: stats[k] for k in ("single", "primary", "secondary", "flagged")}
    assert len(res.reads.ids) == 8
    with open(pre + ".ccs-1.fq", "rb") as f:
        assert f.read() == b"".join(b"@" + (r[0] + (" " + r[1] if r[1] else "")).encode() + b"\n" + r[2] + b"\n+\n" + r[3] + b"\n" for r in out)
    # step 2: the sr-noccs tasks on ccseq's reads and their masked reference
    ccs = correct.LongReads([r[0] for r in out], [bytes(r[2]) for r in out], [bytes(r[3]) for r in out])
    masked, _, _ = mask.run(ccs.seqs, ccs.quals, mask.params(T.hcr_mask("ccs-1"), 100))
    assert any(m != s for m, s in zip(masked, ccs.seqs))
    stages = correct.GpuStages()
    stages.load(ccs)
    stages.set_map(masked)
    srs = correct.ShortReads(srd)
    stages.load_short_reads(srs)
    chim, _, log = correct.run_tasks(stages, srs, list(T.MODE_TASKS["sr-noccs"][1:]), correct.LoopConfig(**CFG), "sr-noccs", 100, True)
    assert [e.task for e in log] == tasks[2:]
    assert [(e.bpt, e.bpn, e.n_tasks) for e in log] == [(e.bpt, e.bpn, e.n_tasks) for e in res.log[2:]]
    _same_reads(stages.reads(), res.reads)
    assert chim == res.chim
    # and the subreads were collapsed: one read per ZMW, the primaries' ids
    assert res.reads.ids == [r[0] for r in out]


def test_a_foreign_id_falls_back_to_noccs(inputs):
    lrs, srd = inputs
    lrs = list(lrs)
    lrs[3] = ("contig_17", lrs[3][1], lrs[3][2])
    got = correct.run(lrs, srd, correct.LoopConfig(mode="sr", **CFG))
    want = correct.run(lrs, srd, correct.LoopConfig(mode="sr-noccs", **CFG))
    assert [e.task for e in got.log] == [e.task for e in want.log] and "ccs-1" not in [e.task for e in got.log]
    _same_reads(got.reads, want.reads)
    assert got.chim == want.chim and len(got.reads.ids) == len(correct.read_long(lrs, 200)[0].ids)

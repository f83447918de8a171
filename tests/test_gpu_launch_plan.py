"""k_small's launch geometry (bsdc_run: one dispatch per non-empty size class over the side streams,
four families a workgroup) changes no output byte whatever the classes' sizes: batches shaped to the
edges of that geometry, consensus bases, quals, lengths and status against oracle/ as
tests/test_gpu_parity.py compares them.

The shapes are made by moving families of a small synthetic batch into wider size classes (a wider
arena holds a narrower family).  No launch plan was built (profiles/occupancy/README.md: none
paid), so there is no plan function to test on the CPU; these are the batch shapes such a plan
would have met, kept as parity tests of the geometry there is.
"""
import numpy as np
import pytest

from bsseqconsensusreads_amd import _lib, pipeline, synth
from bsseqconsensusreads_amd.batch import materialize, plan_families
from bsseqconsensusreads_amd.pipeline import MODE_CONVERT, MODE_EXTEND, MODE_TAGS, MODE_VOTE
from oracle import oracle
from test_gpu_parity import assert_consensus_equal

pytestmark = pytest.mark.gpu

NQ = _lib.SMALL_BUCKETS
WG = 4  # families a k_small workgroup
_cache = {}


def dataset(cfg, n):
    """-> (synthetic set, its families planned, oracle/'s consensus): made once per shape."""
    if (cfg, n) not in _cache:
        s = synth.generate(cfg, n, seed=47, device="cpu", genome_len=200_000)
        plan = plan_families(s.raw, "full", s.ref)
        assert not plan.split_ext
        _cache[cfg, n] = (s, plan, oracle.run(s.raw, s.ref))
    return _cache[cfg, n]


def reshape_classes(fb, want):
    """Move the batch's small families into classes of `want` families each (None: the rest): the
    narrowest families to the narrowest classes, none into a class below its own."""
    own = np.concatenate([np.full(b.shape[0], q) for q, b in enumerate(fb.small_buckets)])
    fams = fb.small_fams
    rest = fams.shape[0] - sum(w for w in want if w is not None)
    want = [rest if w is None else w for w in want]
    assert rest >= 0 and sum(want) == fams.shape[0] and len(want) == NQ
    out, at = [], 0
    for q, w in enumerate(want):
        assert w == 0 or own[at:at + w].max() <= q, "class %d cannot hold these families" % q
        out.append(fams[at:at + w].astype(np.uint32))
        at += w
    fb.small_buckets = out
    return fb


def sizes(fb):
    return np.array([b.shape[0] for b in fb.small_buckets], np.int64)


def run(engine, s, fb, tags=False, times=1):
    engine.load_reference(s.ref)
    db = engine.upload(fb, tags=tags)
    out = []
    for _ in range(times):
        engine.run(db, MODE_CONVERT | MODE_EXTEND | MODE_VOTE | (MODE_TAGS if tags else 0))
        out.append(pipeline.consensus_from_output(fb, db.fetch(ss=tags)))
    return out[0] if times == 1 else out


def test_one_class(engine):
    s, plan, ref = dataset("C0", 300)
    fb = materialize(plan, 0, plan.n_fam)
    assert (sizes(fb) > 0).sum() == 1
    assert_consensus_equal(run(engine, s, fb), ref, "one class")


def test_two_unequal_classes(engine):
    s, plan, ref = dataset("C2", 300)
    fb = reshape_classes(materialize(plan, 0, plan.n_fam), [0, 0, 0, 0, 0, None, 5, 0])
    n = sizes(fb)
    assert (n > 0).sum() == 2 and n[5] > 50 * n[6] > 0
    assert_consensus_equal(run(engine, s, fb), ref, "two classes")


def test_seven_classes_one_dominant(engine):
    """Every class non-empty, more than 80% of the families in one whose size is no multiple of
    the workgroup's four (a ragged last workgroup), as are the small classes'."""
    s, plan, ref = dataset("C2", 300)
    fb = reshape_classes(materialize(plan, 0, plan.n_fam), [6, 6, 6, 6, None, 6, 7, 0])
    n = sizes(fb)
    assert (n > 0).sum() == 7 and n[4] > 0.8 * n.sum() and n[4] % WG != 0
    assert_consensus_equal(run(engine, s, fb, tags=True), ref, "dominant class")


def test_6144_class_holds_most_families(engine):
    """The class whose workgroups went from 8 wavefronts to 4: most of the batch in it, many
    workgroups and a ragged last one."""
    s, plan, ref = dataset("C2", 300)
    fb = materialize(plan, 0, plan.n_fam)
    wider = int(sizes(fb)[4:].sum())  # (families that need more than 6144 B: to the 12288-B class)
    assert sizes(fb)[6:].sum() == 0
    fb = reshape_classes(fb, [6, 6, 6, None, 0, wider, 0, 0])
    n = sizes(fb)
    assert fb.small_arenas[3] == 6144 and n[3] > 0.8 * n.sum() and n[3] > 50 * WG and n[3] % WG != 0
    assert_consensus_equal(run(engine, s, fb, tags=True), ref, "6144-B class")


def test_widest_class_shorter_than_a_workgroup(engine):
    """3 families of the widest class (one workgroup, its fourth wavefront without a family) beside
    2 narrow ones."""
    s, _, _ = dataset("C2", 300)
    raw = synth.subset_families(s.raw, 5)
    plan = plan_families(raw, "full", s.ref)
    fb = materialize(plan, 0, plan.n_fam)
    fb = reshape_classes(fb, [0, 0, 0, 0, fb.small_fams.shape[0] - 3, 0, 0, 3])
    assert sizes(fb)[7] == 3 < WG
    assert_consensus_equal(run(engine, s, fb), oracle.run(raw, s.ref), "short widest class")


def test_with_large_and_split_families(engine):
    """C4's shape: every small class beside k_large's classes and the split families' parts and
    join, all forked over the side streams and joined."""
    s, plan, ref = dataset("C4", 300)
    fb = materialize(plan, 0, plan.n_fam)
    assert (sizes(fb) > 0).sum() > 4 and sum(b.shape[0] for b in fb.large_buckets) > 0 and fb.split_fams.shape[0] > 0
    assert_consensus_equal(run(engine, s, fb, tags=True), ref, "C4")


def test_same_batch_twice(engine):
    s, plan, ref = dataset("C2", 300)
    fb = reshape_classes(materialize(plan, 0, plan.n_fam), [6, 6, 6, 6, None, 6, 7, 0])
    a, b = run(engine, s, fb, times=2)
    for k in ("status", "length", "seq", "qual"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert_consensus_equal(b, ref, "second run")

"""The consensus kernels on what a record's alignment decides, on inputs built for it
(tests/align_inputs.py; the CPU side of every case, with the hand-derived trims, survivors and
overlap values, is checked in tests/test_align_inputs.py): indels, N ops, = / X and clips at every
place in a read, the overlap consensus across indels (with a quality byte >= 128 in the family,
and switched off), the read-through trim with its boundary inside and beside indels and with
stale mate fields, source reads emptied by the trims, the most-common-alignment filter with ties,
prefixes and truncated cigars, near-tie columns in a set the filter has reordered, and a family
whose largest alignment group is the 71st defined, and the largest family the filter's 16-bit
slot offsets admit.

Every case: GPU == oracle/ bit for bit (consensus, single-strand reads and tag statistics, and
the tool-2 records where the tools run), then the fp64 bar (helpers.gpu_vs_fp64).  Routes as in
test_gpu_edges.py: the default routing (k_small takes the small families), every family through
k_large with its arena in LDS and in HBM, and part mode with a small cap, where a family holding
a complex cigar must stay whole.
"""
import numpy as np
import pytest

import align_inputs as A
from bsseqconsensusreads_amd import batch
from helpers import gpu_vs_fp64
from test_gpu_edges import KERNELS, check, route

pytestmark = pytest.mark.gpu


def run_case(engine, c, what, **kw):
    """The case with the tools and the dump (test_gpu_edges.check) or the caller alone."""
    if c.run_tools:
        return check(engine, c, what, **kw)
    cons, cnt, _, r = gpu_vs_fp64(engine, c.raw, c.ref, False, what, **kw)
    assert 2 * int(r.status.sum()) >= len(r.status) > 0
    return cons, cnt, r


def assert_routed(seen, how):
    """default: k_small took every family of 64 records or fewer that holds a complex cigar;
    lds / global: k_large took them all; parts: no family with a complex cigar was cut."""
    assert len(seen) >= 1
    n_cx = 0
    for fb in seen:
        fam_of = np.repeat(np.arange(fb.n_fam), np.diff(fb.fam_off.astype(np.int64)))
        cx = np.zeros(fb.n_fam, bool)
        cx[fam_of[(fb.rec_link & batch.LINK_COMPLEX) != 0]] = True
        cx = np.nonzero(cx)[0]
        n_cx += cx.shape[0]
        sizes = np.diff(fb.fam_off.astype(np.int64))
        small = np.concatenate(fb.small_buckets).astype(np.int64)
        large = np.concatenate([b[:, 0] for b in fb.large_buckets]).astype(np.int64)
        if how == "default":
            assert np.isin(cx[sizes[cx] <= 64], small).all() and np.isin(cx[sizes[cx] > 64], large).all()
        else:
            assert small.shape[0] == 0 and np.isin(cx, large).all()
        if how == "parts":
            assert not np.isin(cx, fb.split_fams[:, 0].astype(np.int64)).any()
    assert n_cx > 0


@pytest.mark.parametrize("how", KERNELS + ["parts"])
@pytest.mark.parametrize("name", list(A.CASES))
def test_alignment_edges(engine, monkeypatch, name, how):
    c = A.case(name)
    seen = route(monkeypatch, how, cap=2800)
    run_case(engine, c, "%s %s" % (name, how))
    assert_routed(seen, how)


@pytest.mark.parametrize("how", KERNELS)
@pytest.mark.parametrize("name", ["overlap", "overlap_wild", "shapes"])
def test_alignment_edges_overlap_off(engine, monkeypatch, name, how):
    c = A.case(name)
    seen = route(monkeypatch, how)
    run_case(engine, c, "%s overlap off %s" % (name, how), overlap=False)
    assert_routed(seen, how)


@pytest.mark.parametrize("how", ["default", "global"])
def test_largest_filter_slot_family(engine, monkeypatch, how):
    """The largest family BSDC_MAX_FILTER_SLOTS admits with these cigars: 3,276 templates, 19
    slots per forward record and 1 per reverse one, 65,520 slots -- k_large's slot offsets run up
    to 65,519, past 32,767 and beside the 16-bit edge (tests/test_host_plan.py refuses one template
    more).  One group on each side, so the filter rejects nothing and every read votes."""
    c = A.slot_family(3276)
    seen = route(monkeypatch, how)
    cons, cnt, r = run_case(engine, c, "slots %s" % how)
    assert_routed(seen, how)
    fb = seen[0]
    cx = (fb.rec_link & batch.LINK_COMPLEX) != 0
    assert int((fb.cig_info[cx] & 0xFFFF).sum()) + 2 * int(cx.sum()) + int((~cx).sum()) == 65520 <= batch.MAX_FILTER_SLOTS
    assert r.sources["count"].tolist() == [[3276, 3276, 0, 0]] and int(cons.status[0] & 1) == 1

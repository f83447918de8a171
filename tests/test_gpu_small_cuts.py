"""k_small at the edges its vote epilogue, queue, convert and overlap phases branch on: absent
sides (the epilogue skips a side no read of the family belongs to), consensus lengths beside the
lane (4 columns) and pass (256 columns) edges, slow columns of every best base with one to three
competing bases and more than one queue round, every count of converted records around the
4-record rounds, overlaps of 1 to 65 positions at each byte alignment, and quality bytes >= 128.

Every case: <= 300 families built with tests/edge_inputs.py, run through k_small alone (asserted
on the device batch), bases, quals, lengths and status bit-exact against oracle.run, without and
with the consensus tags (the TAGS instance; assert_ss_equal's columns).  What each case must
contain is asserted on the input or on the oracle's result, never on the GPU's.
"""
import numpy as np
import pytest

import edge_inputs as E
from bsseqconsensusreads_amd import batch, pipeline
from bsseqconsensusreads_amd import records as R
from oracle import oracle
from test_gpu_parity import assert_consensus_equal, assert_ss_equal

_cache = {}


def _place(fams, glen, seed):
    rng = np.random.default_rng(seed)
    for f in fams:
        f.start = int(rng.integers(0, glen - f.frag + 1))
    fams[0].start = 0
    fams[-1].start = glen - fams[-1].frag
    return fams


def _fam(n_ab, n_ba, lens, frag, ab_top=True, unpaired=None):
    return E.Family(n_ab, n_ba, list(lens), 0, int(frag), ab_top=ab_top, unpaired_r1=unpaired)


# ---- the cases' inputs (built once; the tests leave them unchanged) --------------------------------
def absent_sides():
    """AB-only, BA-only and two-strand families, then families cut down to the records of one set
    (AB-R1, AB-R2, BA-R1, BA-R2 alone: not emitted) and to one strand's R1s plus the other's R2s."""
    rng = np.random.default_rng(21)
    fams = []
    for k in range(120):
        nt = int(rng.integers(1, 5))
        na = (nt, 0, int(rng.integers(0, nt + 1)))[k % 3]
        L = int(rng.integers(30, 60))
        fams.append(_fam(na, nt - na, [(L, L - int(rng.integers(0, 5)))] * nt, L + int(rng.integers(0, 20)),
                         ab_top=bool(k & 1)))
    for k in range(48):  # one AB and one BA template each; records dropped below
        fams.append(_fam(1, 1, [(40, 38)] * 2, 50, ab_top=bool(k & 1)))
    es = E.build(_place(fams, 4000, 22), E.q_bins, seed=23, contig_len=4000, extra_error=0.05)
    raw = es.raw
    r1 = (raw.flag & 0x40) != 0
    ab = raw.mi_strand == 0
    keep = np.ones(raw.n, bool)
    for k in range(48):
        m = raw.mi_id == 120 + k
        want = k % 6  # 0..3: that set alone; 4: AB-R1 + BA-R1 (both ends' pairs broken); 5: AB-R1 + BA-R2
        sel = [ab & r1, ab & ~r1, ~ab & r1, ~ab & ~r1, r1, (ab & r1) | (~ab & ~r1)][want]
        keep[m & ~sel] = False
    return E.EdgeSet(R.take(raw, np.nonzero(keep)[0]), es.ref, es.families)


LENGTHS = (1, 3, 4, 5, 8, 9, 127, 128, 129, 252, 253, 254, 255, 256, 257)


def length_edges():
    """Per family one R1 length and one R2 length, both from LENGTHS and its neighbours and never
    the same: the consensus lengths land on every lane and pass edge, and the two ends' passes
    differ (one end's second 256-column pass, or its lanes past the first, stay empty)."""
    rng = np.random.default_rng(31)
    pool = sorted(set(l + d for l in LENGTHS for d in (-2, -1, 0) if 1 <= l + d <= 257))
    fams = []
    for k, l1 in enumerate(pool * 4):
        l2 = int(rng.choice([l for l in pool if l != l1]))
        if k & 1:
            l1, l2 = l2, l1
        nt = int(rng.integers(1, 4))
        na = int(rng.integers(0, nt + 1)) if k % 5 else nt
        fams.append(_fam(na, nt - na, [(l1, l2)] * nt, max(l1, l2) + int(rng.integers(0, 4)), ab_top=bool(rng.random() < 0.5)))
    return E.build(_place(fams, 3000, 32), E.q_bins, seed=33, contig_len=3000, extra_error=0.02)


def slow_columns():
    """3 to 8 reads per set at 25 % wrong bases whatever the quality: disagreeing columns with one,
    two and three competing bases, equal-quality ties, and families with far more than 32 queued
    columns (two queue rounds and more)."""
    rng = np.random.default_rng(41)
    fams = []
    for k in range(150):
        na, nb = int(rng.integers(3, 9)), int(rng.integers(0, 9))
        L = int(rng.integers(40, 70))
        fams.append(_fam(na, nb, [(L, L)] * (na + nb), L + int(rng.integers(0, 10)), ab_top=bool(k & 1)))
    return E.build(_place(fams, 4000, 42), E.q_bins, seed=43, contig_len=4000, extra_error=0.25)


NCONV = (0, 1, 2, 3, 4, 5, 8, 9)
CONV_LENGTHS = (1, 3, 4, 5, 63, 64, 65)


def converted_records():
    """nconv converted records (the bottom strand's, flags 83 / 163: AB with ab_top off, its
    unpaired R1 making the count odd) of lengths CONV_LENGTHS, equal or mixed inside the family,
    beside 0 to 2 top-strand templates."""
    rng = np.random.default_rng(51)
    fams = []
    for rep in range(5):
        for nc in NCONV:
            for L in CONV_LENGTHS + ("mixed",):
                nb = nc // 2  # bottom templates
                nt = int(rng.integers(0, 3)) if nc else int(rng.integers(1, 4))
                pick = (lambda: int(rng.choice(CONV_LENGTHS))) if L == "mixed" else (lambda: L)
                lens = [(pick(), pick()) for _ in range(nb + nt)]
                un = pick() if nc & 1 else None
                frag = max([max(p) for p in lens] + [un or 1]) + int(rng.integers(0, 3))
                fams.append(_fam(nb, nt, lens, frag, ab_top=False, unpaired=un))
    fams = [fams[int(i)] for i in rng.permutation(len(fams))][:250]
    return E.build(_place(fams, 3000, 52), E.q_full_range, seed=53, contig_len=3000, extra_error=0.02)


OVERLAPS = (1, 3, 4, 5, 64, 65)


def overlaps():
    """Mates overlapping by exactly OVERLAPS positions, the overlap starting at each of the four
    byte alignments inside R1 (four consecutive R1 lengths), on both strands."""
    fams = []
    for ov in OVERLAPS:
        for l1 in (70, 71, 72, 73):
            for top in (True, False):
                for nt in (1, 3):
                    fams.append(_fam(nt, 1, [(l1, 75)] * (nt + 1), l1 + 75 - ov, ab_top=top))
    return E.build(_place(fams, 4000, 62), E.q_full_range, seed=63, contig_len=4000, extra_error=0.1)


def wild_quals():
    """Every family: one record with quality bytes >= 128 (a few bytes, or all 0xFF)."""
    rng = np.random.default_rng(71)
    fams = []
    for k in range(100):
        nt = int(rng.integers(1, 5))
        na = int(rng.integers(0, nt + 1))
        L = int(rng.integers(20, 80))
        fams.append(_fam(na, nt - na, [(L, L)] * nt, L + int(rng.integers(0, 30)), ab_top=bool(k & 1)))
    es = E.build(_place(fams, 4000, 72), E.q_full_range, seed=73, contig_len=4000, extra_error=0.1)
    raw = es.raw
    qual = raw.qual.copy()
    off = np.concatenate([[0], np.cumsum(raw.l_seq.astype(np.int64))])
    for f in range(100):
        rec = int(rng.choice(np.nonzero(raw.mi_id == f)[0]))
        a, b = int(off[rec]), int(off[rec + 1])
        if f % 4 == 0:
            qual[a:b] = 0xFF
        else:
            hit = a + rng.choice(b - a, size=min(3, b - a), replace=False)
            qual[hit] = rng.integers(128, 255, size=hit.shape[0]).astype(np.uint8)
    import dataclasses
    return E.EdgeSet(dataclasses.replace(raw, qual=qual), es.ref, es.families)


CASES = {"absent": absent_sides, "lengths": length_edges, "slow": slow_columns, "nconv": converted_records,
         "overlaps": overlaps, "wild": wild_quals}


def case(name):
    """-> (EdgeSet, oracle result), built and computed once per session."""
    if name not in _cache:
        es = CASES[name]()
        _cache[name] = (es, oracle.run(es.raw, es.ref, keep_sources=name == "slow"))
    return _cache[name]


# ---- what each case must contain: on the input and the oracle's result ------------------------------
def _slow_cols(r):
    """From the source reads each set's vote saw (oracle keep_sources; column j of a read is its
    byte j), per column of every emitted family's sets where more than one of A/C/G/T shows:
    (called base, distinct A/C/G/T bases, near tie), and the count of such columns per family.
    Near tie as the kernels define it: the two best of the four sums of
    oracle.tables()' lr[q] are at most one unit per read of the set apart."""
    lr = oracle.tables()[0]
    src = r.sources
    F = len(r.status)
    first = np.concatenate([[0], np.cumsum(src["count"].ravel())])  # reads before (family, set)
    off = np.concatenate([[0], np.cumsum(src["len"].astype(np.int64))])
    called, distinct, tie, per_fam = [], [], [], np.zeros(F, np.int64)
    for f in np.nonzero(r.status == 1)[0]:
        for s_ in range(4):
            n, L = int(src["count"][f, s_]), int(r.ss["len"][f, s_])
            if n == 0:
                continue
            D = np.zeros((4, L), np.int64)
            depth = np.zeros(L, np.int64)
            for k in range(int(first[4 * f + s_]), int(first[4 * f + s_]) + n):
                b = src["base"][off[k]:off[k + 1]][:L]
                q = src["qual"][off[k]:off[k + 1]][:L]
                for i, code in enumerate((E.A, E.C, E.G, E.T)):
                    D[i, :b.shape[0]] += np.where(b == code, lr[q], 0)
                    depth[:b.shape[0]] += b == code
            assert np.array_equal(depth, r.ss["depth"][f, s_, :L])  # (the columns are the vote's)
            nd = (D != 0).sum(axis=0)
            top = np.sort(D, axis=0)
            cols = nd > 1
            called.append(r.ss["base"][f, s_, :L][cols])
            distinct.append(nd[cols])
            tie.append((top[3] - top[2] <= n)[cols])
            per_fam[f] += int(cols.sum())
    return np.concatenate(called), np.concatenate(distinct), np.concatenate(tie), per_fam


def assert_case(name, es, r):
    raw = es.raw
    F = len(r.status)
    assert 0 < F <= 300
    sl = r.ss["len"] > 0  # [F, 4]: AB-R1, AB-R2, BA-R1, BA-R2
    if name == "absent":
        pat = set(map(tuple, sl.tolist()))
        for want in ((1, 1, 0, 0), (0, 0, 1, 1), (1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1),
                     (1, 0, 1, 0), (1, 0, 0, 1)):
            assert tuple(bool(x) for x in want) in pat, want
        assert int((r.status == 0).sum()) >= 32 and int((r.status == 1).sum()) >= 100
        one = sl.sum(axis=1) == 1
        assert (r.status[one] == 0).all()
        # AB-R1 + BA-R1: end 0 has side A alone, end 1 side B alone, and the pair is emitted;
        # AB-R1 + BA-R2 are both sides of end 0 with no end 1: not emitted
        assert (r.status[(sl == (True, False, True, False)).all(axis=1)] == 1).any()
        assert (r.status[(sl == (True, False, False, True)).all(axis=1)] == 0).all()
    elif name == "lengths":
        em = r.status == 1
        got = set(r.cons_len[em].ravel().tolist())
        assert set(LENGTHS) <= got, sorted(set(LENGTHS) - got)
        assert all(f.lens[0][0] != f.lens[0][1] for f in es.families)
        # (tool 1's prepended and tool 2's added bases can level a pair one base apart)
        assert float((r.cons_len[em][:, 0] != r.cons_len[em][:, 1]).mean()) > 0.8
        assert int((np.abs(r.cons_len[em][:, 0] - r.cons_len[em][:, 1]) > 128).sum()) > 10
        assert int(raw.l_seq.max()) == 257
    elif name == "slow":
        called, distinct, tie, per_fam = _slow_cols(r)
        for b in (E.A, E.C, E.G, E.T):
            for k in (1, 2, 3):  # the called base against k other bases in the column
                assert int(((called == b) & (distinct == k + 1)).sum()) > 0, (b, k)
            assert int(((called == b) & tie).sum()) > 0, b  # and through the near-tie pick
        assert int(tie.sum()) > 50
        assert int(per_fam.max()) > 64 and int((per_fam > 32).sum()) > 20  # two queue rounds and more
    elif name == "nconv":
        conv = batch.tool1_plan(raw)[1]
        members = [r.fam_src[r.fam_rec_off[f]:r.fam_rec_off[f + 1]] for f in range(F)]  # (the oracle's families)
        nconv = np.array([int(conv[m].sum()) for m in members], np.int64)
        assert set(NCONV) <= set(nconv.tolist()) and int(nconv.max()) == 9
        assert set(CONV_LENGTHS) <= set(raw.l_seq[conv].tolist())
        mixed = [f for f in range(F) if nconv[f] >= 2 and len(set(raw.l_seq[members[f]][conv[members[f]]].tolist())) > 1]
        assert len(mixed) > 10
        # the RD trim on the first, a middle and the last converted record of a family
        t1 = r.tool1
        rd = np.zeros(raw.n, bool)
        rd[t1.src[t1.rd == 1]] = True
        where = set()
        for f in np.nonzero(nconv >= 3)[0]:
            idx = np.sort(members[f][conv[members[f]]])  # (record order = image order)
            hit = np.nonzero(rd[idx])[0]
            where |= {"first" if h == 0 else "last" if h == len(idx) - 1 else "middle" for h in hit.tolist()}
        assert where == {"first", "middle", "last"}, where
    elif name == "overlaps":
        seen = set()
        for f in es.families:
            l1, l2 = f.lens[0]
            seen.add((l1 + l2 - f.frag, l1 & 3))
        assert seen == {(ov, a) for ov in OVERLAPS for a in range(4)}
    elif name == "wild":
        assert E.family_has_wild(raw).all() and (raw.qual == 0xFF).any() and ((raw.qual >= 128) & (raw.qual < 0xFF)).any()
        assert int((r.status == 1).sum()) > 50


def test_inputs_hold_their_edges_on_the_oracle():
    """(no GPU: it runs with the CPU suite, so drift in the generated inputs shows there first; the
    GPU tests assert the same before they run)"""
    for name in CASES:
        es, r = case(name)
        assert_case(name, es, r)


@pytest.mark.gpu
@pytest.mark.parametrize("tags", [False, True], ids=["plain", "tags"])
@pytest.mark.parametrize("name", list(CASES))
def test_small_cuts(engine, monkeypatch, name, tags):
    es, r = case(name)
    assert_case(name, es, r)
    seen = []
    real = batch.materialize

    def spy(*a, **kw):
        fb = real(*a, **kw)
        seen.append(fb)
        return fb
    monkeypatch.setattr(batch, "materialize", spy)
    monkeypatch.setattr(pipeline, "materialize", spy)
    engine.load_reference(es.ref)
    cons, _ = pipeline.run_step5(engine, es.raw, tags=tags)
    # k_small alone
    assert seen and sum(int(b.shape[0]) for fb in seen for b in fb.small_buckets) == len(r.status)
    assert all(int(fb.large_fams.shape[0]) == 0 and int(fb.split_fams.shape[0]) == 0 for fb in seen)
    what = "%s %s" % (name, "tags" if tags else "plain")
    assert_consensus_equal(cons, r, what)
    assert np.array_equal(cons.status & 1, r.status.astype(cons.status.dtype)), what
    if tags:
        assert_ss_equal(cons, r, what)

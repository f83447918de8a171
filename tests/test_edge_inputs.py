"""The edge-input builder (tests/edge_inputs.py) on the CPU: every case the GPU edge tests
(tests/test_gpu_edges.py) run really holds its edge, the restatement emits most of its families
(a comparison against it is never vacuous), and the restatement's own vote meets the fp64 bar of
tests/test_fgbio_vote.py on it -- at every quality sampler and every accepted error-rate pair.
Seeds are the builders' defaults, chosen so that oracle/ alone meets all of this.
"""
import numpy as np
import pytest

import edge_inputs as E
from bsseqconsensusreads_amd import batch
from oracle import oracle
from test_fgbio_vote import assert_fp64_bar, fp64_check

CASES = [("quality", s) for s in ("full_range", "high", "wild")] + [("size", False), ("size", True)] + \
        [("length", n) for n in list(E.LENGTH_SETS) + ["mixed"]] + [("stride", a) for a in (15, 16, 17, 31, 32, 33)] + \
        [("params", None)]


def make(kind, arg):
    if kind == "params":
        return E.params_case()
    return {"quality": E.quality_case, "size": E.size_case, "length": E.length_case, "stride": E.stride_case}[kind](arg)


def live_ss(r):
    return np.arange(r.ss["qual"].shape[2])[None, None, :] < r.ss["len"][:, :, None]


def test_builder_is_deterministic_and_follows_the_pairing_model():
    a, b = E.quality_case("wild"), E.quality_case("wild")
    for k in ("flag", "pos", "l_seq", "seq", "qual", "next_pos", "tlen", "mi_id", "mi_strand", "name_id", "mc_cigar"):
        assert np.array_equal(getattr(a.raw, k), getattr(b.raw, k)), k
    assert np.array_equal(a.ref.packed, b.ref.packed)
    assert not np.array_equal(a.raw.seq, E.quality_case("wild", seed=4).raw.seq)
    raw = a.raw
    assert set(np.unique(raw.flag).tolist()) == {83, 99, 147, 163}
    fwd = (raw.flag & 16) == 0
    assert (raw.tlen[fwd] > 0).all() and (raw.tlen[~fwd] < 0).all()
    # mates point at each other: the forward read's PNEXT is its mate's POS and the reverse one's likewise
    by = {}
    for k in range(raw.n):
        by.setdefault((int(raw.mi_id[k]), int(raw.name_id[k])), []).append(k)
    for ks in by.values():
        assert len(ks) == 2
        x, y = ks
        assert raw.next_pos[x] == raw.pos[y] and raw.next_pos[y] == raw.pos[x] and raw.tlen[x] == -raw.tlen[y]
        assert raw.mc_cigar[raw.mc_off[x]] >> 4 == raw.l_seq[y] and {int(raw.flag[x]) & 0xC0, int(raw.flag[y]) & 0xC0} == {0x40, 0x80}
        assert raw.mi_strand[x] == raw.mi_strand[y]


@pytest.mark.parametrize("kind,arg", CASES)
def test_case_holds_its_edge(kind, arg):
    es = make(kind, arg)
    raw = es.raw
    glen = int(es.ref.contig_len[0])
    assert raw.n <= 8000
    assert (raw.pos == 0).any() and (raw.pos + raw.l_seq == glen).any()  # reads at both contig ends
    r, ss, c = fp64_check(raw, es.ref)
    assert_fp64_bar(c, "%s %s" % (kind, arg))
    assert c["qual_pm1"] == 0  # (45, 30): DESIGN.md 3.5's +-0 (qualities above 93 included, as it turns out)
    assert 2 * int(r.status.sum()) >= len(r.status) > 0
    if kind == "quality":
        E.assert_quality_edges(arg, raw)
        assert len(es.families) == 150 and raw.l_seq.min() == raw.l_seq.max() == 40
    elif kind == "size":
        sizes = np.diff(r.fam_rec_off)
        want = sorted(list(E.FAMILY_SIZES) * 3 + [E.DEEP_FAMILY])
        assert sorted(sizes.tolist()) == want
        assert (r.status[sizes == 1] == 0).all() and (r.status[sizes > 1] == 1).all()
        p = batch.plan_families(raw, "full", es.ref)
        assert sorted(np.diff(p.fam_off).tolist()) == want  # the planner's families are these too
        if arg:  # AB-only: the two AB sets hold n / 2 reads each, nothing on the BA side
            assert (raw.mi_strand == 0).all()
            cnt = oracle.run(raw, es.ref, keep_sources=True).sources["count"]
            assert (cnt[:, 2:] == 0).all()
            for n in (64, 65, 127, 128, 129):
                assert (cnt[:, 0] == n).any() or (cnt[:, 1] == n).any(), n
            f = int(np.nonzero(sizes == E.DEEP_FAMILY)[0][0])
            assert r.ss["depth"][f].max() > 255
            assert r.ss["depth"][sizes == 255].max() <= 128
    elif kind == "length":
        lens = set(raw.l_seq.tolist())
        if arg == "mixed":
            assert len(lens) > 50 and min(lens) == 1 and max(lens) == 66
            per_fam = [len(set(raw.l_seq[raw.mi_id == k].tolist())) for k in range(len(es.families))]
            assert np.mean(np.asarray(per_fam) > 1) > 0.9  # lengths vary inside the families
        else:
            assert lens == set(E.LENGTH_SETS[arg])
        if arg == "tiny":
            # converted 1-3 base records, among them ones whose RD trim drops the last base: of a
            # 1-base read only tool 1's prepended base is left
            t1 = r.tool1
            short = raw.l_seq[t1.src] <= 3
            trimmed = short & (t1.rd == 1)
            assert int(trimmed.sum()) >= 3
            assert int((trimmed & (raw.l_seq[t1.src] == 1) & (t1.l_seq == 1)).sum()) >= 1
            assert int(r.tool2.l_seq.min()) == 1
    elif kind == "stride":
        assert int(raw.l_seq.max()) + 2 == arg
        assert batch.build_family_batch(raw, "full", es.ref).stride == int(batch.round16(arg))
    elif kind == "params":
        assert len(es.families) == 300
        q1, q2, b1, b2 = E.overlap_pairs(raw)
        assert int((q1 + q2 > 93).sum()) > 200


@pytest.mark.parametrize("pre,post", E.RATES_ACCEPTED + E.RATES_REFUSED)
def test_restatement_vs_fp64_at_other_rates(pre, post):
    """oracle.run(pre=, post=) against fv.ss_vote(pre=, post=) on the parameter input.  The two
    pairs libbsdc refuses are in: the restatements have no such limit, and at (60, 40) the
    single-strand qualities pass 46 -- the agreement table's last entry (tests/test_abi.py)."""
    es = E.params_case()
    r = oracle.run(es.raw, es.ref, pre=pre, post=post, keep_sources=True)
    src = r.sources
    import fgbio_vote as fv
    ss = fv.ss_vote(src["count"], src["len"], src["base"], src["qual"], r.ss["base"].shape[2], pre=pre, post=post)
    c = fv.compare_ss(r.ss, ss)
    assert_fp64_bar(c, "params (%g, %g)" % (pre, post))
    qmax = int(r.ss["qual"][live_ss(r)].max())
    assert qmax == int(pre)  # a column's quality reaches floor(pre)
    if (pre, post) == (60.0, 40.0):
        assert int((live_ss(r) & (r.ss["qual"] >= 47)).sum()) > 1000


def test_parameter_cases_do_something():
    """overlap off changes over 100 consensus columns; min_consensus_base_quality 94 masks every
    single-strand column, 40 some of them and 0 none but the depth-0 ones."""
    es = E.params_case()
    on, off = oracle.run(es.raw, es.ref), oracle.run(es.raw, es.ref, overlap=False)
    assert np.array_equal(on.cons_len, off.cons_len)
    assert int(((on.cons_seq != off.cons_seq) | (on.cons_qual != off.cons_qual)).sum()) > 100
    n_masked = []
    for m in (0, 2, 10, 40, 94):
        r, ss, c = fp64_check(es.raw, es.ref, min_consensus_base_quality=m)
        assert_fp64_bar(c, "min_cbq %d" % m)
        live = live_ss(r) & (r.status == 1)[:, None, None]
        n_masked.append(int((live & (r.ss["base"] == 15) & (r.ss["qual"] == 2)).sum()))
        if m == 94:
            assert n_masked[-1] == int(live.sum())
    assert n_masked == sorted(n_masked) and n_masked[0] < n_masked[2] < n_masked[3] < n_masked[4]

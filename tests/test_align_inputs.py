"""The alignment-edge cases (tests/align_inputs.py) on the CPU: every case reaches the path it is
built for (complex and read-through records counted on the device batch, reads trimmed and reads
the filter rejected counted on the restatement's source reads), the restatement's source reads
equal what a few lines of plain Python derive from the case's own description -- the kept length
after the read-through and trailing-N trims, the filter's survivors, the qualities after the
overlap consensus -- and its vote meets the fp64 bar, so tests/test_gpu_align_edges.py compares
the kernels against something that is neither vacuous nor a shared misreading of a boundary.
"""
import re

import numpy as np
import pytest

import align_inputs as A
import edge_inputs as E
from bsseqconsensusreads_amd import batch
from test_fgbio_vote import assert_fp64_bar, fp64_check

_runs = {}
COMP = {E.A: E.T, E.T: E.A, E.C: E.G, E.G: E.C, E.N: E.N}


def run(name):
    """(case, oracle result with sources, fp64 single-strand reads, their comparison), once."""
    if name not in _runs:
        c = A.case(name)
        _runs[name] = (c,) + fp64_check(c.raw, c.ref, run_tools=c.run_tools)
    return _runs[name]


def sources_by_mi(r):
    """MI -> per set the source reads [(len, bases, quals)] in the vote's order (an MI that
    TemplateCoordinate order breaks into several runs has its families' reads concatenated)."""
    out = {}
    ri = bi = 0
    for f in range(len(r.status)):
        sets = out.setdefault(int(r.fam_mi[f]), [[], [], [], []])
        for s in range(4):
            for _ in range(int(r.sources["count"][f, s])):
                n = int(r.sources["len"][ri])
                sets[s].append((n, r.sources["base"][bi:bi + n], r.sources["qual"][bi:bi + n]))
                ri += 1
                bi += n
    return out


def counters(name):
    """What proves reach, per case: records, complex and read-through records on the device
    batch, source reads kept, reads shortened, reads dropped (emptied by a trim or rejected)."""
    c, r, _, _ = run(name)
    fb = batch.build_family_batch(c.raw, "full" if c.run_tools else "vote", c.ref)
    kept = [n for sets in sources_by_mi(r).values() for s in sets for n, _, _ in s]
    return {"records": int(c.raw.n), "complex": int(((fb.rec_link & batch.LINK_COMPLEX) != 0).sum()),
            "rt": int(((fb.rec_link & batch.LINK_RT) != 0).sum()), "kept": len(kept),
            "dropped": int(r.tool2.src.shape[0]) - len(kept), "emitted": int(r.status.sum()), "families": len(r.status)}


# ---- the case's own description, restated in plain Python ----------------------------------------------
def ops_of(cigar):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def aligned(rec):
    """[(reference position, read offset)] of the record's aligned bases."""
    out, rp, qp = [], rec.pos, 0
    for n, op in ops_of(rec.cigar):
        if op in "M=X":
            out += [(rp + i, qp + i) for i in range(n)]
        if op in "M=XDN":
            rp += n
        if op in "M=XIS":
            qp += n
    return out


def mate_unclipped(rec):
    """(start, end) of the mate with its clips, as PNEXT and MC state them."""
    ops = ops_of(rec.mc)
    lead = trail = 0
    for n, op in ops:
        if op not in "SH":
            break
        lead += n
    for n, op in reversed(ops):
        if op not in "SH":
            break
        trail += n
    return rec.next_pos - lead, rec.next_pos + sum(n for n, op in ops if op in "M=XDN") - 1 + trail


def expected_keep(rec, seq):
    """Source length of the record: fgbio's read-through trim (a mapped FR pair on one contig with
    MC: a forward read loses what lies past the mate's unclipped end, a reverse read what lies
    before the mate's unclipped start), then the trailing Ns in sequencing order.  Where the mate's
    end falls inside a deletion of this read, this takes the last aligned base before it -- the
    reading oracle/ and the kernels make too; SURVEY.md 8a row 4 does not pin fgbio's behaviour at
    that one point (its readPosAtRefPos may answer differently inside a deletion), so there, and
    only there, this check is not independent."""
    L, neg = rec.read_len, bool(rec.flag & 16)
    keep = L
    if rec.mc is not None and rec.next_tid == 0 and not (rec.flag & 12) and bool(rec.flag & 32) != neg:
        end = rec.pos + rec.ref_len - 1
        five_pos, five_neg = (rec.next_pos, end) if neg else (rec.pos, rec.pos + rec.tlen)
        if five_pos < five_neg:
            us, ue = mate_unclipped(rec)
            if not neg and end > ue:
                keep = max([o + 1 for p, o in aligned(rec) if p <= ue], default=0)
            if neg and rec.pos < us:
                keep = L - min([o for p, o in aligned(rec) if p >= us], default=L)
    b = seq[::-1] if neg else seq
    while keep > 0 and b[keep - 1] == E.N:
        keep -= 1
    return keep


def set_of(rec):
    r1 = bool(rec.flag & 0x40)
    return (0 if r1 else 1) if rec.strand == "A" else (2 if r1 else 3)


def record_index(c):
    """(family, record in family) -> input record."""
    out, k = {}, 0
    for f, fam in enumerate(c.fams):
        for j in range(len(fam.recs)):
            out[f, j] = k
            k += 1
    return out


# ---- the builder ---------------------------------------------------------------------------------------
def test_builder_is_deterministic_and_writes_what_the_description_says():
    a, b = A.trim_case(), A.trim_case()
    for k in ("flag", "pos", "seq", "qual", "cigar", "next_pos", "next_tid", "tlen", "mc_cigar", "mc_off"):
        assert np.array_equal(getattr(a.raw, k), getattr(b.raw, k)), k
    assert not np.array_equal(a.raw.seq, A.trim_case(seed=99).raw.seq)
    idx = record_index(a)
    for f, fam in enumerate(a.fams):
        for j, rec in enumerate(fam.recs):
            k = idx[f, j]
            assert (int(a.raw.flag[k]), int(a.raw.pos[k]), int(a.raw.next_pos[k]), int(a.raw.tlen[k]), int(a.raw.next_tid[k])) == \
                (rec.flag, rec.pos, rec.next_pos, rec.tlen, rec.next_tid)
            assert int(a.raw.l_seq[k]) == rec.read_len and (a.raw.mc_off[k] >= 0) == (rec.mc is not None)
            assert [(int(x) >> 4, "MIDNSHP=X"[int(x) & 0xF]) for x in a.raw.record_cigar(k)] == ops_of(rec.cigar)
    stale = sum(rec.next_pos != mate.pos or rec.mc != mate.cigar or rec.next_tid != 0
                for fam in a.fams for rec, mate in ((fam.recs[0], fam.recs[1]), (fam.recs[1], fam.recs[0])))
    assert stale >= 12  # the mate fields disagree with the mate where the case says so
    for name in A.CASES:
        c = A.case(name)
        assert len(c.fams) <= 300 and 1 <= int(c.raw.l_seq.min()) and int(c.raw.l_seq.max()) <= 48


# ---- reach and non-vacuity, every case -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.CASES))
def test_case_reaches_its_path(name):
    c, r, ss, cmp = run(name)
    n = counters(name)
    print(name, n)
    assert_fp64_bar(cmp, name)
    assert 2 * n["emitted"] >= n["families"] > 0
    assert n["complex"] > 0
    if name in ("filter", "near_tie", "groups", "groups_control", "tools"):
        assert n["dropped"] > 0  # (no trim empties a read in these: every dropped read is the filter's)
    if name in ("filter", "near_tie", "groups", "groups_control"):
        assert n["dropped"] == sum(f.note.get("rejected", 0) for f in c.fams)
    if name == "trim":
        assert n["rt"] >= 40 and n["dropped"] >= 3
    if name == "shapes":
        assert n["complex"] == 4 * (len(A.SHAPES) - 1) and n["dropped"] == 0  # (10=1X19= alone is not complex)


def test_shape_list_holds_what_it_promises():
    ops = {s: ops_of(s) for s in A.SHAPES}
    has = lambda pred: any(pred(o) for o in ops.values())
    for op in "ID":
        assert has(lambda o: o[0] == (1, "M") and o[1] == (1, op)) and has(lambda o: o[-1] == (1, "M") and o[-2][1] == op)
        assert has(lambda o: any(x == (5, op) for x in o))
    assert has(lambda o: any(a[1] == "I" and b[1] == "D" for a, b in zip(o, o[1:])))
    assert has(lambda o: any(a[1] == "D" and b[1] == "I" for a, b in zip(o, o[1:])))
    assert has(lambda o: any(x[1] == "N" for x in o)) and has(lambda o: {"=", "X"} <= {x[1] for x in o})
    assert has(lambda o: sum(x[1] in "ID" for x in o) == 2) and has(lambda o: sum(x[1] in "ID" for x in o) == 3)
    assert has(lambda o: len(o) >= 12)
    assert has(lambda o: o[0][1] == "H" and o[1][1] == "S") and has(lambda o: o[-1][1] == "H" and o[-2][1] == "S")
    assert has(lambda o: o == [(29, "S"), (1, "M")]) and has(lambda o: o == [(1, "M"), (29, "S")])


# ---- hand-derived expectations ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shapes", "overlap", "overlap_wild", "filter", "near_tie", "groups", "groups_control"])
def test_survivors_are_the_hand_written_ones(name):
    """Per family and set, the source lengths in the vote's order equal expect_lens, which each
    case states by hand."""
    c, r, _, _ = run(name)
    got = sources_by_mi(r)
    assert sorted(got) == list(range(len(c.fams)))
    for f, fam in enumerate(c.fams):
        want = [list(fam.expect_lens.get(s, [])) for s in range(4)]
        assert [[n for n, _, _ in s] for s in got[f]] == want, "%s family %d (%s)" % (name, f, fam.what)


def test_trims_keep_the_hand_derived_lengths():
    c, r, _, _ = run("trim")
    got = sources_by_mi(r)
    idx = record_index(c)
    shortened = whole = emptied = 0
    for f, fam in enumerate(c.fams):
        want = [[], [], [], []]
        for j, rec in enumerate(fam.recs):
            keep = expected_keep(rec, c.raw.record_seq(idx[f, j]))
            if keep:
                want[set_of(rec)].append(keep)
            shortened += 0 < keep < rec.read_len
            whole += keep == rec.read_len
            emptied += keep == 0
        assert [[n for n, _, _ in s] for s in got[f]] == want, "family %d (%s)" % (f, fam.what)
    print("trim: %d reads shortened, %d whole, %d emptied" % (shortened, whole, emptied))
    assert shortened >= 30 and whole >= 30 and emptied >= 3
    # the families named after what they expect, spelled out (forward record 0, reverse record 1)
    named = {fam.what: [expected_keep(rec, c.raw.record_seq(idx[f, j])) for j, rec in enumerate(fam.recs)]
             for f, fam in enumerate(c.fams)}
    at_ = {fam.what: f for f, fam in enumerate(c.fams)}
    for d, keep in ((-3, 30), (-1, 30), (0, 30), (1, 29), (2, 28), (12, 18)):
        assert named["simple forward ends %d past the mate's end" % d][0] == keep
        assert named["simple reverse starts %d before the mate's start" % d][1] == (30 + d if d <= 0 else 30)
    for e, keep in ((8, 9), (9, 10), (10, 10), (11, 10), (12, 10), (13, 11), (14, 12)):
        assert named["forward 10M3D20M, mate ends at +%d" % e][0] == keep
    for e, keep in ((8, 9), (9, 10), (10, 14), (11, 15)):
        assert named["forward 10M3I17M, mate ends at +%d" % e][0] == keep
    for b, keep in ((16, 14), (19, 11), (20, 10), (21, 10), (22, 10)):
        assert named["reverse 20M3D10M, mate starts at +%d" % b][1] == keep
    for b, keep in ((16, 14), (17, 10), (18, 9)):
        assert named["reverse 17M3I10M, mate starts at +%d" % b][1] == keep
    assert named["forward trimmed to 0 bases"][0] == 0 and named["reverse trimmed to its last 2 bases"][1] == 2
    assert named["forward trim uncovers 3 Ns"][0] == 17 and named["reverse trim uncovers 2 Ns"][1] == 24
    assert named["MC 20M2S3H: mate end +5"][0] == 25 and named["MC 2H3S30M: reverse sees the mate start 5 earlier"][1] == 31
    for what in ("tlen 0", "tlen of the wrong sign", "flag & 32 equal to flag & 16 (forward)", "mate on another contig", "no MC"):
        assert named[what][0] == 30, what
    for what in ("AB-R1 all N, BA survives", "AB-R1 trimmed to 0 bases, BA survives"):
        assert named[what] == [0, 30, 30, 30] and [len(x) for x in got[at_[what]]] == [0, 1, 1, 1], what
        f = int(np.nonzero(r.fam_mi == at_[what])[0][0])
        assert r.status[f] == 1  # the pair is emitted, its first read from BA-R2 alone
    assert named["all-N forward read: AB-R1 empty"] == [0, 30] and named["all-N reverse read: AB-R2 empty"] == [30, 0]
    assert named["forward read whose only base is the first"][0] == 1
    assert named["reverse read whose only base is the first in record order"][1] == 30
    assert named["reverse read with a leading N run in record order"][1] == 23
    # the candidate window of batch.py: a record up to 2 bases short of the mate's end is a
    # candidate (the tools may yet extend it), one 3 short is not
    fb = batch.build_family_batch(c.raw, "vote", c.ref)
    rt = np.zeros(c.raw.n, bool)
    rt[fb.src] = (fb.rec_link & batch.LINK_RT) != 0
    at = {fam.what: f for f, fam in enumerate(c.fams)}
    for d, want in ((-3, False), (-2, False), (-1, True), (0, True), (1, True)):
        assert rt[idx[at["simple forward ends %d past the mate's end" % d], 0]] == want, d
        assert rt[idx[at["simple reverse starts %d before the mate's start" % d], 1]] == want, d
    for d, want in ((-3, False), (-2, False), (-1, True), (0, True)):
        assert rt[idx[at["forward 10M2I18M1D2M ends %d past the mate's end" % d], 0]] == want, d


@pytest.mark.parametrize("name", ["overlap", "overlap_wild"])
def test_overlap_consensus_values(name):
    """The source reads of each single-template family equal the records after the overlap rule
    applied by hand at every reference position both mates have a base at: equal bases sum their
    qualities (cap 93), unequal ones take the better base at the difference, equal qualities N at
    Q2; an N on either side leaves both alone."""
    c, r, _, _ = run(name)
    got = sources_by_mi(r)
    idx = record_index(c)
    changed = 0
    for f, fam in enumerate(c.fams):
        recs = fam.recs
        b = [c.raw.record_seq(idx[f, j]).copy() for j in (0, 1)]
        q = [c.raw.record_qual(idx[f, j]).astype(np.int64) for j in (0, 1)]
        m0, m1 = dict(aligned(recs[0])), dict(aligned(recs[1]))
        both = sorted(set(m0) & set(m1))
        for p in both:
            i, j = m0[p], m1[p]
            if b[0][i] == E.N or b[1][j] == E.N:
                continue
            changed += 1
            if b[0][i] == b[1][j]:
                q[0][i] = q[1][j] = min(q[0][i] + q[1][j], 93)
            elif q[0][i] != q[1][j]:
                w = 0 if q[0][i] > q[1][j] else 1
                b[0][i] = b[1][j] = (b[0][i], b[1][j])[w]
                q[0][i] = q[1][j] = abs(q[0][i] - q[1][j])
            else:
                b[0][i] = b[1][j] = E.N
                q[0][i] = q[1][j] = 2
        (n0, b0, q0), = got[f][0]
        (n1, b1, q1), = got[f][1]
        assert np.array_equal(b0, b[0]) and np.array_equal(q0, q[0]), fam.what
        assert np.array_equal(b1, np.array([COMP[int(x)] for x in b[1][::-1]], np.uint8)), fam.what
        assert np.array_equal(q1, q[1][::-1]), fam.what
    assert changed > 100
    one = [fam for fam in c.fams if fam.what.startswith("overlap of one position")]
    assert len(one) == 2


def test_overlap_case_geometry():
    """The overlaps named in the case are the ones its cigars give."""
    c = A.case("overlap")
    n_both = {}
    for fam in c.fams:
        m0, m1 = dict(aligned(fam.recs[0])), dict(aligned(fam.recs[1]))
        n_both[fam.what] = sorted(set(m0) & set(m1))
    s = lambda what: [p - next(f for f in c.fams if f.what == what).recs[0].pos for p in n_both[what]]
    assert s("overlap of one position") == [29] and s("overlap of one position, both complex") == [28]
    assert s("no overlap: the mates abut") == []
    assert s("overlap begins on the base after R1's deletion")[0] == 24
    assert s("overlap begins inside R1's deletion")[0] == 24  # (R2 starts at 22, inside the deletion 20..23)
    assert s("overlap ends on the base before R2's insertion") == [29]
    assert s("overlap ends on R1's last base, R2's deletion next") == [29]
    assert len(s("insertion in R1 inside the overlap")) == 23 and len(s("deletion in R1 inside the overlap")) == 26


# ---- near ties under the filter -------------------------------------------------------------------------
def test_near_tie_picks_depend_on_the_filters_order():
    """The near-tie case holds exact ties of the fp64 sums, and columns whose fp64 pick in the
    filter's order (the restatement's, checked against fgbio_vote by the fp64 bar) differs from the
    pick the same reads give in input order: a vote that summed in input order would fail them."""
    import fgbio_vote as fv
    c, r, ss, cmp = run("near_tie")
    assert cmp["tie_columns"] > 50 and cmp["tie_diff"] == 0 and cmp["base_diff"] == 0, cmp
    src = r.sources
    cnt, lens = src["count"], src["len"]
    off = np.cumsum(lens) - lens
    order, ri = [], 0
    for f in range(cnt.shape[0]):
        for s in range(4):
            idx = list(range(ri, ri + int(cnt[f, s])))
            ri += int(cnt[f, s])
            if s == 0:  # the filter's order is t2, t3, t0, t1 (34, 34, 30, 30 bases); input order t0 .. t3
                assert [int(lens[i]) for i in idx] == [34, 34, 30, 30]
                idx = [idx[2], idx[3], idx[0], idx[1]]
            order += idx
    b = np.concatenate([src["base"][off[i]:off[i] + lens[i]] for i in order])
    q = np.concatenate([src["qual"][off[i]:off[i] + lens[i]] for i in order])
    by_input = fv.ss_vote(cnt, lens[order], b, q, r.ss["base"].shape[2])
    differ = by_input["base"][:, 0] != ss["base"][:, 0]
    print("near_tie: %d exact-tie columns, %d columns whose pick depends on the order" % (cmp["tie_columns"], int(differ.sum())))
    assert int(differ.sum()) > 50
    assert np.array_equal(r.ss["base"][:, 0][differ], ss["base"][:, 0][differ])  # the restatement takes the filter's order
    assert not (by_input["base"][:, 1:] != ss["base"][:, 1:]).any()

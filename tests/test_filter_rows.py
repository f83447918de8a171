"""The fabricated filter inputs of tests/filter_rows.py against the ground each set is for, on the
CPU with tests/filter_ref.py alone: the float32 read-rate ties and their neighbours, the per-base
fp64 grid against e / d > T in Python floats, the depth thresholds, the two checks after masking,
the one-column masks, the sums past 2^31, and that no verdict depends on the garbage past the
lengths.  test_gpu_filter_rows.py runs the same sets through the kernel."""
import numpy as np
import pytest

import filter_ref as FR
import filter_rows as W

GATE_DROPPED_AT_TIE = {0.025: True, 0.1: True, W.F32_THIRD_BELOW: True, 0.7: False, 0.35: False, W.F32_THIRD: False,
                       0.125: False}
PAIR_OF = {t: pair for pair, ties in W.GATE_PAIRS.items() for t, _ in ties}


def test_gate_pairs_round_as_the_sets_assume():
    """float32 rounds 1/40 and 1/10 up past the double threshold and 7/10 and 7/20 down; 1/3 is
    float32(1/3), one ulp above its neighbour; 1/8 is exact"""
    f = lambda a, b: float(np.float32(a) / np.float32(b))  # noqa: E731
    assert f(1, 40) > 0.025 and f(1, 10) > 0.1 and f(7, 10) < 0.7 and f(7, 20) < 0.35 and f(1, 8) == 0.125
    assert f(1, 3) == W.F32_THIRD > W.F32_THIRD_BELOW
    for t, drop in GATE_DROPPED_AT_TIE.items():
        assert dict(W.GATE_PAIRS[PAIR_OF[t]])[t] == drop
    for (num, den) in W.GATE_PAIRS:
        ks = W.gate_ks(den)
        assert len(ks) >= 6 and ks[-1] * den > W.GATE_L * 255 >= ks[0] * den  # byte rows and wide rows


@pytest.mark.parametrize("name", ["gate32", "gate32_mol"])
@pytest.mark.parametrize("t", sorted(GATE_DROPPED_AT_TIE))
def test_gate32_ties_and_their_neighbours(name, t):
    x = W.make(name)
    seen = set()
    for s in range(3):
        filt = W.reference(name, "E%r_slot%d" % (t, s))[0]
        assert not (filt & (255 ^ FR.READERR)).any()
        for f, m in enumerate(x.fam):
            if s not in m["slots"] or m["pair"] != PAIR_OF[t]:
                continue
            want = {-1: False, 0: GATE_DROPPED_AT_TIE[t], 1: True}[m["delta"]]
            assert (filt[f] == FR.READERR) == want, (name, t, s, m)
            seen.add((s, m["shape"], m["delta"], m["k"] * m["pair"][1] > W.GATE_L * 255))
    # every shape met in its slot, with every neighbour, on byte rows and on wide rows
    shapes = {("mol", 0)} if x.kind else {("a_max", 2), ("b_max", 2), ("a_min", 1), ("b_min", 1), ("c", 0), ("c_disagree", 0),
                                          ("ab_only", 0), ("ab_only", 2), ("ba_only", 2), ("a_nodepth", 2), ("b_nodepth", 0)}
    for shape, s in shapes:
        for delta in (-1, 0, 1):
            assert any((s, shape, delta, w) in seen for w in (False, True)), (shape, s, delta)
    assert {w for _, sh, _, w in seen if sh in ("mol", "c")} == {False, True}


@pytest.mark.parametrize("name", ["gate32", "gate32_mol"])
def test_gate32_sums_are_the_pairs(name):
    """each tie family holds the sums it is named for, in the rows the filter reads (the wide rows
    where it has them; its byte rows then hold garbage)"""
    x = W.make(name)
    n_wide = 0
    for f, m in enumerate(x.fam):
        if "pair" not in m:
            continue
        E, D = m["k"] * m["pair"][0] + m["delta"], m["k"] * m["pair"][1]
        for e in range(2):
            ae, ad, be, bd = x.sums(f, e)
            if m["shape"] in ("mol", "a_max", "a_min", "ab_only", "b_nodepth"):
                assert (ae, ad) == (E, D), m
            elif m["shape"] in ("b_max", "b_min", "ba_only", "a_nodepth"):
                assert (be, bd) == (E, D), m
            else:
                assert ad + bd == D and (m["shape"] == "c_disagree" or ae + be == E), m
        n_wide += D > W.GATE_L * 255
        if not m["shape"].startswith("c"):  # (a pair split over both strands may still fit bytes)
            assert (x.ss_wide[f] >= 0) == (D > W.GATE_L * 255)
    assert n_wide >= 10


def test_gate32_each_slot_decides_alone():
    """with 0.1 in one slot and 1.0 in the others some family is dropped, and kept once that slot is
    1.0 too; with 0.1 in all three, lifting the duplex or the BA slot alone changes a verdict (the AB
    slot's min(aE, bE) never exceeds what the BA slot's max does)"""
    lax, allthree = W.reference("gate32", "lax")[0], W.reference("gate32", "E0.1_all")[0]
    assert not lax[W.make("gate32").notes["ab_only"]].any()
    for s in range(3):
        one = W.reference("gate32", "E0.1_slot%d" % s)[0]
        assert ((one == FR.READERR) & (lax == 0)).any(), s
        if s != 1:
            but = W.reference("gate32", "E0.1_all_but%d" % s)[0]
            changed = np.nonzero((allthree != 0) & (but == 0))[0]
            assert changed.size and (one[changed] == FR.READERR).all(), s
    f = W.make("gate32").notes["c_only"][0]
    assert allthree[f] == FR.READERR and W.reference("gate32", "E0.1_all_but0")[0][f] == 0
    assert W.reference("gate32", "E0.125_slot0")[0][f] == 0  # 10 / 80 is exact


def test_gate32_no_depth_families():
    x = W.make("gate32")
    for pn in x.params:
        filt = W.reference("gate32", pn)[0]
        assert (filt[x.notes["no_depth"]] == 0).all(), pn                 # NaN exceeds nothing
        assert (filt[x.notes["err_no_depth"]] == FR.READERR).all(), pn    # inf exceeds everything
    assert all(len(x.notes[k]) >= 18 for k in ("ab_only", "ba_only", "a_nodepth", "b_nodepth"))


@pytest.mark.parametrize("name", ["base64", "base64_mol"])
@pytest.mark.parametrize("t", W.BASE_THRESHOLDS)
def test_base64_masks_are_e_over_d_in_python_floats(name, t):
    x = W.make(name)
    exact_kept, per_slot = 0, [0, 0, 0]
    for s in range(3):
        filt, masked, seq, _ = W.reference(name, "B%r_slot%d" % (t, s))
        assert not filt.any()
        for f, m in enumerate(x.fam):
            if s not in m["slots"]:
                continue
            for e in range(2):
                want = np.asarray([d > 0 and er / d > t for er, d in m["cols"][e]], bool)
                got = seq[f, e, :len(want)] == W.N
                assert np.array_equal(got, want), (name, t, s, m["app"], e)
                assert masked[f, e] == want.sum()
                exact_kept += sum(1 for (er, d), g in zip(m["cols"][e], got) if d > 0 and er / d == t and not g)
                per_slot[s] += int(want.sum())
    if t in (0.1, 0.025, 0.5):
        assert exact_kept >= 1
    if t < 1.0 or x.kind == 1:
        assert all(n > 0 for n in per_slot[:1 if x.kind else 3]), per_slot


def test_base64_grid_is_whole():
    assert len(W.BASE_GRID) == sum(d + 2 for d in range(41))
    for name, apps in (("base64", set(W.BASE_APPS)), ("base64_mol", {"mol"})):
        x = W.make(name)
        for app in apps:
            cols = [c for f in x.notes[app] for part in x.fam[f]["cols"] for c in part]
            assert sorted(cols) == sorted(W.BASE_GRID), app
    # a strand with no read in the column: min is 0, max the other strand's rate
    x = W.make("base64")
    f = x.notes["a_zero"][1]
    assert (x.ss_depth[f, 3, :16] == 0).all() and (x.ss_depth[f, 0, :16] > 0).all()


def _sole(filt, fams, bit):
    return (filt[fams] == bit).any()


def test_reads_thresholds():
    x = W.make("reads")
    per_read = x.notes["per_read"] + x.notes["per_read_one_strand"] + x.notes["byte255"] + x.notes["wide256"] + x.notes["wide_max"]
    for pn, M in W.READS_MIN.items():
        filt, masked, seq, _ = W.reference("reads", pn)
        assert not (filt & (255 ^ FR.MINREADS)).any()
        for f in per_read:  # hand rule on the uniform families
            a, b = x.fam[f]["depth"]
            M3 = FR.three(M)
            want = a + b < M3[0] or max(a, b) < M3[1] or min(a, b) < M3[2]
            assert (filt[f] != 0) == want, (pn, a, b)
        if pn == "M65535":
            assert filt[(x.status & 1) == 1].all()  # drops everything
        elif pn == "M0":
            assert not filt.any()
        else:
            assert (filt[per_read] == 0).any() and (filt[per_read] == FR.MINREADS).any()
    for pn, M in (("M3_2_1", (3, 2, 1)), ("M2_1_0", (2, 1, 0)), ("M1", (1, 1, 1))):  # per base
        filt, masked, seq, _ = W.reference("reads", pn)
        for f in x.notes["per_base"]:
            L = int(x.length[f, 0])
            ad, bd = x.ss_depth[f, 0, :L].astype(int), x.ss_depth[f, 3, :L].astype(int)
            want = (ad + bd < M[0]) | (np.maximum(ad, bd) < M[1]) | (np.minimum(ad, bd) < M[2])
            assert filt[f] == 0 and np.array_equal(seq[f, 0, :L] == W.N, want) and 0 < want.sum() < L
    f = x.notes["wide_max_per_base"][0]
    filt, masked, seq, _ = W.reference("reads", "M65534")
    assert filt[f] == 0 and (seq[f, 0, :8] == W.N).tolist() == [False, True, True, True, True, True, True, False]
    assert filt[x.notes["wide_max"]].tolist() == [0, FR.MINREADS, FR.MINREADS]
    assert int(x.ss_wdepth[x.ss_wide[x.notes["wide_max"][0]], 0, 0]) == 32767
    assert (x.ss_wide[x.notes["wide256"]] >= 0).all() and (x.ss_wide[x.notes["byte255"]] == -1).all()
    filt = W.reference("reads", "M256_255_1")[0]
    assert filt[x.notes["byte255"]].tolist() == [0, 1, 1, 1] and filt[x.notes["wide256"]].tolist() == [0, 0, 1, 1, 1]
    # the wide table's other shapes
    assert W.make("reads_nowide").ss_wide is None
    m1 = W.make("reads_minus1")
    assert (m1.ss_wide == -1).all() and m1.ss_wdepth.shape[0] == 1
    for pn in W.make("reads_nowide").params:
        assert np.array_equal(W.reference("reads_nowide", pn)[0], W.reference("reads_minus1", pn)[0])
    filt = W.reference("reads_mol", "M1")[0]
    assert filt[:5].tolist() == [1, 0, 0, 0, 0] and W.reference("reads_mol", "M3_2_1")[0][:5].tolist() == [1, 1, 1, 0, 0]


@pytest.mark.parametrize("name", ["after", "after_mol"])
def test_after_masking_ties(name):
    x = W.make(name)
    for frac in W.NOCALL_AT:
        filt, masked, seq, qual = W.reference(name, "n%r" % frac)
        here = [f for f in x.notes["nocall"] if x.fam[f]["nocall"][0] == frac]
        for f in here:
            m = x.fam[f]
            assert (filt[f] == FR.NOCALL) == (m["nocall"][1] > 0) and filt[f] in (0, FR.NOCALL), m
            assert masked[f].tolist() == [m["n"] - m["old"]] * 2  # (the old no-calls are not counted as masked)
            assert int((seq[f, 0, :x.length[f, 0]] == W.N).sum()) == m["n"]
        deltas = {x.fam[f]["nocall"][1] for f in here}
        assert 0 in deltas and (1 in deltas or frac == 1.0) and (-1 in deltas or frac == 0.0)
        assert {x.fam[f]["old"] > 0 for f in here} == {False, True} or frac == 0.0
    for mq in (30, 93):
        filt = W.reference(name, "q%d" % mq)[0]
        for f in x.notes["meanq"] + x.notes["meanq_old_n"]:
            m = x.fam[f]["meanq"]
            if m[0] == mq:
                assert filt[f] == (FR.MEANQ if m[1] < 0 else 0), m
                assert int(x.qual[f, 0, :8].astype(int).sum()) == mq * 8 + m[1]
    f, g = x.notes["qual_bytes"][0], x.notes["qual_bytes_n"][0]
    for nq, want in ((0, []), (2, [0, 5]), (93, [0, 1, 5, 6, 7])):
        filt, masked, seq, qual = W.reference(name, "N%d" % nq)
        assert np.nonzero(seq[f, 0, :8] == W.N)[0].tolist() == want and masked[f, 0] == len(want)
        assert qual[g, 0, :8].tolist() == [2 if (k in want and k % 2 == 0) else int(x.qual[g, 0, k]) for k in range(8)]
    for k in ("len0_end0", "len0_end1", "len0_both"):
        f = x.notes[k][0]
        assert 0 in x.length[f].tolist()
        assert W.reference(name, "N93_n0.25_q30")[0][f] == (0 if k == "len0_both" else FR.NOCALL | FR.MEANQ)
        assert W.reference(name, "M1")[0][f] == FR.MINREADS
    # each reason alone
    em = np.nonzero(x.status & 1)[0]
    assert _sole(W.reference(name, "M1")[0], em, FR.MINREADS) and _sole(W.reference(name, "E0.5")[0], em, FR.READERR)
    assert _sole(W.reference(name, "n0.25")[0], em, FR.NOCALL) and _sole(W.reference(name, "q30")[0], em, FR.MEANQ)
    assert W.reference(name, "E0.5")[0][x.notes["readerr"]].tolist() == [FR.READERR]


@pytest.mark.parametrize("stride", [16, 32, 1040])
def test_lanes_one_column_each(stride):
    name = "lanes%d" % stride
    x = W.make(name)
    assert x.stride == stride
    Ls = {int(k[1:]) for k in x.notes if k[0] == "L"}
    assert Ls == {n for n in W.LANE_LENGTHS + (stride - 1, stride) if n <= stride}
    filt, masked, seq, qual = W.reference(name, "q10")
    before = W.unpack(x.seq)
    cols = set()
    for f in x.notes["one_hot"]:
        c = x.fam[f]["one_hot"]
        cols.add(c)
        for e in range(2):
            assert np.nonzero(seq[f, e] != before[f, e])[0].tolist() == [c] and masked[f, e] == 1 and filt[f] == 0
            assert qual[f, e, c] == 2 and np.array_equal(np.delete(qual[f, e], c), np.delete(x.qual[f, e], c))
    assert {c % 16 for c in cols} == set(range(16)) if stride == 16 else {0, 15} <= {c % 16 for c in cols}
    if stride == 1040:
        assert {0, 511, 512, 1023, 1024, 1039} <= cols
    f = x.notes["disagree"][0]
    c = x.fam[f]["disagree"]
    assert (x.ss_base[f] > 15).all() and masked[f].tolist() == [0, 0]
    f2, m2, s2, _ = W.reference(name, "q10_agree")
    assert m2[f].tolist() == [1, 1] and np.nonzero(s2[f, 0] != before[f, 0])[0].tolist() == [c]
    for k, bad in (("end0_fails", 0), ("end1_fails", 1)):
        f = x.notes[k][0]
        assert filt[f] == FR.MINREADS and masked[f, bad] == 0 and masked[f, 1 - bad] == 1
        assert np.array_equal(seq[f, bad], before[f, bad]) and np.array_equal(qual[f, bad], x.qual[f, bad])
        assert seq[f, 1 - bad, stride // 2] == W.N and qual[f, 1 - bad, stride // 2] == 2
    for pn in ("typical", "single_ok"):  # the messy families give the filter something to decide
        filt, masked, _, _ = W.reference(name, pn)
        em = (x.status & 1) == 1
        assert (filt[em] == 0).any() and (filt[em] != 0).any() and masked[filt == 0].sum() > 0, pn


def test_long_sums_pass_2_31():
    x = W.make("long")
    assert x.stride == 65520 and x.length.tolist() == [[65519, 65519]] * 2
    f = x.notes["duplex"][0]
    for e in range(2):
        ae, ad, be, bd = x.sums(f, e)
        assert (ae + be, ad + bd) == x.fam[f]["sums"]
        for s in (ae + be, ad + bd):
            assert 2 ** 31 < s < 2 ** 32
        wd = x.ss_wdepth[x.ss_wide[f]]
        assert (wd[e, 1:65519] == 32767).all() and (wd[3 - e, 1:65519] == 32767).all()
    g = x.notes["ab_only"][0]
    assert x.ss_len[g].tolist() == [65519, 65519, 0, 0]
    verdicts = {pn: int(W.reference("long", pn)[0][f]) for pn in x.params}
    assert verdicts["E_at"] == 0 and verdicts["E_below"] == FR.READERR
    assert W.reference("long", "E_at")[1][f].tolist() == [5, 5]  # and an end that passes is masked


def test_counts_patterns():
    for n, pat in W.COUNTS.items():
        x = W.make("counts%d" % n)
        assert x.n_fam == n and "".join(str(int(s) & 1) for s in x.status) == pat
        filt, masked, _, _ = W.reference(x.name, "q10")
        off = (x.status & 1) == 0
        assert not filt[off].any() and not masked[off].any()
    assert set(W.COUNTS) == {0, 1, 3, 4, 5, 9}


@pytest.mark.parametrize("name", [s for s in W.SETS if s != "lanes1040"])
def test_verdicts_do_not_depend_on_the_garbage(name):
    """the bytes past the lengths, in absent strands, in families not emitted and in the byte rows
    under a wide row re-drawn with another seed: the same verdicts, masks and bases inside the lengths"""
    x, y = W.make(name), W.make(name, 1)
    assert x.n_fam == y.n_fam
    if x.n_fam:
        assert not np.array_equal(x.qual, y.qual) or not x.qual.size
    pns = list(x.params)
    for pn in pns[:2] + pns[-2:] if name != "long" else pns[-1:]:
        a, b = W.reference(name, pn), W.reference(name, pn, 1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, pn)
        live = (np.arange(x.stride)[None, None, :] < x.length[:, :, None]) & ((x.status & 1) == 1)[:, None, None]
        assert np.array_equal(a[2][live], b[2][live]) and np.array_equal(a[3][live], b[3][live])

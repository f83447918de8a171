"""The numpy restatement of the consensus filter (tests/filter_ref.py) against
hand-derived answers on tiny hand-built single-strand rows, and the inputs of test_gpu_filter.py
against the ground they must reach -- on the CPU, with oracle/ alone."""
import numpy as np
import pytest

import filter_inputs as FI
import filter_ref as FR

A, C, G, T, N = 1, 2, 4, 8, 15
S = 16  # stride of the hand-built rows


def rows(F=1):
    """All-zero single-strand rows and consensus of F families; fill in what a case needs."""
    ss = {"len": np.zeros((F, 4), np.int32), "base": np.full((F, 4, S), N, np.uint8), "qual": np.zeros((F, 4, S), np.uint8),
          "depth": np.zeros((F, 4, S), np.uint16), "err": np.zeros((F, 4, S), np.uint16)}
    return ss, np.full((F, 2, S), N, np.uint8), np.zeros((F, 2, S), np.uint8), np.zeros((F, 2), np.int32), np.ones(F, np.int32)


def strand(ss, s, base, qual, depth, err, f=0):
    n = len(base)
    ss["len"][f, s] = n
    ss["base"][f, s, :n], ss["qual"][f, s, :n], ss["depth"][f, s, :n], ss["err"][f, s, :n] = base, qual, depth, err


def molecular_pair(depth, err, L=8):
    """One step-1 family whose two ends are alike: L columns of A at Q40."""
    ss, seq, qual, ln, st = rows()
    for e in range(2):
        strand(ss, e, [A] * L, [40] * L, depth, err)
        seq[0, e, :L], qual[0, e, :L], ln[0, e] = A, 40, L
    return ss, seq, qual, ln, st


def test_read_rate_is_a_float32_divide_compared_in_double():
    """1 error in 40 reads: float32(1/40) = 0.025000000372..., above the double 0.025 -> dropped;
    1 in 8 is exact in both -> kept."""
    case = molecular_pair([5] * 8, [1] + [0] * 7)
    filt, masked, _, _ = FR.apply(*case, molecular=True, **dict(FI.LAX, max_read_error_rate=(0.025,)))
    assert filt[0] == FR.READERR and masked.sum() == 0
    case = molecular_pair([1] * 8, [1] + [0] * 7)
    filt, masked, _, _ = FR.apply(*case, molecular=True, **dict(FI.LAX, max_read_error_rate=(0.125,)))
    assert filt[0] == 0 and masked.sum() == 0


def test_no_depth_is_dropped_by_min_reads_only():
    """Depth 0 everywhere: the rate is 0/0 = NaN, which exceeds no threshold (not even 0); the max
    depth 0 is below min_reads 1.  A read that fails the gate is not masked nor checked further:
    max_no_call_fraction 0 and min_mean_base_quality 93 add no reason."""
    ss, seq, qual, ln, st = molecular_pair([0] * 8, [0] * 8)
    p = dict(FI.LAX, min_reads=(1,), max_read_error_rate=(0.0,), max_no_call_fraction=0.0, min_mean_base_quality=93,
             min_base_quality=93)
    filt, masked, s2, q2 = FR.apply(ss, seq, qual, ln, st, molecular=True, **p)
    assert filt[0] == FR.MINREADS and masked.sum() == 0
    assert np.array_equal(s2, seq) and np.array_equal(q2, qual)
    filt, _, _, _ = FR.apply(ss, seq, qual, ln, st, molecular=True, **dict(p, min_reads=(0,), min_base_quality=0,
                                                                          min_mean_base_quality=-1, max_no_call_fraction=1.0))
    assert filt[0] == 0


def duplex_family(ad, bd, ae=0, be=0, L=4):
    """One duplex family, both ends alike: AB rows (0, 1) at depth ad, BA rows (3, 2) at bd (None:
    the strand is absent), errors in column 0."""
    ss, seq, qual, ln, st = rows()
    for e in range(2):
        if ad is not None:
            strand(ss, e, [C] * L, [40] * L, [ad] * L, [ae] + [0] * (L - 1))
        if bd is not None:
            strand(ss, 3 - e, [C] * L, [30] * L, [bd] * L, [be] + [0] * (L - 1))
        seq[0, e, :L], qual[0, e, :L], ln[0, e] = C, 60, L
    return ss, seq, qual, ln, st


def test_two_values_expand_to_three():
    assert FR.three((3, 2)) == [3, 2, 2] and FR.three((5,)) == [5, 5, 5] and FR.three(4) == [4, 4, 4]
    assert FR.three((3, 2, 1)) == [3, 2, 1]
    case = duplex_family(2, 1)  # cD 3, max(aD, bD) 2, min(aD, bD) 1
    assert FR.apply(*case, **dict(FI.LAX, min_reads=(3, 2, 1)))[0][0] == 0
    assert FR.apply(*case, **dict(FI.LAX, min_reads=(3, 2)))[0][0] == FR.MINREADS      # BA needs 2
    assert FR.apply(*case, **dict(FI.LAX, min_reads=(3, 2, 2)))[0][0] == FR.MINREADS   # the same set


@pytest.mark.parametrize("only", ["AB", "BA"])
def test_one_strand_ends(only):
    """A family with one strand: that strand is 'a' whichever it is; bD = 0 and bE = 0, so min_reads
    (1) drops it and (1, 1, 0) keeps it, and the BA rate limit sees max(aE, 0) = aE."""
    case = duplex_family(4, None, ae=2) if only == "AB" else duplex_family(None, 4, be=2)
    assert FR.apply(*case, **dict(FI.LAX, min_reads=(1,)))[0][0] == FR.MINREADS
    p = dict(FI.LAX, min_reads=(1, 1, 0))
    filt, masked, _, _ = FR.apply(*case, **p)
    assert filt[0] == 0 and masked.sum() == 0
    # aE = 2 / 16 = 0.125: min(aE, bE) = 0 passes any AB limit, max(aE, bE) = 0.125 is held to the BA one
    assert FR.apply(*case, **dict(p, max_read_error_rate=(1.0, 0.0, 1.0)))[0][0] == 0
    assert FR.apply(*case, **dict(p, max_read_error_rate=(1.0, 1.0, 0.124)))[0][0] == FR.READERR
    assert FR.apply(*case, **dict(p, max_read_error_rate=(1.0, 1.0, 0.125)))[0][0] == 0
    # per base: column 0 has 2 errors in 4 reads; the other strand's rate is 0
    filt, masked, seq, qual = FR.apply(*case, **dict(p, max_base_error_rate=(1.0, 0.4, 1.0)))
    assert filt[0] == 0 and masked.sum() == 0
    filt, masked, seq, qual = FR.apply(*case, **dict(p, max_base_error_rate=(1.0, 1.0, 0.4)))
    assert filt[0] == 0 and masked.tolist() == [[1, 1]]
    assert seq[0, :, :4].tolist() == [[N, C, C, C]] * 2 and qual[0, :, :4].tolist() == [[2, 60, 60, 60]] * 2


def test_per_base_min_and_max_rate_with_a_zero_depth_strand():
    """Both strands present; in column 0 the BA strand has no read: its rate is 0 there, so the
    smaller rate is 0 and the larger is the AB strand's 2 / 4."""
    ss, seq, qual, ln, st = duplex_family(4, 3, ae=2)
    for e in range(2):
        ss["depth"][0, 3 - e, 0] = 0
    p = dict(FI.LAX, min_reads=(1, 1, 0))
    assert FR.apply(ss, seq, qual, ln, st, **dict(p, max_base_error_rate=(1.0, 0.4, 1.0)))[1].sum() == 0
    assert FR.apply(ss, seq, qual, ln, st, **dict(p, max_base_error_rate=(1.0, 1.0, 0.4)))[1].tolist() == [[1, 1]]
    assert FR.apply(ss, seq, qual, ln, st, **dict(p, max_base_error_rate=(0.4, 1.0, 1.0)))[1].tolist() == [[1, 1]]
    # and that column's smaller depth is 0: masked once the BA strand must show a read
    assert FR.apply(ss, seq, qual, ln, st, **dict(p, min_reads=(1, 1, 1)))[1].tolist() == [[1, 1]]


def test_strand_agreement_counts_a_no_call_as_a_disagreement():
    ss, seq, qual, ln, st = duplex_family(2, 2)
    for e in range(2):
        ss["base"][0, e, 1] = N      # AB calls nothing in column 1, BA calls C: the duplex base is C
        ss["base"][0, 3 - e, 2] = T  # column 2: C against T
    p = dict(FI.LAX, min_reads=(1,))
    assert FR.apply(ss, seq, qual, ln, st, **p)[1].sum() == 0
    filt, masked, s2, q2 = FR.apply(ss, seq, qual, ln, st, **dict(p, require_single_strand_agreement=True))
    assert filt[0] == 0 and masked.tolist() == [[2, 2]]
    assert s2[0, 0, :4].tolist() == [C, N, N, C] and q2[0, 0, :4].tolist() == [60, 2, 2, 60]
    # a one-strand family has nothing to disagree with
    case = duplex_family(4, None)
    assert FR.apply(*case, **dict(FI.LAX, require_single_strand_agreement=True))[1].sum() == 0


def test_no_call_fraction_and_mean_quality_after_masking():
    """4 columns at Q60, one masked by its error rate: 1 / 4 no-calls, quality sum 182."""
    case = duplex_family(4, 4, ae=4, be=4)
    p = dict(FI.LAX, max_base_error_rate=(0.5,))
    assert FR.apply(*case, **dict(p, max_no_call_fraction=0.25))[0][0] == 0
    assert FR.apply(*case, **dict(p, max_no_call_fraction=0.24))[0][0] == FR.NOCALL
    assert FR.apply(*case, **dict(p, min_mean_base_quality=45))[0][0] == 0       # 182 >= 45 * 4
    assert FR.apply(*case, **dict(p, min_mean_base_quality=46))[0][0] == FR.MEANQ  # 182 < 184
    # a family that is not emitted is not looked at
    ss, seq, qual, ln, st = case
    assert FR.apply(ss, seq, qual, ln, np.zeros(1, np.int32), **dict(p, max_no_call_fraction=0.0))[0][0] == 0


@pytest.mark.parametrize("name", ["c2", "molecular", "strands"])
def test_a_second_application_changes_nothing(name):
    c = FI.case(name)
    r = c.oracle
    for pn in ("typical", "agree", "q93"):
        p = FI.PARAM_SETS[pn]
        filt, masked, seq, qual = c.reference(p)
        f2, m2, s2, q2 = FR.apply(r.ss, seq, qual, r.cons_len, r.status, molecular=c.molecular, **p)
        assert np.array_equal(f2, filt) and np.array_equal(s2, seq) and np.array_equal(q2, qual), (name, pn)
        gate_ok = np.ones(len(filt), bool)  # (nothing new to mask: every masked column is N now)
        assert m2[gate_ok].sum() == 0, (name, pn)


# The sets that reach the whole ground on their input, found by trying seeds and thresholds on the
# oracle's output alone: "typical" on the main C2 input (synth seed 11, messify seed 2) and
# "molecular_typical" on the step-1 input (seed 13, messify 4).
@pytest.mark.parametrize("name,pn", [("c2", "typical"), ("molecular", "molecular_typical")])
def test_main_inputs_reach_the_ground(name, pn):
    c = FI.case(name)
    em = c.oracle.status == 1
    filt, masked, _, _ = c.reference(FI.PARAM_SETS[pn])
    for bit in (FR.MINREADS, FR.READERR, FR.NOCALL, FR.MEANQ):
        assert int(((filt & bit) != 0).sum()) >= 1, "no template dropped with reason %d" % bit
    kept = em & (filt == 0)
    assert kept.sum() >= 0.1 * em.sum(), "%d of %d kept" % (kept.sum(), em.sum())
    assert masked[kept].sum() > 0, "no kept record holds a newly masked base"
    assert (filt[~em] == 0).all()


def test_parameter_extremes_do_what_they_say():
    c = FI.case("c2")
    r = c.oracle
    em = r.status == 1
    live = np.arange(r.cons_seq.shape[2])[None, None, :] < r.cons_len[:, :, None]
    filt, masked, seq, qual = c.reference(FI.PARAM_SETS["lax"])
    assert not filt.any() and not masked.any() and np.array_equal(seq, r.cons_seq) and np.array_equal(qual, r.cons_qual)
    filt, masked, seq, qual = c.reference(FI.PARAM_SETS["q93"])
    assert not filt.any() and (seq[em][live[em]] == N).all() and (qual[em][live[em]] == 2).all()
    assert masked[em].sum() == int((live[em] & (r.cons_seq[em] != N)).sum())
    filt, _, _, _ = c.reference(FI.PARAM_SETS["q93_nocall0"])
    assert (filt[em] == FR.NOCALL).all()
    filt, masked, _, _ = c.reference(FI.PARAM_SETS["three_reads"])
    assert ((filt == 0) & em).sum() > 0 and (filt[em & (filt != 0)] == FR.MINREADS).all() and masked.sum() > 0


@pytest.mark.parametrize("name", FI.EDGE_CASES + ("c3",))
def test_edge_inputs_hold_their_edges(name):
    """What each edge input is for, and that the filter has something to decide on it: under
    "single_ok" (one-strand families pass the gate) it keeps and drops templates and masks bases."""
    c = FI.case(name)
    r = c.oracle
    em = r.status == 1
    L = r.cons_len[em]
    if name == "tiny":
        assert L.min() <= 3  # (a 1-base read gains tool 2's appended base)
    if name.startswith("stride"):
        assert int(c.raw.l_seq.max()) + 2 == int(name[6:])
    if name == "rounds":
        assert {511, 512, 513} <= set(int(x) for x in np.unique(L)) | set(int(x) - 1 for x in np.unique(L))
    if name == "strands":
        used = {"AB": ((r.ss["len"][:, 0] > 0) & (r.ss["len"][:, 3] == 0) & em).sum(),
                "BA": ((r.ss["len"][:, 0] == 0) & (r.ss["len"][:, 3] > 0) & em).sum(), "none": (~em).sum()}
        assert min(used.values()) >= 5, used
        assert (~em[1:-1] & em[:-2] & em[2:]).any()  # a family that emits nothing between two that do
    if name == "wide":
        assert int(r.ss["depth"].max()) > 255 and int(np.diff(r.fam_rec_off).max()) >= 256
    if name == "c3":
        assert int((np.diff(r.fam_rec_off) > 64).sum()) >= 40  # families past k_small's 64 records: k_large
    filt, masked, _, _ = c.reference(FI.PARAM_SETS["single_ok"])
    kept = em & (filt == 0)
    assert kept.any() and (em & (filt != 0)).any(), name
    if name not in ("wide", "c3"):
        assert masked[kept].sum() > 0, name


def test_cli_refuses_what_it_cannot_do(capsys):
    from bsseqconsensusreads_amd import cli
    from bsseqconsensusreads_amd.filter import FilterParams
    for argv in (["step5", "-r", "x.fa", "in.bam", "out.bam", "--filter-min-reads", "3"],
                 ["molecular", "in.bam", "out.bam", "--filter-max-no-call-fraction", "0.1"],
                 ["step5", "-r", "x.fa", "in.bam", "out.bam", "--gpus", "2", "--filter-min-base-quality", "10"],
                 ["step5", "-r", "x.fa", "in.bam", "out.bam", "--filter-min-base-quality", "10", "--filter-min-reads",
                  "3", "2", "1", "1"]):
        with pytest.raises(SystemExit) as e:
            cli.parse(argv)
        assert e.value.code == 2
    assert "not supported with --gpus 2 yet" in capsys.readouterr().err
    a = cli.parse(["molecular", "in.bam", "out.bam", "--filter-min-base-quality", "10", "--filter-min-reads", "3", "2"])
    assert cli.filter_params(a) == FilterParams(10, min_reads=(3, 2))
    assert cli.filter_params(cli.parse(["molecular", "in.bam", "out.bam"])) is None

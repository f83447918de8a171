"""The C++ family formation (include/bsdc_host.h, csrc/bsdc_host.cpp) against the numpy statement
of batch.plan_families / batch.materialize (plan_families_py / materialize_py): every plan array
and every device-batch array equal, on clean and messy synthetic inputs (clips, indels, hard
clips, missing MC, unmapped mates), tool-2 output (vote mode), both family orders, small_cap 0
(every family large) and family ranges."""
import numpy as np
import pytest

from bsseqconsensusreads_amd import batch, hostplan, pipeline, synth
from oracle import oracle

PLAN_KEYS = ("order", "fam_off", "fam_mi", "t2_rank", "fam_split", "conv", "ext_right", "ext_left", "rd_in",
             "partner_raw", "sL", "L", "kfirst", "kn")
BATCH_KEYS = ("fam_off", "rec_off", "fam_entry", "rec_pos", "rec_lenflag", "rec_tid", "rec_link", "rec_win", "cig_off",
              "cig_info", "cigar", "rt", "seq", "qual", "src", "fam_mi", "t2_rank")


def _same_plan(a, b):
    for k in PLAN_KEYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and np.array_equal(x.astype(np.int64), y.astype(np.int64)), k


def _same_batch(a, b):
    for k in BATCH_KEYS:
        x, y = np.asarray(getattr(a, k)), np.asarray(getattr(b, k))
        assert x.shape == y.shape, (k, x.shape, y.shape)
        assert np.array_equal(x.astype(np.int64), y.astype(np.int64)), k
    for k in ("max_len", "n_bases", "n_slots", "split_ext", "small_arenas", "large_arenas"):
        assert getattr(a, k) == getattr(b, k), k
    for k in ("small_buckets", "large_buckets"):
        xa, xb = getattr(a, k), getattr(b, k)
        assert len(xa) == len(xb), k
        for u, v in zip(xa, xb):
            assert np.array_equal(np.asarray(u).reshape(-1), np.asarray(v).reshape(-1)), k


def _check(raw, mode, ref, order="template-coordinate", small_cap=batch.SMALL_ARENA_CAP, ranges=None):
    p_py = batch.plan_families_py(raw, mode, ref, order)
    p_c = hostplan.plan_families(raw, mode, ref, order)
    _same_plan(p_c, p_py)
    for a, b in ranges or [(0, p_py.n_fam)]:
        _same_batch(hostplan.materialize(p_c, a, b, small_cap), batch.materialize_py(p_py, a, b, small_cap))
    return p_py


@pytest.mark.parametrize("cfg,messy", [("C0", 0.0), ("C2", 0.0), ("C2", 0.25), ("C4", 0.15), ("C1", 0.3)])
def test_full_mode_matches_numpy(cfg, messy):
    s = synth.generate(cfg, 300, seed=41, device="cpu", genome_len=120_000)
    raw = synth.messify(s.raw, frac=messy, seed=7) if messy else s.raw
    _check(raw, "full", s.ref)


def test_read_through_and_forced_large():
    s = synth.generate("C1", 400, seed=6, device="cpu", genome_len=200_000, frag=(140, 40, 60))
    _check(s.raw, "full", s.ref)
    _check(s.raw, "full", s.ref, small_cap=0)


def test_mi_group_order_and_ranges():
    s = synth.generate("C2", 500, seed=8, device="cpu", genome_len=150_000)
    raw = synth.messify(s.raw, frac=0.2, seed=3)
    _check(raw, "full", s.ref, order="mi-group")
    p = batch.plan_families_py(raw, "full", s.ref)
    from bsseqconsensusreads_amd import shard
    _check(raw, "full", s.ref, ranges=shard.plan_batches(p.fam_bases(), 5000))


def test_vote_mode_matches_numpy():
    s = synth.generate("C2", 400, seed=24, device="cpu", genome_len=60_000)
    res = oracle.run(s.raw, s.ref)
    raw2 = pipeline.raw_from_records(s.raw, res.tool2)
    _check(raw2, "vote", None)
    _check(raw2, "vote", None, order="mi-group")


def test_split_partner_and_missing_mi():
    s = synth.generate("C0", 400, seed=15, device="cpu", genome_len=100_000)
    raw = s.raw
    k = int(np.nonzero(raw.flag == 163)[0][7])
    raw.next_tid[k] = 1
    p = _check(raw, "full", s.ref)
    assert p.split_ext
    raw.mi_id[int(np.nonzero(raw.flag == 99)[0][3])] = -1
    with pytest.raises(batch.MissingMITag):
        hostplan.plan_families(raw, "full", s.ref)


def _one_family(n_templates):
    """One MI family of n_templates one-template pairs (99 / 147) of 1-base reads at one position."""
    from bsseqconsensusreads_amd import records as R
    n = 2 * n_templates
    r1 = np.arange(n) % 2 == 0
    z, one = np.zeros(n, np.int32), np.ones(n, np.int32)
    raw = R.RawRecords(
        flag=np.where(r1, 99, 147).astype(np.uint16), tid=z, pos=np.full(n, 50, np.int32), mapq=np.full(n, 60, np.uint8),
        l_seq=one, seq_off=np.arange(n, dtype=np.int64), seq=np.full(n, 1, np.uint8), qual=np.full(n, 30, np.uint8),
        cig_off=np.arange(n, dtype=np.int64), n_cig=one, cigar=np.full(n, (1 << 4) | R.OP_M, np.uint32), next_tid=z,
        next_pos=np.full(n, 50, np.int32), tlen=np.where(r1, 1, -1).astype(np.int32),
        name_id=(np.arange(n) // 2).astype(np.int32), names=synth._LazyNames("t"), mi_id=z, mi_strand=np.zeros(n, np.int8),
        mi_names=synth._LazyNames(""), mc_off=np.arange(n, dtype=np.int64), mc_n=one,
        mc_cigar=np.full(n, (1 << 4) | R.OP_M, np.uint32))
    return raw, R.Reference.from_codes(["chrL"], [np.full(200, 1, np.uint8)])


@pytest.mark.parametrize("native", [True, False])
def test_family_size_limit(native):
    """The link word's in-family mate index is 16 bits with 0xFFFF = none (BSDC_LINK_MATE_MASK), so
    a family holds at most BSDC_MAX_FAMILY_RECORDS = 65534 records: the largest one materializes
    with every R1's mate index right (the last one's included), one template more -- index 0xFFFF
    would read as "no mate" -- and 65,536 templates -- indices past 16 bits would overwrite the
    strand bits -- are refused by name, in the C++ planner and in the numpy statement.  No kernel
    runs."""
    plan_f = hostplan.plan_families if native else batch.plan_families_py
    mat = (lambda p: hostplan.materialize(p, 0, p.n_fam, 0)) if native else (lambda p: batch.materialize_py(p, 0, p.n_fam, 0))
    assert batch.MAX_FAMILY_RECORDS == 65534
    raw, ref = _one_family(batch.MAX_FAMILY_RECORDS // 2)
    fb = mat(plan_f(raw, "full", ref))
    assert fb.n_fam == 1 and fb.n_rec == batch.MAX_FAMILY_RECORDS
    local = np.empty(fb.n_rec, np.int64)
    local[fb.src] = np.arange(fb.n_rec)              # family-local index of each input record
    is_r1 = (fb.rec_lenflag >> 16) == 99
    mate = (fb.rec_link & batch.LINK_MATE_NONE).astype(np.int64)
    assert np.array_equal(mate[is_r1], local[fb.src[is_r1] + 1])  # R2 follows its R1 in the input
    assert (mate[~is_r1] == batch.LINK_MATE_NONE).all()
    last_r1 = int(np.nonzero(is_r1)[0][-1])
    assert last_r1 >= fb.n_rec - 2 and mate[last_r1] == local[fb.src[last_r1] + 1] < batch.LINK_MATE_NONE
    assert mate[is_r1].max() == batch.MAX_FAMILY_RECORDS - 1  # the largest index in use, below "none"
    assert ((fb.rec_link & (batch.LINK_AB | batch.LINK_BA)) == batch.LINK_AB).all()
    for n_templates in (batch.MAX_FAMILY_RECORDS // 2 + 1, 65536):
        raw, ref = _one_family(n_templates)
        with pytest.raises(ValueError, match="65534 records"):
            mat(plan_f(raw, "full", ref))


@pytest.mark.parametrize("native", [True, False])
def test_filter_slot_limit(native):
    """k_large keeps each source read's simplified cigar at a 16-bit offset into the family's
    slots -- one per M-only record, ops + 2 per complex record -- and packs the op count above it,
    so the last record's offset must stay below 65536: a family holding a complex cigar may have
    BSDC_MAX_FILTER_SLOTS = 65536 slots.  With 17-op forward records (19 slots) and plain reverse
    ones (1), 3,276 templates need 65,520 and materialize; 3,277 need 65,540 and are refused by
    name, in the C++ planner and in the numpy statement (k_small's 64 records cannot get there; a
    family without a complex cigar runs no filter and is not bounded).  No kernel runs."""
    import align_inputs as A
    plan_f = hostplan.plan_families if native else batch.plan_families_py
    mat = (lambda p: hostplan.materialize(p, 0, p.n_fam, 0)) if native else (lambda p: batch.materialize_py(p, 0, p.n_fam, 0))
    assert batch.MAX_FILTER_SLOTS == 65536
    c = A.slot_family(3276)
    fb = mat(plan_f(c.raw, "vote", c.ref))
    assert fb.n_fam == 1 and fb.n_rec == 2 * 3276
    assert int(((fb.rec_link & batch.LINK_COMPLEX) != 0).sum()) == 3276
    assert int((fb.cig_info[(fb.rec_link & batch.LINK_COMPLEX) != 0] & 0xFFFF).sum()) + 2 * 3276 + 3276 == 65520
    c = A.slot_family(3277)
    with pytest.raises(ValueError, match="65536 cigar slots"):
        mat(plan_f(c.raw, "vote", c.ref))


def test_empty_input():
    s = synth.generate("C0", 10, seed=1, device="cpu", genome_len=20_000)
    from bsseqconsensusreads_amd import records as R
    raw = R.take(s.raw, np.zeros(0, np.int64))
    p = hostplan.plan_families(raw, "full", s.ref)
    assert p.n_fam == 0
    fb = hostplan.materialize(p, 0, 0, batch.SMALL_ARENA_CAP)
    assert fb.n_rec == 0 and fb.n_fam == 0

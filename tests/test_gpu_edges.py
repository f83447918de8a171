"""The consensus kernels at the edges of the layout and of the ABI's parameter
domain (include/bsdc.h bsdc_params), on inputs built for it (tests/edge_inputs.py; the CPU side
of every case is checked in tests/test_edge_inputs.py): quality bytes over the whole byte range
(sums above the cap, the SWAR overlap's branch for sums of 128 and over, the `wild` overlap path of
families with a byte >= 128, BAM's 0xFF), family sizes on every threshold (64 | 65 records, 64 | 65
and 128 | 129 reads per set, 254 .. 258 records, a depth past a byte), reads of 1 base up, strides
beside a multiple of 16, and every flag of bsdc_params away from its default.

Every case: GPU == oracle/ bit for bit (consensus, single-strand reads and tag statistics, the
tool-2 records), then the fp64 restatement of fgbio within the fp64 bar (helpers.gpu_vs_fp64).
Routes: the default routing, every family through k_large with its arena in LDS and in HBM
("both kernels"), and k_large's part mode.  The count of single-strand qualities off by one
against fp64 is printed per case (`pytest -s`); it must be 0 at (45, 30) with qualities <= 93.
"""
import numpy as np
import pytest

import edge_inputs as E
from bsseqconsensusreads_amd import batch, pipeline
from bsseqconsensusreads_amd import records as R
from bsseqconsensusreads_amd.device import ConsensusParams, Engine
from helpers import gpu_vs_fp64
from oracle import oracle
from test_gpu_parity import assert_consensus_equal, assert_ss_equal, force_large, force_parts

pytestmark = pytest.mark.gpu

KERNELS = ["default", "lds", "global"]
_cache = {}


def case(kind, arg=None):
    """The builder's case, built once per session (the tests leave it unchanged)."""
    if (kind, arg) not in _cache:
        _cache[kind, arg] = E.params_case() if kind == "params" else {
            "quality": E.quality_case, "size": E.size_case, "length": E.length_case, "stride": E.stride_case}[kind](arg)
    return _cache[kind, arg]


def route(monkeypatch, how, cap=2800):
    """-> the list the run's device batches are collected in.  cap (part mode): the parts' LDS
    bytes; 2800 holds one template of 40-base reads and not two, so every family of two templates
    or more is cut (but tool 2's 4-groups, which cannot be)."""
    seen = []
    if how == "parts":
        force_parts(monkeypatch, cap, seen)
        return seen
    if how in ("lds", "global"):
        force_large(monkeypatch, how)
    real = batch.materialize  # (force_large's when set)

    def spy(plan, f0, f1, small_cap=None, images=None):
        fb = real(plan, f0, f1, small_cap=small_cap, images=images) if how == "default" else real(plan, f0, f1, images=images)
        seen.append(fb)
        return fb
    monkeypatch.setattr(batch, "materialize", spy)
    monkeypatch.setattr(pipeline, "materialize", spy)
    return seen


def check(engine, es, what, exact_quals=False, **kw):
    """Step 5 with the tools, dump and tags on `es`: bit-exact against oracle/ (tool-2 records
    included) and inside the fp64 bar.  exact_quals: no quality may be off by one either."""
    cons, c, t2, r = gpu_vs_fp64(engine, es.raw, es.ref, True, what, dump=True, **kw)
    for k in ("src", "pos", "seq", "qual", "cigar"):
        assert np.array_equal(getattr(t2, k), getattr(r.tool2, k)), "%s: tool-2 %s" % (what, k)
    assert 2 * int(r.status.sum()) >= len(r.status) > 0
    print("%s: single-strand qualities off by one against fp64: %d of %d columns" % (what, c["qual_pm1"], c["columns"]))
    if exact_quals:
        assert c["qual_pm1"] == 0, what
    return cons, c, r


def n_split(seen):
    return sum(int(fb.split_fams.shape[0]) for fb in seen)


# ---- qualities ---------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,how", [(s, h) for s in ("full_range", "high", "wild") for h in KERNELS] +
                         [("wild", "parts")])
def test_quality_edges(engine, monkeypatch, sampler, how):
    es = case("quality", sampler)
    E.assert_quality_edges(sampler, es.raw)
    seen = route(monkeypatch, how)
    check(engine, es, "quality %s %s" % (sampler, how), exact_quals=sampler == "full_range")
    if how == "parts":
        assert n_split(seen) > 0.5 * len(es.families), n_split(seen)
    elif how == "default":
        assert sum(int(b.shape[0]) for fb in seen for b in fb.small_buckets) > 100  # k_small ran them


# ---- family sizes --------------------------------------------------------------------------------
def _by_size(fb):
    return np.diff(fb.fam_off.astype(np.int64))


@pytest.mark.parametrize("how", KERNELS + ["parts"])
@pytest.mark.parametrize("ab_only", [False, True])
def test_family_size_edges(engine, monkeypatch, ab_only, how):
    es = case("size", ab_only)
    seen = route(monkeypatch, how, cap=16384)
    cons, c, r = check(engine, es, "sizes ab_only=%s %s" % (ab_only, how), exact_quals=True)
    sizes = np.diff(r.fam_rec_off)
    assert sorted(sizes.tolist()) == sorted(list(E.FAMILY_SIZES) * 3 + [E.DEEP_FAMILY])
    assert ((cons.status[sizes == 1] & 1) == 0).all() and ((cons.status[sizes > 1] & 1) == 1).all()
    fb = seen[0]
    assert len(seen) == 1 and np.array_equal(_by_size(fb), sizes)
    if how == "default":
        small = np.concatenate(fb.small_buckets).astype(np.int64)
        large = fb.large_fams[:, 0].astype(np.int64)
        large = np.concatenate([large, fb.split_fams[:, 0].astype(np.int64)])
        assert small.shape[0] > 0 and large.shape[0] > 0 and small.shape[0] + large.shape[0] == fb.n_fam
        assert np.isin(np.nonzero(sizes == 64)[0], small).all()    # 64 records: one wavefront, k_small
        assert np.isin(np.nonzero(sizes == 65)[0], large).all()    # 65: k_large
        assert sizes[small].max() == 64 and sizes[large].min() == 65
    if how == "parts":
        cut = fb.split_fams[:, 0].astype(np.int64)
        assert cut.shape[0] > 0 and np.isin(np.nonzero(sizes >= 254)[0], cut).all()
        per_part = fb.split_parts[:, 2] & 0xFF
        assert per_part.max() <= batch.MAX_PART_REC and per_part.min() >= 1
        # a family of more than MAX_PART_REC records is in several parts whatever the cap
        nparts = fb.split_fams[:, 5].astype(np.int64)
        assert (nparts[np.isin(cut, np.nonzero(sizes > batch.MAX_PART_REC)[0])] >= 2).all()
    # wide rows: the families of WIDE_MIN_RECORDS records or more, and only they
    wide = np.asarray(cons.ss["wide"])
    assert np.array_equal(wide >= 0, sizes >= batch.WIDE_MIN_RECORDS) and (sizes >= batch.WIDE_MIN_RECORDS).sum() == 13
    d16, _ = batch.ss_stats16(cons.ss)
    if ab_only:
        f = int(np.nonzero(sizes == E.DEEP_FAMILY)[0][0])
        assert int(d16[f].max()) > 255 and int(d16[f].max()) == int(r.ss["depth"][f].max())
        assert int(np.asarray(cons.ss["depth"])[f].max()) == 255  # (the byte saturates)
        # 255 records, below the wide rows: the kernels' bytes alone are the exact depths and errors
        for f in np.nonzero(sizes == 255)[0]:
            assert wide[f] < 0
            for k in ("depth", "err"):
                got = np.asarray(cons.ss[k])
                assert got.dtype == np.uint8
                for s_ in range(4):
                    n = int(r.ss["len"][f, s_])
                    assert np.array_equal(got[f, s_, :n].astype(np.int64), r.ss[k][f, s_, :n]), (k, f, s_)
            assert 64 < int(np.asarray(cons.ss["depth"])[f].max()) <= 128


# ---- read lengths --------------------------------------------------------------------------------
@pytest.mark.parametrize("how", KERNELS)
@pytest.mark.parametrize("name", list(E.LENGTH_SETS) + ["mixed"])
def test_read_length_edges(engine, monkeypatch, name, how):
    es = case("length", name)
    route(monkeypatch, how)
    cons, c, r = check(engine, es, "lengths %s %s" % (name, how), exact_quals=True)
    if name == "tiny":  # converted 1-base records whose RD trim leaves tool 1's prepended base alone
        t1 = r.tool1
        assert int(((es.raw.l_seq[t1.src] == 1) & (t1.rd == 1) & (t1.l_seq == 1)).sum()) >= 1
    assert cons.seq.shape[2] == batch.round16(int(es.raw.l_seq.max()) + 2)


@pytest.mark.parametrize("how", KERNELS)
@pytest.mark.parametrize("arg", [15, 16, 17, 31, 32, 33])
def test_stride_edges(engine, monkeypatch, arg, how):
    """max_len + 2 == arg: the output stride is round16 of it (16 | 16 | 32, 32 | 32 | 48)."""
    es = case("stride", arg)
    assert int(es.raw.l_seq.max()) + 2 == arg
    seen = route(monkeypatch, how)
    cons, c, r = check(engine, es, "max_len + 2 = %d %s" % (arg, how), exact_quals=True)
    want = {15: 16, 16: 16, 17: 32, 31: 32, 32: 32, 33: 48}[arg]
    assert want == batch.round16(arg) == seen[0].stride == cons.seq.shape[2] == cons.ss["base"].shape[2]


# ---- parameters (one engine, Engine.flags / bsdc_ctx_set_params) ---------------------------------
@pytest.mark.parametrize("how", KERNELS + ["parts"])
def test_overlap_off(engine, monkeypatch, how):
    es = case("params")
    seen = route(monkeypatch, how)
    cons, c, r = check(engine, es, "overlap off %s" % how, overlap=False)
    if how == "parts":
        assert n_split(seen) > 100
    on = _cache.setdefault("params-on", oracle.run(es.raw, es.ref))
    assert np.array_equal(cons.length, on.cons_len)
    w = min(cons.seq.shape[2], on.cons_seq.shape[2])
    assert int(((cons.seq[:, :, :w] != on.cons_seq[:, :, :w]) | (cons.qual[:, :, :w] != on.cons_qual[:, :, :w])).sum()) > 100
    if how == "default":  # and against the GPU's own overlap-on result
        g, _ = pipeline.run_step5(engine, es.raw)
        assert_consensus_equal(g, on, "overlap on")
    assert engine.params == ConsensusParams()


@pytest.mark.parametrize("how", KERNELS + ["parts"])
@pytest.mark.parametrize("pre,post", E.RATES_ACCEPTED)
def test_error_rates(engine, monkeypatch, pre, post, how):
    es = case("params")
    seen = route(monkeypatch, how)
    cons, c, r = check(engine, es, "rates (%g, %g) %s" % (pre, post, how), pre=pre, post=post,
                       exact_quals=(pre, post) == (45.0, 30.0))
    if how == "parts":
        assert n_split(seen) > 100
    live = np.arange(cons.ss["qual"].shape[2])[None, None, :] < cons.ss["len"][:, :, None]
    assert int(cons.ss["qual"][live & ((cons.status & 1) != 0)[:, None, None]].max()) == int(pre)
    assert engine.params == ConsensusParams()


def test_refused_params_leave_the_engine_as_it_was(engine):
    """Rates whose consensus qualities pass the agreement table (pre >= 46.999: the oracle's
    single-strand reads reach Q47 and more at (60, 40)), and a min_input_base_quality no kernel
    reads: bsdc_ctx_set_params and bsdc_ctx_create refuse them by name, and the context goes on
    with its own tables."""
    es = case("params")
    engine.load_reference(es.ref)
    before, _ = pipeline.run_step5(engine, es.raw, tags=True)
    for pre, post in E.RATES_REFUSED:
        r = oracle.run(es.raw, es.ref, pre=pre, post=post)
        live = np.arange(r.ss["qual"].shape[2])[None, None, :] < r.ss["len"][:, :, None]
        assert int((live & (r.ss["qual"] >= 47)).sum()) > 1000
        with pytest.raises(RuntimeError, match="error_rate_pre_umi"):
            with engine.flags(error_rate_pre_umi=pre, error_rate_post_umi=post):
                pass
        with pytest.raises(RuntimeError, match="bsdc_ctx_create failed"):
            Engine(0, ConsensusParams(error_rate_pre_umi=pre, error_rate_post_umi=post))
    with pytest.raises(RuntimeError, match="min_input_base_quality: only 0 is supported"):
        with engine.flags(min_input_base_quality=10):
            pass
    with pytest.raises(RuntimeError, match="bsdc_ctx_create failed"):
        Engine(0, ConsensusParams(min_input_base_quality=10))
    assert engine.params == ConsensusParams()
    after, _ = pipeline.run_step5(engine, es.raw, tags=True)
    assert after.seq.tobytes() == before.seq.tobytes() and after.qual.tobytes() == before.qual.tobytes()
    assert_consensus_equal(after, oracle.run(es.raw, es.ref), "after refused params")


@pytest.mark.parametrize("caller", ["duplex", "molecular"])
@pytest.mark.parametrize("min_cbq", [0, 2, 10, 40, 94])
def test_min_consensus_base_quality_values(engine, caller, min_cbq):
    es = case("params")
    raw = es.raw
    if caller == "molecular":
        raw = R.take(raw, np.lexsort((raw.mi_strand, raw.mi_id)))
    what = "min_cbq %d %s" % (min_cbq, caller)
    cons, c, _, r = gpu_vs_fp64(engine, raw, es.ref, caller == "duplex", what, molecular=caller == "molecular",
                                min_cbq=min_cbq, dump=caller == "duplex")
    print("%s: single-strand qualities off by one against fp64: %d of %d columns" % (what, c["qual_pm1"], c["columns"]))
    assert c["qual_pm1"] == 0
    em = (cons.status & 1) != 0
    assert 2 * int(em.sum()) >= em.shape[0]
    live = (np.arange(cons.ss["qual"].shape[2])[None, None, :] < cons.ss["len"][:, :, None]) & em[:, None, None]
    masked = live & (cons.ss["base"] == 15) & (cons.ss["qual"] == 2)
    if min_cbq == 94:  # every single-strand column is (N, 2), and so every consensus column
        assert masked.sum() == live.sum() > 10000
        cl = np.arange(cons.seq.shape[2])[None, None, :] < cons.length[:, :, None]
        assert (cons.seq[cl] == 15).all() and (cons.qual[cl] == 2).all()
    else:
        assert (cons.ss["qual"][live & ~masked] >= min_cbq).all()
        assert masked.sum() < live.sum()
    assert engine.params == ConsensusParams()


def test_switching_rates_on_one_context(engine):
    """(45, 30), then (30, 20), then (45, 30) again on one context: bsdc_ctx_set_params rebuilds
    the tables each time, the first and third results are the same bytes, and the engine's own
    params are back after the block."""
    es = case("params")
    engine.load_reference(es.ref)
    own = engine.params
    outs = []
    for pre, post in ((45.0, 30.0), (30.0, 20.0), (45.0, 30.0)):
        with engine.flags(error_rate_pre_umi=pre, error_rate_post_umi=post):
            assert engine.params.error_rate_pre_umi == pre and engine.params.error_rate_post_umi == post
            cons, t2 = pipeline.run_step5(engine, es.raw, dump=True, tags=True)
        assert engine.params == own == ConsensusParams()
        r = oracle.run(es.raw, es.ref, pre=pre, post=post)
        assert_consensus_equal(cons, r, "switch (%g, %g)" % (pre, post))
        assert_ss_equal(cons, r, "switch (%g, %g)" % (pre, post))
        outs.append(cons)
    a, b, c = outs
    for k in ("status", "length", "seq", "qual"):
        assert getattr(a, k).tobytes() == getattr(c, k).tobytes(), k
    for k in ("len", "base", "qual", "depth", "err"):
        assert np.asarray(a.ss[k]).tobytes() == np.asarray(c.ss[k]).tobytes(), k
    assert a.qual.tobytes() != b.qual.tobytes()

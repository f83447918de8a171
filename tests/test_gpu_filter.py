"""bsdc_filter (fgbio FilterConsensusReads on the device) against the numpy
restatement tests/filter_ref.py applied to oracle/'s consensus: filt, masked and the masked
seq / qual bit for bit, on the inputs and parameter sets of tests/filter_inputs.py (whose ground
test_filter_ref.py checks on the CPU), through Engine.filter, the pipeline calls and the CLI."""
import ctypes as C
import gzip

import numpy as np
import pytest
import torch

import filter_inputs as FI
import filter_ref as FR
from bsseqconsensusreads_amd import bam, batch, cli, pipeline
from bsseqconsensusreads_amd import records as R
from bsseqconsensusreads_amd.filter import FilterParams

pytestmark = pytest.mark.gpu

_RUNS = {}  # case name -> its batch on the device after the vote, with pristine copies of seq / qual


def _voted(engine, name):
    """The case's families voted once with the tags' rows on the device (one batch), unfiltered
    parity with oracle/ asserted; later calls restore seq / qual and filter again."""
    if name not in _RUNS:
        c = FI.case(name)
        r = c.oracle
        if c.molecular:
            plan = pipeline.plan_families(pipeline.molecular_records(c.raw), "vote", family_order="mi-group")
            mode, flags = pipeline.MODE_VOTE, dict(min_consensus_base_quality=0)
        else:
            engine.load_reference(c.ref)
            plan = pipeline.plan_families(c.raw, "full", engine.ref)
            assert not plan.split_ext
            mode, flags = pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE, {}
        fb = batch.materialize(plan, 0, plan.n_fam)
        db = engine.upload(fb, tags=True, filt=True)
        with engine.flags(**flags):
            engine.run(db, mode | pipeline.MODE_TAGS)
        out = db.fetch()
        assert "filt" in out and not out["filt"].any()  # (zeroed, the filter has not run)
        seq = bam.unpack_nibbles(out["seq"])
        assert np.array_equal((out["status"] & 1).astype(np.int32), r.status) and np.array_equal(out["len"], r.cons_len)
        w = min(r.cons_seq.shape[2], db.stride)  # (either stride holds every read)
        live = (np.arange(w)[None, None, :] < r.cons_len[:, :, None]) & (r.status == 1)[:, None, None]
        assert np.array_equal(seq[:, :, :w][live], r.cons_seq[:, :, :w][live])
        assert np.array_equal(out["qual"][:, :, :w][live], r.cons_qual[:, :, :w][live])
        d16, e16 = batch.ss_stats16({"depth": out["ss_depth"], "err": out["ss_err"], "wide": out["ss_wide"],
                                     "wdepth": out["ss_wdepth"], "werr": out["ss_werr"]})
        em = r.status == 1
        assert np.array_equal(d16[em][:, :, :w], r.ss["depth"][em][:, :, :w])
        assert np.array_equal(e16[em][:, :, :w], r.ss["err"][em][:, :, :w])
        _RUNS[name] = (db, db.seq.clone(), db.qual.clone(), live, w)
    return _RUNS[name]


def _check(engine, name, pn):
    c = FI.case(name)
    p = FI.PARAM_SETS[pn]
    db, seq0, qual0, live, w = _voted(engine, name)
    db.seq.copy_(seq0)
    db.qual.copy_(qual0)
    db.filt.fill_(0xAA)  # (the kernel writes every family's entry, kept and not emitted included)
    db.masked.fill_(-1)
    engine.filter(db, FI.filter_params(p), molecular=c.molecular)
    out = db.fetch(ss=False)
    assert "ss_len" not in out and "ss_base" not in out
    filt, masked, seq, qual = c.reference(p)
    what = "%s / %s" % (name, pn)
    bad = np.nonzero(out["filt"] != filt)[0]
    assert bad.size == 0, "%s: filt differs at families %s: gpu %s ref %s" % (what, bad[:8], out["filt"][bad[:8]], filt[bad[:8]])
    assert np.array_equal(out["masked"], masked), what + ": masked counts"
    got = bam.unpack_nibbles(out["seq"])[:, :, :w]
    assert np.array_equal(got[live], seq[:, :, :w][live]), what + ": masked bases"
    assert np.array_equal(out["qual"][:, :, :w][live], qual[:, :, :w][live]), what + ": masked qualities"
    return filt, masked


@pytest.mark.parametrize("pn", sorted(FI.PARAM_SETS))
def test_main_c2_families_every_parameter_set(engine, pn):
    """~2,000 messy C2 families (k_small's rows)."""
    if pn != "molecular_typical":
        _check(engine, "c2", pn)


@pytest.mark.parametrize("pn", sorted(FI.PARAM_SETS))
def test_molecular_records_every_parameter_set(engine, pn):
    """Step-1 records: one strand per end, the molecular rules."""
    _check(engine, "molecular", pn)


@pytest.mark.parametrize("name", ("c3",) + FI.EDGE_CASES)
def test_edge_inputs(engine, name):
    """k_large's rows (c3), reads of 1 base, max_len + 2 on and beside a multiple of 16, consensus
    lengths around the 512-column round, one-strand and unemitted families interleaved, a wide row."""
    for pn in ("single_ok", "typical", "three_reads", "fgbio_defaults", "agree", "q93", "base_rate0", "lax"):
        _check(engine, name, pn)


def _tiny(engine):
    c = FI.case("stride48")
    engine.load_reference(c.ref)
    return c


def test_without_a_filter_nothing_changes(engine):
    """No filter=: fetch has no new keys, Consensus.filt is None, and the bytes are the parent's
    (oracle/'s, bit for bit: tests/test_gpu_parity.py), whether or not the batch holds the filter's
    buffers."""
    c = _tiny(engine)
    plan = pipeline.plan_families(c.raw, "full", engine.ref)
    fb = batch.materialize(plan, 0, plan.n_fam)
    mode = pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE
    outs = []
    for filt in (False, True):
        db = engine.upload(fb, tags=True, filt=filt)
        engine.run(db, mode | pipeline.MODE_TAGS)
        outs.append(db.fetch())
    assert "filt" not in outs[0] and "masked" not in outs[0]
    assert set(outs[1]) - set(outs[0]) == {"filt", "masked"}
    for k in outs[0]:
        assert np.array_equal(np.asarray(outs[0][k]), np.asarray(outs[1][k])), k
    cons, _ = pipeline.run_step5(engine, c.raw, tags=True)
    assert cons.filt is None and cons.masked is None
    from test_gpu_parity import assert_consensus_equal, assert_ss_equal
    assert_consensus_equal(cons, c.oracle, "unfiltered")
    assert_ss_equal(cons, c.oracle, "unfiltered")


BAD = [("min_reads", dict(min_reads=(-1,))), ("min_reads", dict(min_reads=(1, 2, 2))), ("min_reads", dict(min_reads=(3, 1, 2))),
       ("max_read_error_rate", dict(max_read_error_rate=(0.1, 1.5))), ("max_read_error_rate", dict(max_read_error_rate=(-0.1,))),
       ("max_base_error_rate", dict(max_base_error_rate=(float("nan"),))), ("min_base_quality", dict(min_base_quality=94)),
       ("min_base_quality", dict(min_base_quality=-1)), ("max_no_call_fraction", dict(max_no_call_fraction=1.01)),
       ("min_mean_base_quality", dict(min_mean_base_quality=94))]


def test_refused_parameters_name_the_field(engine):
    c = _tiny(engine)
    plan = pipeline.plan_families(c.raw, "full", engine.ref)
    fb = batch.materialize(plan, 0, plan.n_fam)
    db = engine.upload(fb, filt=True)
    engine.run(db, pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE | pipeline.MODE_TAGS)
    before = db.fetch(ss=False)
    for field, kw in BAD:
        p = dict(FI.PARAM_SETS["fgbio_defaults"], **kw)
        with pytest.raises(RuntimeError, match=r"bsdc_filter failed \(-22\).*" + field):
            engine.filter(db, FI.filter_params(p))
    with pytest.raises(ValueError, match="one to three"):
        FilterParams(10, min_reads=(3, 2, 1, 1)).c_struct()
    after = db.fetch(ss=False)
    for k in ("seq", "qual", "filt", "masked"):
        assert np.array_equal(before[k], after[k]), k
    # a batch run without the tags' rows: BSDC_EINVAL
    plain = engine.upload(fb)
    engine.run(plain, pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE)
    with pytest.raises(ValueError):
        engine.filter(plain, FilterParams(10))
    fp = FilterParams(10).c_struct()
    rc = engine.lib.bsdc_filter(engine.ctx, C.byref(fp), 0, plain.n_fam, C.byref(plain._o), C.c_void_p(db.filt.data_ptr()),
                                C.c_void_p(db.masked.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -22 and b"ss_" in engine.lib.bsdc_last_error(engine.ctx)


def test_pipeline_calls_filter_every_batch(engine):
    """run_step5 / run_molecular with filter=, the stream cut into several device batches: the
    concatenated filt / masked / seq / qual are the one-batch reference's; without tags=True no
    single-strand rows come back."""
    c = FI.case("c2")
    engine.load_reference(c.ref)
    p = FI.PARAM_SETS["typical"]
    filt, masked, seq, qual = c.reference(p)
    _, _, _, live, w = _voted(engine, "c2")
    for tags in (False, True):
        cons, _ = pipeline.run_step5(engine, c.raw, tags=tags, batch_bases=400_000, filter=FI.filter_params(p))
        assert (cons.ss is not None) == tags
        assert np.array_equal(cons.filt, filt) and np.array_equal(cons.masked, masked)
        assert np.array_equal(cons.seq[:, :, :w][live], seq[:, :, :w][live])
        assert np.array_equal(cons.qual[:, :, :w][live], qual[:, :, :w][live])
    m = FI.case("molecular")
    p = FI.PARAM_SETS["molecular_typical"]
    filt, masked, seq, qual = m.reference(p)
    cons, _ = pipeline.run_molecular(engine, m.raw, filter=FI.filter_params(p))
    assert cons.ss is None and np.array_equal(cons.filt, filt) and np.array_equal(cons.masked, masked)
    assert engine.params.min_consensus_base_quality == 2


# ---- end to end: the CLI on files ---------------------------------------------------------------
def _flags(p):
    a = ["--filter-min-base-quality", str(p["min_base_quality"]), "--filter-min-reads"] + [str(x) for x in p["min_reads"]]
    a += ["--filter-max-read-error-rate"] + [repr(x) for x in p["max_read_error_rate"]]
    a += ["--filter-max-base-error-rate"] + [repr(x) for x in p["max_base_error_rate"]]
    a += ["--filter-max-no-call-fraction", repr(p["max_no_call_fraction"])]
    if p["min_mean_base_quality"] >= 0:
        a += ["--filter-min-mean-base-quality", str(p["min_mean_base_quality"])]
    return a + ["--filter-require-single-strand-agreement", "true" if p["require_single_strand_agreement"] else "false"]


def _fastq_text(names, seqs, quals, which):
    return "".join("@%s/%d\n%s\n+\n%s\n" % (n.decode(), which, R.NT16_TO_ASCII[s].tobytes().decode(),
                                            (q + 33).astype(np.uint8).tobytes().decode())
                   for n, s, q in zip(names, seqs, quals))


def _check_files(tmp_path, cmd, inp, extra, r, pset, reference, capsys):
    """cmd = "step5" / "molecular" on `inp` with the filter flags of the set `pset`, `reference` =
    filter_ref's answer for it on oracle/'s consensus r: --stream true
    and false write the same bytes; the records are the unfiltered run's minus the dropped
    templates, SEQ / QUAL as filter_ref says, tags as the unfiltered run's; the FASTQ pair is the
    text of those records; without per-base tags, the same SEQ / QUAL and no consensus tags."""
    filt, masked, seq, qual = reference
    em = np.nonzero(r.status == 1)[0]
    kept = np.nonzero((r.status == 1) & (filt == 0))[0]
    assert 0 < kept.size < em.size
    p = lambda n: str(tmp_path / n)
    assert cli.main([cmd] + extra + [inp, p("plain.bam"), "--stream", "false", "--threads", "4"]) == 0
    fl = _flags(pset)
    for mode in ("true", "false"):
        assert cli.main([cmd] + extra + [inp, p("f_%s.bam" % mode), "--stream", mode, "--threads", "4", "--fastq1",
                                         p("f_%s_1.fq.gz" % mode), "--fastq2", p("f_%s_2.fq.gz" % mode)] + fl) == 0
        info = capsys.readouterr().err.strip().splitlines()[-1]
        assert '"filter"' in info and '"kept": %d' % kept.size in info and '"templates": %d' % em.size in info
    for n in ("f_%s.bam", "f_%s_1.fq.gz", "f_%s_2.fq.gz"):
        assert open(p(n % "true"), "rb").read() == open(p(n % "false"), "rb").read(), n
    assert cli.main([cmd] + extra + [inp, p("notags.bam"), "--stream", "true", "--threads", "4",
                                     "--output-per-base-tags", "false"] + fl) == 0
    _, plain = bam.read_bam(p("plain.bam"))
    _, got = bam.read_bam(p("f_true.bam"))
    _, bare = bam.read_bam(p("notags.bam"))
    assert plain.n == 2 * em.size and got.n == bare.n == plain.n - 2 * (em.size - kept.size)
    pa, ga, ba = bam._aux_table(plain), bam._aux_table(got), bam._aux_table(bare)
    where = {int(f): j for j, f in enumerate(em)}
    names, seqs, quals = [], ([], []), ([], [])
    for j, f in enumerate(kept):
        for e in range(2):
            k, k0, L = 2 * j + e, 2 * where[int(f)] + e, int(r.cons_len[f, e])
            assert got.qname(k) == plain.qname(k0) == bare.qname(k)
            assert np.array_equal(got.record_seq(k), seq[f, e, :L]) and np.array_equal(got.record_qual(k), qual[f, e, :L])
            assert np.array_equal(bare.record_seq(k), seq[f, e, :L]) and np.array_equal(bare.record_qual(k), qual[f, e, :L])
            assert bytes(ga[k]) == bytes(pa[k0])  # the consensus tags are the unfiltered read's
            assert len(ba[k]) < len(ga[k]) and bytes(ga[k]).startswith(bytes(ba[k])) and b"cD" not in bytes(ba[k])
            seqs[e].append(seq[f, e, :L])
            quals[e].append(qual[f, e, :L])
        names.append(got.qname(2 * j))
    assert masked[kept].sum() > 0
    for e in range(2):
        with gzip.open(p("f_true_%d.fq.gz" % (e + 1)), "rt") as fh:
            assert fh.read() == _fastq_text(names, seqs[e], quals[e], e + 1)


def test_cli_step5_filtered_outputs(tmp_path, capsys):
    from oracle import oracle
    from test_gpu_stream import _inputs
    inp, fa = _inputs(tmp_path, "C2", 400, 0.1, 23)
    _, whole = bam.read_bam(inp, threads=4)
    r = oracle.run(whole, bam.read_fasta(fa, bam.read_bam_header(inp)), threads=8)
    ref = FR.apply(r.ss, r.cons_seq, r.cons_qual, r.cons_len, r.status, **FI.PARAM_SETS["typical"])
    _check_files(tmp_path, "step5", inp, ["--reference", fa], r, FI.PARAM_SETS["typical"], ref, capsys)


def test_cli_molecular_filtered_outputs(tmp_path, capsys):
    import types

    from oracle import oracle
    from test_molecular_stream import grouped_bam
    _, inp = grouped_bam(tmp_path, n_fam=300, messy=0.1, seed=19)
    _, whole = bam.read_bam(inp, threads=4)
    r = oracle.run(pipeline.molecular_records(whole), types.SimpleNamespace(names=[], contig_off=[], contig_len=[], letters={}),
                   threads=4, run_tools=False, family_order="mi-group", min_consensus_base_quality=0)
    ref = FR.apply(r.ss, r.cons_seq, r.cons_qual, r.cons_len, r.status, molecular=True, **FI.PARAM_SETS["molecular_typical"])
    _check_files(tmp_path, "molecular", inp, [], r, FI.PARAM_SETS["molecular_typical"], ref, capsys)

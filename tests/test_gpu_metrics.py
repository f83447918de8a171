"""bsdc_metrics / bsdc_metrics_filter (the per-run consensus metrics reduced on the device, DESIGN.md
3.9 / 8.10): the kernel against its host twin, counter for counter, on the fabricated rows of
tests/metrics_inputs.py; against the numpy restatement tests/metrics_ref.py on voted batches
(oracle/'s rows); that launches accumulate and repeat bit for bit; the filter's counters; and the CLI's
--metrics, whose JSON does not depend on where the outputs are made and which changes no output byte."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import filter_inputs as FI
import metrics_inputs as MI
import metrics_ref as MR
from bsseqconsensusreads_amd import _lib, batch, cli, metrics, pipeline
from test_metrics_host import assert_words, twin

pytestmark = pytest.mark.gpu


def _device_rows(engine, x):
    """The set's arrays in HBM, exactly their sizes -> (ConsensusC, tensors kept alive, n_wide)."""
    dev = engine.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    t = {"status": up(x.status.astype(np.uint8)), "len": up(x.length.astype(np.uint16)), "seq": up(x.seq),
         "qual": up(x.qual), "ss_len": up(x.ss_len.astype(np.uint16)), "ss_base": up(x.ss_base), "ss_qual": up(x.ss_qual),
         "ss_depth": up(x.ss_depth), "ss_err": up(x.ss_err)}
    W = int(x.ss_wdepth.shape[0])
    if x.ss_wide is not None:
        t["ss_wide"] = up(x.ss_wide.astype(np.int32))
        if W:
            t["ss_wdepth"], t["ss_werr"] = up(x.ss_wdepth.astype(np.uint16)), up(x.ss_werr.astype(np.uint16))
    o = _lib.ConsensusC()
    o.stride = x.stride
    for k, v in t.items():
        setattr(o, k, int(v.data_ptr()))
    return o, t, W


def _kernel(engine, x, acc=None, times=1):
    o, keep, W = _device_rows(engine, x)
    n = metrics.words(x.cycles)
    acc = torch.zeros(n, dtype=torch.int64, device=engine.device) if acc is None else acc
    s = torch.cuda.current_stream(engine.device)
    for _ in range(times):
        rc = engine.lib.bsdc_metrics(engine.ctx, C.byref(o), x.n_fam, W, x.kind, x.cycles, C.c_void_p(int(acc.data_ptr())),
                                     C.c_void_p(s.cuda_stream))
        assert rc == 0, engine.lib.bsdc_last_error(engine.ctx).decode()
    s.synchronize()
    del keep
    return acc


def _words(acc):
    return acc.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", MI.NAMES)
def test_kernel_equals_the_twin_on_fabricated_rows(engine, name):
    x = MI.make(name)
    got = _words(_kernel(engine, x))
    assert_words(got, twin(x), x.cycles, name + " (kernel / twin)")
    assert_words(got, MI.reference(name), x.cycles, name + " (kernel / restatement)")


def test_launches_accumulate_and_repeat(engine):
    x, y = MI.make("s32_f300"), MI.make("s16_f3100")
    acc = _kernel(engine, x)
    _kernel(engine, y, acc)
    assert_words(_words(acc), np.asarray(MI.reference("s32_f300")) + np.asarray(MI.reference("s16_f3100")), 512, "sum")
    twice = _words(_kernel(engine, x, times=2))
    assert_words(twice, 2 * np.asarray(MI.reference("s32_f300")), 512, "two launches")
    for name in ("s528_f65", "s16_f3100", "edges"):  # two identical runs: identical words
        a, b = _words(_kernel(engine, MI.make(name))), _words(_kernel(engine, MI.make(name)))
        assert a.tobytes() == b.tobytes(), name


def test_launcher_refusals(engine):
    x = MI.make("s16_f3")
    o, keep, W = _device_rows(engine, x)
    acc = torch.zeros(metrics.words(512), dtype=torch.int64, device=engine.device)
    call = lambda o, cycles=512, a=acc: engine.lib.bsdc_metrics(  # noqa: E731
        engine.ctx, C.byref(o), x.n_fam, W, 0, cycles, C.c_void_p(int(a.data_ptr())) if a is not None else None, None)
    for k in ("status", "len", "seq", "qual", "ss_len", "ss_base", "ss_qual", "ss_depth", "ss_err"):
        old = getattr(o, k)
        setattr(o, k, None)
        assert call(o) == -22 and k + " is null" in engine.lib.bsdc_last_error(engine.ctx).decode()
        setattr(o, k, old)
    assert call(o, cycles=1) == -22 and "cycles" in engine.lib.bsdc_last_error(engine.ctx).decode()
    o.stride = 24
    assert call(o) == -22 and "stride" in engine.lib.bsdc_last_error(engine.ctx).decode()
    o.stride = x.stride
    assert call(o, a=None) == -22
    torch.cuda.synchronize()
    assert not _words(acc).any()  # nothing was enqueued
    engine._metrics = None
    with pytest.raises(ValueError, match="metrics_begin"):
        engine.metrics_fetch()


def _voted_metrics(engine, name, flt=None):
    """The case voted through pipeline.run_batches with metrics on -> (the accumulator's words, Consensus)."""
    c = FI.case(name)
    if c.molecular:
        plan = pipeline.plan_families(pipeline.molecular_records(c.raw), "vote", family_order="mi-group")
        mode, flags = pipeline.MODE_VOTE, dict(min_consensus_base_quality=0)
    else:
        engine.load_reference(c.ref)
        plan = pipeline.plan_families(c.raw, "full", engine.ref)
        assert not plan.split_ext
        mode, flags = pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE, {}
    n = plan.n_fam
    fbs = [batch.materialize(plan, a, b) for a, b in ((0, n // 3), (n // 3, n))]  # two batches, one accumulator
    engine.metrics_begin(512)
    with engine.flags(**flags):
        parts = pipeline.run_batches(engine, fbs, mode, False, None, flt, c.molecular, metrics=True)
    assert all(p.ss is None for p in parts)  # (the rows stayed in HBM)
    return engine.metrics_fetch(), pipeline.concat_consensus(parts)


@pytest.mark.parametrize("name", ["c2", "c3", "wide", "molecular"])
def test_voted_batches_equal_the_restatement(engine, name):
    """~2,000 C2 families (k_small's rows), ~60 C3 (k_large's), a wide-row family, step-1 records"""
    c = FI.case(name)
    r = c.oracle
    got, cons = _voted_metrics(engine, name)
    want = MR.words(MR.run(r.ss, r.cons_seq, r.cons_qual, r.cons_len, r.status, molecular=c.molecular))
    assert_words(got, want, 512, name)
    assert got[metrics.SKIPPED] == 0 and got[metrics.RECORDS] == 2 * int((cons.status & 1).sum()) > 0


@pytest.mark.parametrize("name,pn", [("c2", "typical"), ("molecular", "molecular_typical"), ("c3", "typical")])
def test_filter_counters_and_unfiltered_histograms(engine, name, pn):
    c = FI.case(name)
    r = c.oracle
    p = FI.PARAM_SETS[pn]
    filt, masked, _, _ = c.reference(p)
    got, cons = _voted_metrics(engine, name, FI.filter_params(p))
    assert np.array_equal(cons.filt, filt) and filt.any()
    want = MR.words(MR.run(r.ss, r.cons_seq, r.cons_qual, r.cons_len, r.status, molecular=c.molecular, filt=filt,
                           masked=masked))
    assert_words(got, want, 512, "%s / %s" % (name, pn))
    plain, _ = _voted_metrics(engine, name)
    assert np.array_equal(got[16:], plain[16:]) and np.array_equal(got[:4], plain[:4]) and not plain[4:16].any()
    assert got[metrics.MASKED] == int(masked[(r.status & 1) != 0].sum())
    assert name == "c3" or got[metrics.MASKED] > 0  # (the C3 set drops every template at the gate: nothing masked)


def test_cli_metrics_json_and_unchanged_outputs(tmp_path, capsys):
    from oracle import oracle
    from test_gpu_stream import _inputs
    from bsseqconsensusreads_amd import bam
    inp, fa = _inputs(tmp_path, "C2", 400, 0.1, 23)
    _, whole = bam.read_bam(inp, threads=4)
    r = oracle.run(whole, bam.read_fasta(fa, bam.read_bam_header(inp)), threads=8)
    p = lambda n: str(tmp_path / n)  # noqa: E731
    base = ["step5", "--reference", fa, inp]
    tail = ["--threads", "4", "--stream", "true"]
    outs = lambda t: [p(t + ".bam"), "--fastq1", p(t + "_1.fq.gz"), "--fastq2", p(t + "_2.fq.gz")]  # noqa: E731
    gpu = ["--gpu-bam", "true", "--gpu-fastq", "true", "--gpu-image", "true"]
    assert cli.main(base + outs("plain") + tail) == 0
    assert cli.main(base + outs("m") + tail + ["--metrics", p("m.json")]) == 0
    assert cli.main(base + outs("gplain") + tail + gpu) == 0
    assert cli.main(base + outs("g") + tail + gpu + ["--metrics", p("g.json")]) == 0
    assert cli.main(base + outs("w") + ["--threads", "4", "--stream", "false", "--metrics", p("w.json")]) == 0
    assert cli.main(base + ["-", "--fastq1", p("q_1.fq.gz"), "--fastq2", p("q_2.fq.gz")] + tail + [
        "--metrics", p("q.json"), "--output-per-base-tags", "false", "--metrics-cycles", "64"]) == 0
    capsys.readouterr()
    for a, b in (("plain", "m"), ("gplain", "g"), ("plain", "w")):
        for n in ("%s.bam", "%s_1.fq.gz", "%s_2.fq.gz"):
            assert open(p(n % a), "rb").read() == open(p(n % b), "rb").read(), (a, b, n)
    assert open(p("q_1.fq.gz"), "rb").read() == open(p("plain_1.fq.gz"), "rb").read()
    m, g, w = (open(p(n + ".json")).read() for n in "mgw")
    assert m == g == w
    doc = json.loads(m)
    want = metrics.report(MR.words(MR.run(r.ss, r.cons_seq, r.cons_qual, r.cons_len, r.status)), 512, doc["params"])
    assert doc == json.loads(json.dumps(want))
    assert doc["params"]["mode"] == "duplex" and doc["params"]["filter"] is None
    assert doc["counts"]["families_emitted"] == int((r.status & 1).sum()) and doc["counts"]["families_skipped"] == 0
    q = json.loads(open(p("q.json")).read())
    assert q["cycles"] == 64 and q["depth_hist"] == doc["depth_hist"] and q["qual_hist"] == doc["qual_hist"]
    assert len(q["by_cycle"]["r1"]) == 64 and q["by_cycle"]["r1"][:63] == doc["by_cycle"]["r1"][:63]
    with pytest.raises(SystemExit):
        cli.main(base + outs("x") + ["--metrics", p("x.json"), "--gpus", "2"])
    assert "--metrics" in capsys.readouterr().err

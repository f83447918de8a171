"""The metrics reduction's host twin (bsdc_metrics_host / bsdc_metrics_filter_host, csrc/bsdc_metrics.hip;
DESIGN.md 3.9) against the numpy restatement tests/metrics_ref.py, word for word: on the fabricated
rows of tests/metrics_inputs.py and on oracle/'s consensus of a C2 and a C3 input; its refusals; that
calls accumulate; the JSON document; the CLI's refusals; and the twin under the sanitizers as a
stand-alone program.  No GPU: test_gpu_metrics.py runs the same sets through the kernel."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import filter_inputs as FI
import filter_ref as FR
import metrics_inputs as MI
import metrics_ref as MR
from bsseqconsensusreads_amd import _lib, cli, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def twin(x, acc=None):
    acc = np.zeros(metrics.words(x.cycles), np.uint64) if acc is None else acc
    metrics.host(acc, x.cycles, x.status, x.length, x.seq, x.qual, x.ss_len, x.ss_base, x.ss_qual, x.ss_depth, x.ss_err,
                 x.ss_wide, x.ss_wdepth, x.ss_werr, molecular=bool(x.kind), stride=x.stride)
    return acc


def assert_words(got, want, cycles, what):
    if np.array_equal(got, want):
        return
    g, w = metrics.views(got, cycles), metrics.views(np.asarray(want), cycles)
    for k in g:
        bad = np.argwhere(g[k] != w[k])
        assert bad.shape[0] == 0, "%s: %s differs at %s: got %s want %s" % (
            what, k, bad[:6].tolist(), [int(g[k][tuple(i)]) for i in bad[:6]], [int(w[k][tuple(i)]) for i in bad[:6]])


def test_layout_and_exports():
    lib = _lib.load()
    assert lib.bsdc_abi_version() == 19
    for k in ("bsdc_metrics_words", "bsdc_metrics", "bsdc_metrics_filter", "bsdc_metrics_host",
              "bsdc_metrics_filter_host", "bsdc_metrics_last_error"):
        assert k in _lib.EXPORTS and hasattr(lib, k)
    assert metrics.words(512) == 16 + 1536 + 612 + 190 + 12 * 512 == MR.words(MR.empty(512)).shape[0]
    assert metrics.words(2) == metrics.BY_CYCLE + 24
    for bad in (1, 0, -3, 1025):
        with pytest.raises(ValueError, match="cycles"):
            metrics.words(bad)


@pytest.mark.parametrize("name", MI.NAMES)
def test_twin_equals_the_restatement_on_fabricated_rows(name):
    x = MI.make(name)
    assert_words(twin(x), MI.reference(name), x.cycles, name)


def test_fabricated_rows_hold_their_edges():
    """what the sets are for, read off the restatement's tables"""
    v = metrics.views(np.asarray(MI.reference("edges")), 512)
    assert v["rate_hist"][0, 0, 101] >= 2 and v["rate_hist"][1, 0, 101] >= 3       # no depth: NaN
    assert v["rate_hist"][1, 0, 1] >= 1 and v["rate_hist"][1, 0, 100] >= 1          # 1/1000, 100/1000
    assert v["rate_hist"][1, 0, 25] >= 1                                            # 1/40
    assert float(np.float32(1) / np.float32(1000)) * 1000.0 >= 1.0
    assert float(np.float32(1) / np.float32(40)) * 1000.0 >= 25.0
    assert v["depth_hist"][1, 0, 255] == 4 and v["depth_hist"][0, 0, 255] == 4     # 255, 256, 32767 wide + byte 255
    assert (v["qual_hist"].sum(axis=0)[:94] > 0).all() and v["qual_hist"][:, 94].sum() > 0
    x = MI.make("edges")
    f = x.notes["n_columns"][0]
    one = MI.Rows("one", 0, x.stride, 512, x.status[f:f + 1], x.length[f:f + 1], x.seq[f:f + 1], x.qual[f:f + 1],
                  x.ss_len[f:f + 1], x.ss_base[f:f + 1], x.ss_qual[f:f + 1], x.ss_depth[f:f + 1], x.ss_err[f:f + 1], None,
                  x.ss_wdepth[:0], x.ss_werr[:0])
    t = metrics.views(twin(one), 512)
    assert t["by_cycle"][0, :4, 5].tolist() == [0, 0, 1, 0]   # N / base, N / N, C / G, code 3 / base
    assert t["by_cycle"][0, :4, 1].tolist() == [1, 1, 0, 0]
    # the overflow row and cycles 2
    big = metrics.views(np.asarray(MI.reference("s528_f65")), 512)["by_cycle"]
    y = MI.make("s528_f65")
    L0 = y.length[(y.status & 1) != 0, 0]
    assert big[0, 511, 0] == np.maximum(L0 - 511, 0).sum() > (L0 > 511).sum() > 0 and big[0, 510, 0] == (L0 > 510).sum()
    two = metrics.views(np.asarray(MI.reference("s32_c2_f65")), 2)["by_cycle"]
    assert two[0, 1, 0] > two[0, 0, 0] > 0
    for name in ("bad", "bad_mol"):
        c = metrics.views(np.asarray(MI.reference(name)), 512)["counts"]
        assert c[metrics.SKIPPED] == 4 and c[metrics.EMITTED] == 9 and c[metrics.RECORDS] == 10


@pytest.mark.parametrize("name", ["c2", "c3", "wide", "molecular"])
def test_twin_equals_the_restatement_on_oracle_rows(name):
    """~2,000 C2 families, ~60 C3 families, a family whose depths pass a byte, step-1 records"""
    c = FI.case(name)
    r = c.oracle
    want = MR.words(MR.run(r.ss, r.cons_seq, r.cons_qual, r.cons_len, r.status, molecular=c.molecular))
    x = MI.from_oracle(r, c.molecular)
    assert (name == "wide") == bool(x.ss_wdepth.shape[0])
    got = twin(x)
    assert_words(got, want, 512, name)
    assert got[metrics.RECORDS] == 2 * int((r.status & 1).sum()) > 0


def test_two_calls_accumulate_and_filter_counters():
    x, y = MI.make("s16_f65"), MI.make("s16_f300")
    acc = twin(x)
    twin(y, acc)
    assert_words(acc, np.asarray(MI.reference("s16_f65")) + np.asarray(MI.reference("s16_f300")), 512, "sum")
    c = FI.case("c3")
    r = c.oracle
    filt, masked, _, _ = c.reference(FI.PARAM_SETS["typical"])
    want = MR.run(r.ss, r.cons_seq, r.cons_qual, r.cons_len, r.status, filt=filt, masked=masked)["counts"]
    acc = np.zeros(metrics.words(512), np.uint64)
    metrics.host_filter(acc, r.status.astype(np.uint8), filt, masked)
    assert np.array_equal(acc[4:16], want[4:16]) and not acc[:4].any() and not acc[16:].any()
    assert acc[metrics.KEPT] == int(((r.status & 1 != 0) & (filt == 0)).sum())
    assert acc[metrics.READERR] == int((filt & FR.READERR != 0).sum())


def _call(o, F=0, W=0, mol=0, cycles=512, acc=True):
    lib = _lib.load()
    a = np.zeros(metrics.words(512), np.uint64)
    rc = lib.bsdc_metrics_host(None, C.byref(o) if o is not None else None, F, W, mol, cycles,
                               C.c_void_p(a.ctypes.data) if acc else None)
    return rc, lib.bsdc_metrics_last_error().decode()


def test_refusals_name_the_field():
    buf = np.zeros(256, np.uint8)
    fields = ("status", "len", "seq", "qual", "ss_len", "ss_base", "ss_qual", "ss_depth", "ss_err")

    def good():
        o = _lib.ConsensusC()
        o.stride = 16
        for k in fields:
            setattr(o, k, buf.ctypes.data)
        return o
    assert _call(good())[0] == 0
    for k in fields:  # null rows
        o = good()
        setattr(o, k, None)
        rc, msg = _call(o)
        assert rc == -22 and k + " is null" in msg, (k, msg)
    for cyc in (1, 0, -1, 1025):
        rc, msg = _call(good(), cycles=cyc)
        assert rc == -22 and "cycles" in msg
    for stride in (0, 8, 24, 17, -16):
        o = good()
        o.stride = stride
        rc, msg = _call(o)
        assert rc == -22 and "stride" in msg
    assert _call(None)[0] == -22 and "out" in _call(None)[1]
    assert "acc" in _call(good(), acc=False)[1]
    assert "n_fam" in _call(good(), F=-1)[1] and "n_wide" in _call(good(), W=-1)[1]
    assert "molecular" in _call(good(), mol=2)[1]
    o = good()
    o.ss_wide = buf.ctypes.data
    assert "ss_wdepth" in _call(o, W=1)[1]
    lib = _lib.load()
    a = np.zeros(16, np.uint64)
    assert lib.bsdc_metrics_filter_host(None, None, buf.ctypes.data, buf.ctypes.data, 0, a.ctypes.data) == -22
    assert "status" in lib.bsdc_metrics_last_error().decode()


def test_report_is_fixed_and_cut():
    x = MI.make("edges")
    acc = twin(x)
    from bsseqconsensusreads_amd.device import ConsensusParams
    from bsseqconsensusreads_amd.filter import FilterParams
    doc = metrics.report(acc, 512, metrics.run_params(ConsensusParams(), False, FilterParams(20, (2, 1))))
    assert list(doc) == ["version", "cycles", "params", "counts", "depth_hist", "rate_hist", "qual_hist", "by_cycle"]
    assert list(doc["depth_hist"]) == ["cD", "aD", "bD"] and list(doc["rate_hist"])[2:] == ["cE", "aE", "bE"]
    assert doc["params"]["mode"] == "duplex" and doc["params"]["filter"]["min_reads"] == [2, 1, 1]
    assert doc["params"]["error_rate_pre_umi"] == 45.0 and doc["params"]["consensus_call_overlapping_bases"] is True
    assert len(doc["by_cycle"]["r1"]) == 32 == len(doc["by_cycle"]["r2"])  # (the longest read; rows past it cut)
    assert doc["by_cycle"]["columns"][0] == "records" and len(doc["by_cycle"]["r1"][0]) == 6
    assert "filter" in doc["counts"] and sum(doc["qual_hist"]["r1"]) == int(acc[metrics.QUAL_HIST:metrics.QUAL_HIST + 95].sum())
    plain = metrics.report(acc, 512, metrics.run_params(ConsensusParams(), True))
    assert "filter" not in plain["counts"] and plain["params"]["filter"] is None and plain["params"]["mode"] == "molecular"
    assert json.loads(json.dumps(doc)) == doc
    assert metrics.report(np.zeros(metrics.words(4), np.uint64), 4)["by_cycle"]["r1"] == []


def test_cli_and_stream_refusals(capsys):
    a = cli.parse(["step5", "-r", "g.fa", "in.bam", "out.bam", "--metrics", "m.json"])
    assert a.metrics == "m.json" and a.metrics_cycles == 512
    assert cli.parse(["molecular", "in.bam", "-", "--fastq1", "a", "--fastq2", "b", "--metrics", "m.json",
                      "--metrics-cycles", "64"]).metrics_cycles == 64
    assert cli.parse(["step5", "-r", "g.fa", "in.bam", "out.bam"]).metrics is None
    for argv, word in ((["step5", "-r", "g.fa", "in.bam", "out.bam", "--metrics", "m.json", "--gpus", "2"], "--gpus 2"),
                       (["step5", "-r", "g.fa", "in.bam", "out.bam", "--metrics", "m.json", "--metrics-cycles", "1"],
                        "--metrics-cycles")):
        with pytest.raises(SystemExit):
            cli.parse(argv)
        err = capsys.readouterr().err
        assert "--metrics" in err and word in err
    from bsseqconsensusreads_amd import stream
    assert stream.StreamJob("a", "b", "c").metrics is None
    with pytest.raises(ValueError, match="metrics"):
        stream.run(stream.StreamJob("a.bam", "r.fa", "o.bam", metrics="m.json"), runner=object())
    with pytest.raises(ValueError, match="metrics"):
        stream.run(stream.StreamJob("a.bam", "r.fa", "o.bam", metrics="m.json", rng=(0, 1)), engine=object())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_twin_under_sanitizers(tmp_path):
    """tests/sanitize/metrics_twin_main.cpp: the twin on heap buffers of their exact sizes under
    -fsanitize=address,undefined, the bad families counted and never read (host code, its own main)."""
    exe = str(tmp_path / "metrics_twin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-x", "c++", os.path.join(ROOT, "tests", "sanitize", "metrics_twin_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "metrics twin ok" in r.stdout

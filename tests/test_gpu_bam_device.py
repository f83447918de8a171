"""The device BAM record path on the GPU (csrc/bsdc_bam.hip; Engine.bam_records,
GpuBgzf.submit_device, BamWriter.add_device): bsdc_bam_format against the host encoder's bytes
(bam.consensus_tags + the host BAM writer) on fabricated and on voted batches, the writer fed from
HBM against the writer fed the same records on the --gpu-bgzf path byte for byte, and the command
line against the --gpu-bgzf and the default runs."""
import ctypes as C
import gzip

import numpy as np
import pytest
import torch

from bsseqconsensusreads_amd import _lib, bam, batch, pipeline, synth
import bamrec_inputs as BI

pytestmark = pytest.mark.gpu
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
DEV = "cuda:0"
GUARD = 64
CARRY_FAMS = 262145 + 1025  # 258 workgroups of the offset scan (bsdc_devtext.h): a tile of 256 and two more


# ---- 1. the format kernel alone

class _Call:
    """bsdc_bam_format's arguments for a BamRecInput, on the device."""

    def __init__(self, x: BI.BamRecInput, with_filt: bool, molecular: bool, tags: bool):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)  # noqa: E731
        pad = lambda a: a if a.size else np.zeros(4, a.dtype)  # noqa: E731
        self.x, self.F, self.kind, self.tags = x, x.n_fam, int(molecular), int(tags)
        self.keep = [up(x.status), up(x.length.astype(np.uint16)), up(x.seq), up(x.qual), up(x.filt),
                     up(x.ss_len.astype(np.uint16)), up(x.ss_base), up(x.ss_qual), up(x.ss_depth), up(x.ss_err),
                     up(x.ss_wide), up(pad(x.ss_wdepth)), up(pad(x.ss_werr))]
        o = self.o = _lib.ConsensusC()
        o.stride = x.stride
        o.status, o.len, o.seq, o.qual = (t.data_ptr() for t in self.keep[:4])
        (o.ss_len, o.ss_base, o.ss_qual, o.ss_depth, o.ss_err, o.ss_wide, o.ss_wdepth,
         o.ss_werr) = (t.data_ptr() for t in self.keep[5:])
        self.filt = self.keep[4].data_ptr() if with_filt else None
        nb, no, ab, ao = BI.tables(x)
        self.noff_h, self.aoff_h = no, ao
        self.dev = [up(nb if nb.size else np.zeros(1, np.uint8)), up(no), up(ab if ab.size else np.zeros(1, np.uint8)),
                    up(ao)]
        self.lib = _lib.load()
        self.bound = int(self.lib.bsdc_bam_bytes_bound(self.F, int(no[-1]), int(ao[-1]), x.stride, self.kind, self.tags))
        self.tmp = torch.empty(int(self.lib.bsdc_bam_tmp_bytes(self.F)), dtype=torch.uint8, device=DEV)

    def run(self, cap=None, **bad):
        cap = self.bound if cap is None else cap
        buf = torch.full((GUARD + max(cap, 0) + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        off = torch.full((self.F + 1,), -7, dtype=torch.int64, device=DEV)
        a = dict(out=C.byref(self.o), filt=self.filt, kind=self.kind, with_tags=self.tags, n_fam=self.F,
                 name_off=self.dev[1].data_ptr(), name_buf=self.dev[0].data_ptr(), name_off_host=self.noff_h.ctypes.data,
                 aux_off=self.dev[3].data_ptr(), aux_buf=self.dev[2].data_ptr(), aux_off_host=self.aoff_h.ctypes.data,
                 off=off.data_ptr(), rec=buf.data_ptr() + GUARD, cap=cap, tmp=self.tmp.data_ptr(), stream=None)
        a.update(bad)
        rc = self.lib.bsdc_bam_format(*a.values())
        torch.cuda.synchronize()
        return rc, buf.cpu().numpy(), off.cpu().numpy()


def _check(x, with_filt, molecular, tags, tmp_path):
    want, hoff = BI.expected(x, molecular, tags, with_filt, str(tmp_path))
    c = _Call(x, with_filt, molecular, tags)
    rc, buf, off = c.run()
    assert rc == 0
    n = len(want)
    assert np.array_equal(off, hoff) and int(off[-1]) == n <= c.bound
    assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + n:] == 0xA5).all()
    got = buf[GUARD:GUARD + n]
    if got.tobytes() != want:
        d = np.nonzero(got != np.frombuffer(want, np.uint8))[0]
        f = int(np.searchsorted(hoff, d[0], side="right") - 1)
        raise AssertionError("%d bytes differ, the first in family %d at its byte %d" % (d.shape[0], f, d[0] - hoff[f]))
    return c, want


@pytest.mark.parametrize("tags", [False, True], ids=["plain", "tags"])
@pytest.mark.parametrize("molecular", [False, True], ids=["duplex", "molecular"])
@pytest.mark.parametrize("with_filt", [False, True], ids=["nofilt", "filt"])
@pytest.mark.parametrize("stride", [16, 32, 528])
def test_format_equals_the_host_encoder(tmp_path, stride, with_filt, molecular, tags):
    x = BI.make(stride, 300, seed=stride)
    assert {"no_depth", "d255", "d256_m255", "d256_m256", "wide_max", "disagree"} <= set(x.notes)
    _check(x, with_filt, molecular, tags, tmp_path)


@pytest.mark.parametrize("written,n_fam", [("none", 300), ("all", 1), ("first_off", 300), ("last_off", 300),
                                           ("all", 1025), ("mixed", 2500), ("mixed", CARRY_FAMS)])
def test_format_family_patterns(tmp_path, written, n_fam):
    """no family written (total 0), one family, the first / last family unwritten, more families
    than one scan workgroup takes (1024), and more workgroups than k_scan_scan takes in one tile
    (256: the second tile starts from the first one's carry)"""
    big = n_fam == CARRY_FAMS
    x = BI.make(16 if big else 32, n_fam, seed=n_fam, written=written, vector_tables=big)
    _, want = _check(x, False, False, True, tmp_path)
    if written == "none":
        assert want == b""


def test_format_stops_at_cap(tmp_path):
    """cap = the total less 1, 2 and 5: no byte at or past cap changes, the total stays true"""
    x = BI.make(32, 300, seed=8, written="all")  # (the last bytes are a record's)
    c, want = _check(x, False, False, True, tmp_path)
    for cut in (1, 2, 5):
        cap = len(want) - cut
        rc, buf, off = c.run(cap)
        assert rc == 0 and int(off[-1]) == len(want)
        assert buf[GUARD:GUARD + cap].tobytes() == want[:cap]
        assert (buf[GUARD + cap:] == 0xA5).all() and (buf[:GUARD] == 0xA5).all(), cut


def test_format_refusals_and_a_good_call_after_them(tmp_path):
    x = BI.make(32, 40, seed=1)
    c = _Call(x, True, False, True)
    for k in ("out", "name_off", "name_buf", "name_off_host", "aux_off", "aux_buf", "aux_off_host", "off", "rec", "tmp"):
        assert c.run(**{k: None})[0] == -22, k
    assert c.run(n_fam=-1)[0] == -22 and c.run(cap=-1)[0] == -22
    assert c.run(kind=2)[0] == -22 and c.run(kind=-1)[0] == -22
    long = c.noff_h.copy()
    long[7:] += 254 - (long[7] - long[6])  # name 6: 254 bytes
    assert c.run(name_off_host=long.ctypes.data)[0] == -22
    for k, h in (("name_off_host", c.noff_h), ("aux_off_host", c.aoff_h)):
        back = h.copy()
        back[3] = back[2] - 1
        assert c.run(**{k: back.ctypes.data})[0] == -22, k
    ss_len, c.o.ss_len = c.o.ss_len, None
    assert c.run()[0] == -22
    c.o.ss_len = ss_len
    want, hoff = BI.expected(x, False, True, True, str(tmp_path))
    rc, buf, off = c.run()
    assert rc == 0 and np.array_equal(off, hoff) and buf[GUARD:GUARD + len(want)].tobytes() == want


# ---- 2. voted batches

def _vote(engine, raw, ref, molecular=False, tags=True):
    """one batch voted with the tags' rows, its records written on the device -> (db, cons, the host
    records of the same consensus, the fetched offsets)"""
    if molecular:
        raw = pipeline.molecular_records(raw)
        plan = pipeline.plan_families(raw, "vote", family_order="mi-group")
        mode, flags = pipeline.MODE_VOTE, dict(min_consensus_base_quality=0)
    else:
        engine.load_reference(ref)
        plan = pipeline.plan_families(raw, "full", engine.ref)
        assert not plan.split_ext
        mode, flags = pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE, {}
    fb = batch.materialize(plan, 0, plan.n_fam)
    db = engine.upload(fb, tags=True)
    with engine.flags(**flags):
        engine.run(db, mode | pipeline.MODE_TAGS)
    names = bam.family_names(fb.fam_mi, raw.mi_names, "x")
    aux = bam.family_aux(fb.fam_off, fb.src, fb.fam_mi, raw)
    engine.bam_records(db, names, aux, molecular=molecular, tags=tags)
    small = db.fetch(seqqual=False)
    assert set(small) == {"status", "len", "stride", "bam_off"}  # (no seq, qual or ss rows)
    out = db.fetch(ss=tags)
    assert np.array_equal(out["bam_off"], small["bam_off"])
    cons = pipeline.consensus_from_output(fb, out)
    recs = bam.duplex_records(cons, raw, "x", molecular=molecular)
    return db, cons, recs, out["bam_off"]


def _device_equals_host(db, cons, recs, off, tmp_path):
    want = BI.host_bytes(recs, str(tmp_path), "v")
    kept = (cons.status & 1) != 0
    per = np.zeros(cons.status.shape[0], np.int64)
    per[kept] = BI.record_sizes(recs).reshape(-1, 2).sum(axis=1)
    assert np.array_equal(np.diff(off), per) and off[0] == 0 and int(off[-1]) == len(want) <= db.bamrec.cap
    db.bamrec.event.synchronize()
    assert db.bamrec.rec[:len(want)].cpu().numpy().tobytes() == want
    return want


@pytest.fixture(scope="module")
def voted(engine):
    s = synth.generate("C2", 3000, seed=21, device="cpu", genome_len=300_000)
    return _vote(engine, s.raw, s.ref)


def test_voted_c2_records_equal_the_host_encoder(voted, tmp_path):
    _device_equals_host(*voted, tmp_path)


@pytest.mark.parametrize("name", ["c3", "wide", "molecular"])
def test_voted_edge_records_equal_the_host_encoder(engine, tmp_path, name):
    """k_large's rows (c3), a family of 520 records whose wide rows hold depths past a byte (wide),
    and step-1 records (molecular)"""
    import filter_inputs as FI
    c = FI.case(name)
    db, cons, recs, off = _vote(engine, c.raw, c.ref, molecular=c.molecular)
    if name == "wide":
        assert db.n_wide >= 1 and int(db.ss_wdepth.max()) > 255
    _device_equals_host(db, cons, recs, off, tmp_path)


def test_voted_records_without_tags(engine, tmp_path):
    s = synth.generate("C2", 300, seed=5, device="cpu", genome_len=100_000)
    db, cons, recs, off = _vote(engine, s.raw, s.ref, tags=False)
    assert recs.aux2 is None
    _device_equals_host(db, cons, recs, off, tmp_path)


# ---- 3. the writer

CUTS = (0, 500, 1700, 1800, None)  # four adds of unequal size (family indices); a flush after the second
HEADER = bam.BamHeader("@HD\tVN:1.6\tSO:unsorted\tGO:query\n@SQ\tSN:chr1\tLN:300000\n", ["chr1"],
                       np.asarray([300000], np.int64))


def _header_bytes(tmp_path) -> bytes:
    p = str(tmp_path / "hdr.bam")
    bam.BamWriter(p, HEADER, 1).close()
    return gzip.decompress(open(p, "rb").read())


def _write_both(voted, tmp_path, tag, fragment=None, force=None):
    db, cons, recs, off = voted
    F = cons.status.shape[0]
    cuts = [F if c is None else c for c in CUTS]
    em = np.concatenate([[0], np.cumsum((cons.status & 1) != 0)])
    paths, flushed, gpus = {}, {}, {}
    for device in (False, True):
        paths[device] = str(tmp_path / ("%s_%s.bam" % (tag, "dev" if device else "ref")))
        g = gpus[device] = bam.GpuBgzf(0)
        if device:
            g.force_host = force
        w = bam.BamWriter(paths[device], HEADER, 5, gpu=g, fragment=fragment)
        for k in range(4):
            a, b = cuts[k], cuts[k + 1]
            if device:
                w.add_device([[(db.bamrec.rec, int(off[a]), int(off[b]), db.bamrec.event)]], 4)
            else:
                w.add(bam.take_records(recs, np.arange(2 * em[a], 2 * em[b])), 4)
            if k == 1:
                flushed[device] = w.flush(4)
        w.close(4)
    return paths, flushed, gpus, off, cuts


def _members(raw: bytes):
    out, o = [], 0
    while o < len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04" and raw[o + 12:o + 14] == b"BC"
        out.append(o)
        o += int.from_bytes(raw[o + 16:o + 18], "little") + 1
    assert o == len(raw)
    return out


@pytest.mark.parametrize("fragment", [None, "first", "next"])
def test_writer_from_device_records_equals_the_gpu_bgzf_writer(voted, tmp_path, fragment):
    paths, flushed, gpus, off, cuts = _write_both(voted, tmp_path, "w%s" % fragment, fragment)
    assert flushed[True] == flushed[False]
    # (0 handed back is asserted of the device path only after the reference writer's own GpuBgzf saw 0)
    assert gpus[False].blocks >= 8 and gpus[False].fallback_blocks == 0
    assert gpus[True].blocks == gpus[False].blocks and gpus[True].fallback_blocks == 0
    a, b = open(paths[False], "rb").read(), open(paths[True], "rb").read()
    assert a == b
    assert b.endswith(EOF_BLOCK) == (fragment is None)
    head = _header_bytes(tmp_path) if fragment != "next" else b""
    want = voted[0].bamrec.rec[:int(off[-1])].cpu().numpy().tobytes()
    data = gzip.decompress(b) if b else b""
    assert data == head + want
    cut = flushed[True]
    assert cut in _members(b) + [len(b)]
    assert gzip.decompress(b[:cut]) == head + want[:int(off[cuts[2]])]


def test_writer_blocks_handed_back_to_the_host(voted, tmp_path):
    """blocks whose size the (test-only) hook zeroes go down the sink's host deflate with the raw
    bytes fetched for exactly them; the records are the same"""
    pick = lambda first, n: [b for b in range(n) if (first + b) % 7 == 3]  # noqa: E731
    paths, flushed, gpus, off, cuts = _write_both(voted, tmp_path, "h", force=pick)
    g = gpus[True]
    want = [k for k in range(g.blocks) if k % 7 == 3]
    assert want and g.raw_fetched == want and g.fallback_blocks == len(want)
    a, b = open(paths[False], "rb").read(), open(paths[True], "rb").read()
    assert gzip.decompress(a) == gzip.decompress(b) and b.endswith(EOF_BLOCK)
    assert gzip.decompress(b[:flushed[True]]) == gzip.decompress(a[:flushed[False]])


def test_host_device_and_raw_adds_keep_order(voted, tmp_path):
    """add -> add_device -> add_raw -> add_device -> close: the header and the host records go in
    front of the device records (bsdc_bgzf_sink_take_tail), the device remainder in front of the
    raw records; the file holds header + all records in order."""
    db, cons, recs, off = voted
    F = cons.status.shape[0]
    em = np.concatenate([[0], np.cumsum((cons.status & 1) != 0)])
    whole = db.bamrec.rec[:int(off[-1])].cpu().numpy().tobytes()
    p = str(tmp_path / "mix.bam")
    w = bam.BamWriter(p, HEADER, 5, gpu=bam.GpuBgzf(0))
    w.add(bam.take_records(recs, np.arange(2 * em[0], 2 * em[500])), 4)
    w.add_device([[(db.bamrec.rec, int(off[500]), int(off[1700]), db.bamrec.event)]], 4)
    w.add_raw(whole[int(off[1700]):int(off[1800])], 4)
    w.add_device([[(db.bamrec.rec, int(off[1800]), int(off[F]), db.bamrec.event)]], 4)
    w.close(4)
    assert gzip.decompress(open(p, "rb").read()) == _header_bytes(tmp_path) + whole


# ---- 4. the command line

def _cli(capsys, argv):
    """cli.main in this process -> the info it prints (JSON on stderr)"""
    import json

    from bsseqconsensusreads_amd import cli
    capsys.readouterr()
    rc = cli.main(argv)
    err = capsys.readouterr().err
    assert rc == 0, err
    return json.loads([x for x in err.splitlines() if x.startswith("{")][-1])


@pytest.fixture(scope="module")
def long_bam(tmp_path_factory):
    """a 1,500-family coordinate-sorted C2 BAM with long-span templates (tests/test_long_span.py)"""
    from test_long_span import _long_input
    tmp = tmp_path_factory.mktemp("longbam")
    _, p, fa, span = _long_input(tmp, n_fam=1500)
    assert (span > 20_000).sum() >= 20
    return tmp, p, fa


def _step5(capsys, long_bam, tag, fastq, *more):
    tmp, p, fa = long_bam
    fq = [str(tmp / ("%s_%d.fq.gz" % (tag, d))) for d in (1, 2)]
    out = str(tmp / (tag + ".bam"))
    info = _cli(capsys, ["step5", "-r", fa, p, out, "--threads", "4", "--chunk-mb", "1"] +
                (["--fastq1", fq[0], "--fastq2", fq[1]] if fastq else []) + list(more))
    return info, open(out, "rb").read(), [open(x, "rb").read() for x in fq] if fastq else None


COUNTERS = ("records_in", "families", "families_emitted", "records_out", "spliced_families")


@pytest.mark.parametrize("more", [(), ("--filter-min-base-quality", "20", "--filter-min-reads", "2", "1", "1"),
                                  ("--output-per-base-tags", "false")], ids=["plain", "filtered", "notags"])
def test_cli_step5(capsys, long_bam, more):
    """the BAM equals the --gpu-bgzf run's byte for byte and holds the default run's records; the
    deferral's cuts and its second pass fire"""
    t = "%d" % len(more)
    base, b0, _ = _step5(capsys, long_bam, "d" + t, False, *more)
    ref, b1, _ = _step5(capsys, long_bam, "b" + t, False, "--gpu-bgzf", "true", *more)
    info, b2, _ = _step5(capsys, long_bam, "g" + t, False, "--gpu-bam", "true", *more)
    assert info["spliced_families"] > 0 and info["spilled_bytes"] > 0 and info.get("deferred_records", 0) > 0
    assert b2 == b1
    assert gzip.decompress(b2) == gzip.decompress(b0)
    for k in COUNTERS:
        assert info[k] == ref[k] == base[k], k
    g = info["gpu_bam"]
    assert set(g) == {"blocks", "raw_bytes", "compressed_bytes", "fallback_blocks"}
    # (both passes' counters; a piece between two cuts of this small input may be shorter than a
    # block, so the filtered and untagged runs may see no whole block: the tagged records fill some)
    assert g["blocks"] >= (0 if more else 1) and g["raw_bytes"] == 65280 * g["blocks"]
    assert g["compressed_bytes"] <= g["raw_bytes"] and (g["compressed_bytes"] > 0) == (g["blocks"] > 0)
    if len(more) > 2:
        assert info["filter"] == base["filter"] and info["filter"]["kept"] < info["filter"]["templates"]


def test_cli_step5_with_the_fastq_pair(capsys, long_bam):
    """with --gpu-fastq true too: both outputs are the --gpu-bgzf run's; with a host-formatted pair
    beside the device BAM: likewise"""
    ref, b1, fq1 = _step5(capsys, long_bam, "fb", True, "--gpu-bgzf", "true")
    info, b2, fq2 = _step5(capsys, long_bam, "fg", True, "--gpu-bam", "true", "--gpu-fastq", "true")
    assert b2 == b1 and fq2 == fq1
    for k in COUNTERS:
        assert info[k] == ref[k], k
    assert "gpu_bam" in info and "gpu_fastq" in info
    info, b3, fq3 = _step5(capsys, long_bam, "fh", True, "--gpu-bam", "true", "--gpu-bgzf", "true", "--gpu-inflate", "true")
    assert b3 == b1 and fq3 == fq1


def test_cli_molecular(capsys, tmp_path):
    from test_molecular_stream import grouped_bam
    _, p = grouped_bam(tmp_path, n_fam=1500)
    runs = {}
    for tag, more in (("d", ()), ("b", ("--gpu-bgzf", "true")), ("g", ("--gpu-bam", "true"))):
        out = str(tmp_path / (tag + ".bam"))
        runs[tag] = (_cli(capsys, ["molecular", p, out, "--threads", "4", "--chunk-mb", "1"] + list(more)),
                     open(out, "rb").read())
    assert runs["g"][1] == runs["b"][1]
    assert gzip.decompress(runs["g"][1]) == gzip.decompress(runs["d"][1])
    assert runs["g"][0]["records_out"] == runs["d"][0]["records_out"] > 0
    assert runs["g"][0]["gpu_bam"]["blocks"] > 0

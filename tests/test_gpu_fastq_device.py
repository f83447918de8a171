"""The device FASTQ path on the GPU (csrc/bsdc_fastq.hip; Engine.fastq, GpuBgzf.submit_device,
FastqWriter.add_device): bsdc_bgzf_crc32 against zlib, bsdc_fastq_format against the host writer's
text (bam.write_fastq) and bam.fastq_offsets, and the writer fed from HBM against the writer fed
the same records on the --gpu-bgzf path, byte for byte."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest
import torch

from bsseqconsensusreads_amd import _lib, bam, pipeline, synth
import fastq_inputs as FI

pytestmark = pytest.mark.gpu
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
DEV = "cuda:0"


# ---- 1. CRC32

def _crc(data: bytes, blk0: int):
    lib = _lib.load()
    nblk = len(data) // 65280
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(DEV)
    crc = torch.full((nblk,), 0x55AA55AA, dtype=torch.int32, device=DEV)
    assert lib.bsdc_bgzf_crc32(d.data_ptr(), blk0, nblk - blk0, crc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return crc.cpu().numpy().view(np.uint32)


def test_crc32_equals_zlib():
    for name, data in FI.crc_contents().items():
        nblk = len(data) // 65280
        want = [zlib.crc32(data[b * 65280:(b + 1) * 65280]) for b in range(nblk)]
        for blk0 in (0, 1):
            got = _crc(data, blk0)
            assert [int(v) for v in got[blk0:]] == want[blk0:], (name, blk0)
            assert all(int(v) == 0x55AA55AA for v in got[:blk0]), (name, blk0)  # (blocks before blk0 untouched)
        one = _crc(data[:65280], 0)
        assert int(one[0]) == want[0], name
        if name.startswith("pair_"):
            assert want[0] != want[1]


def test_crc32_refusals():
    lib = _lib.load()
    d = torch.zeros(65280 + 16, dtype=torch.uint8, device=DEV)
    crc = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.bsdc_bgzf_crc32(None, 0, 1, crc.data_ptr(), None) == -22
    assert lib.bsdc_bgzf_crc32(d.data_ptr(), 0, 1, None, None) == -22
    assert lib.bsdc_bgzf_crc32(d.data_ptr(), -1, 1, crc.data_ptr(), None) == -22
    assert lib.bsdc_bgzf_crc32(d.data_ptr(), 0, -1, crc.data_ptr(), None) == -22
    assert lib.bsdc_bgzf_crc32(d.data_ptr() + 1, 0, 1, crc.data_ptr(), None) == -22  # (in: 16-byte aligned)
    assert lib.bsdc_bgzf_crc32(d.data_ptr(), 0, 0, crc.data_ptr(), None) == 0


# ---- 2. the format kernel alone

GUARD = 64
CARRY_FAMS = 262145 + 1025  # 258 workgroups of the offset scan (bsdc_devtext.h): a tile of 256 and two more


class _Call:
    """bsdc_fastq_format's arguments for a FastqInput, on the device."""

    def __init__(self, x: FI.FastqInput, with_filt: bool):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)  # noqa: E731
        self.x, self.F = x, x.n_fam
        self.keep = [up(x.status), up(x.length.astype(np.uint16)), up(x.seq), up(x.qual), up(x.filt)]
        self.o = _lib.ConsensusC()
        self.o.stride = x.stride
        self.o.status, self.o.len, self.o.seq, self.o.qual = (t.data_ptr() for t in self.keep[:4])
        self.filt = self.keep[4].data_ptr() if with_filt else None
        buf, off = FI.name_table(x)
        self.off_h = off
        self.nbuf = up(buf if buf.size else np.zeros(1, np.uint8))
        self.noff = up(off)
        self.lib = _lib.load()
        self.bound = int(self.lib.bsdc_fastq_text_bound(self.F, int(off[-1]), x.stride))
        self.tmp = torch.empty(int(self.lib.bsdc_fastq_tmp_bytes(self.F)), dtype=torch.uint8, device=DEV)

    def run(self, caps=None, **bad):
        caps = (self.bound, self.bound) if caps is None else caps
        text = [torch.full((max(c, 0) + GUARD,), 0xA5, dtype=torch.uint8, device=DEV) for c in caps]
        off = torch.full((2, self.F + 1), -7, dtype=torch.int64, device=DEV)
        a = dict(out=C.byref(self.o), filt=self.filt, n_fam=self.F, name_off=self.noff.data_ptr(),
                 name_buf=self.nbuf.data_ptr(), name_off_host=self.off_h.ctypes.data, off0=off[0].data_ptr(),
                 off1=off[1].data_ptr(), text0=text[0].data_ptr(), text1=text[1].data_ptr(), cap0=caps[0], cap1=caps[1],
                 tmp=self.tmp.data_ptr(), stream=None)
        a.update(bad)
        rc = self.lib.bsdc_fastq_format(*a.values())
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy() for t in text], off.cpu().numpy()


def _check(x, with_filt, tmp_path):
    keep = x.kept(with_filt)
    want = FI.host_text(x, np.nonzero(keep)[0], str(tmp_path))
    hoff = bam.fastq_offsets(x.status, x.length, x.filt if with_filt else None, x.names.off)
    c = _Call(x, with_filt)
    rc, text, off = c.run()
    assert rc == 0
    for d in range(2):
        assert np.array_equal(off[d], hoff[d]), d
        n = len(want[d])
        assert int(off[d][-1]) == n <= c.bound
        assert text[d][:n].tobytes() == want[d], d
        assert (text[d][n:] == 0xA5).all(), d
    return c, want


@pytest.mark.parametrize("stride", [16, 32, 528])
@pytest.mark.parametrize("with_filt", [False, True])
def test_format_equals_the_host_writer(tmp_path, stride, with_filt):
    x = FI.make(stride, 300, seed=stride)
    L = set(x.length[x.kept(with_filt)].reshape(-1).tolist())
    assert {0, 1, 2, 3, 4, 5, stride - 2} <= L and any(v & 1 and v > 5 for v in L)
    assert {1, 2, 3, 4, 5, 254} <= set(np.diff(x.names.off)[x.kept(with_filt)].tolist())
    _, want = _check(x, with_filt, tmp_path)
    if stride == 528:  # every code's letter and every quality byte went through
        assert set(b"=ACMGRSVTWYHKDBN") <= set(want[0])
        assert len(set(want[0])) == 256


@pytest.mark.parametrize("written,n_fam", [("none", 300), ("all", 1), ("first_off", 300), ("last_off", 300),
                                           ("all", 1025), ("mixed", 2500), ("mixed", CARRY_FAMS)])
def test_format_family_patterns(tmp_path, written, n_fam):
    """no family written (totals 0), one family, the first / last family unwritten, more families
    than one scan workgroup takes (1024), and more workgroups than k_scan_scan takes in one tile
    (256: the second tile starts from the first one's carry)"""
    big = n_fam == CARRY_FAMS
    x = FI.make(16 if big else 32, n_fam, seed=n_fam, written=written, vector_names=big)
    _, want = _check(x, False, tmp_path)
    if written == "none":
        assert want == (b"", b"")


def test_format_stops_at_cap(tmp_path):
    """cap = the total less 1, 2 and 5: no byte at or past cap changes, the totals stay true"""
    x = FI.make(32, 300, seed=8, written="all")  # (the text's last bytes are a record's)
    c, want = _check(x, False, tmp_path)
    for cut in (1, 2, 5):
        caps = (len(want[0]) - cut, len(want[1]) - cut)
        rc, text, off = c.run(caps)
        assert rc == 0
        for d in range(2):
            assert int(off[d][-1]) == len(want[d])
            assert text[d][:caps[d]].tobytes() == want[d][:caps[d]]
            assert (text[d][caps[d]:] == 0xA5).all(), (cut, d)


def test_format_refusals():
    x = FI.make(32, 20, seed=1)
    c = _Call(x, True)
    for k in ("out", "name_off", "name_buf", "name_off_host", "off0", "off1", "text0", "text1", "tmp"):
        assert c.run(**{k: None})[0] == -22, k
    assert c.run(n_fam=-1)[0] == -22
    assert c.run(cap0=-1)[0] == -22 and c.run(cap1=-1)[0] == -22
    long = c.off_h.copy()
    long[5:] += 255 - (long[5] - long[4])  # name 4: 255 bytes
    assert c.run(name_off_host=long.ctypes.data)[0] == -22
    back = c.off_h.copy()
    back[3] = back[2] - 1
    assert c.run(name_off_host=back.ctypes.data)[0] == -22
    assert c.run()[0] == 0


# ---- 3. the writer

CUTS = (0, 500, 1700, 1800, None)  # four adds of unequal size (family indices); a flush after the second


@pytest.fixture(scope="module")
def voted(engine):
    s = synth.generate("C2", 3000, seed=21, device="cpu", genome_len=300_000)
    engine.load_reference(s.ref)
    fb = pipeline.build_family_batch(s.raw, "full", engine.ref)
    db = engine.upload(fb)
    engine.run(db, pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE)
    names = bam.family_names(fb.fam_mi, s.raw.mi_names, "x")
    fq = engine.fastq(db, names)
    small = db.fetch(seqqual=False)
    cons = pipeline.consensus_from_output(fb, db.fetch())
    assert np.array_equal(small["status"], cons.status) and np.array_equal(small["len"], cons.length)
    recs = bam.duplex_records(cons, s.raw, "x")
    off = bam.fastq_offsets(cons.status, cons.length, None, names.off)
    assert small["fastq_total"] == (int(off[0][-1]), int(off[1][-1])) == fq.total
    return db, cons, recs, off


def _write_both(voted, tmp_path, tag, fragment=False, force=None):
    db, cons, recs, off = voted
    F = cons.status.shape[0]
    cuts = [F if c is None else c for c in CUTS]
    em = np.concatenate([[0], np.cumsum((cons.status & 1) != 0)])
    ref = [str(tmp_path / ("%s_ref%d.fq.gz" % (tag, d))) for d in (1, 2)]
    dev = [str(tmp_path / ("%s_dev%d.fq.gz" % (tag, d))) for d in (1, 2)]
    flushed = {}
    for paths, device in ((ref, False), (dev, True)):
        g = bam.GpuBgzf(0)
        if device:
            g.force_host = force
        w = bam.FastqWriter(paths[0], paths[1], 5, gpu=g, fragment=fragment)
        for k in range(4):
            a, b = cuts[k], cuts[k + 1]
            if device:
                w.add_device([[(db.fastq.text[d], int(off[d][a]), int(off[d][b]), db.fastq.event)] for d in range(2)], 4)
            else:
                w.add(bam.take_records(recs, np.arange(2 * em[a], 2 * em[b])), 4)
            if k == 1:
                flushed[device] = w.flush(4)
        w.close(4)
        if device:
            gdev = g
    return ref, dev, flushed, gdev, off, cuts


def _gunzip_members(raw: bytes) -> bytes:
    """every gzip member inflated and its CRC32 / ISIZE checked (gzip does both)"""
    return gzip.decompress(raw)


@pytest.mark.parametrize("fragment", [False, True])
def test_writer_from_device_text_equals_the_gpu_bgzf_writer(voted, tmp_path, fragment):
    ref, dev, flushed, g, off, cuts = _write_both(voted, tmp_path, "w%d" % fragment, fragment)
    assert flushed[True] == flushed[False]
    assert g.blocks >= 8 and g.fallback_blocks == 0
    for d in range(2):
        a, b = open(ref[d], "rb").read(), open(dev[d], "rb").read()
        assert a == b, d
        assert b.endswith(EOF_BLOCK) != fragment
        text = _gunzip_members(b)
        assert len(text) == int(off[d][-1])
        assert text == voted[0].fastq.text[d][:len(text)].cpu().numpy().tobytes()
        cut = flushed[True][d]
        assert _gunzip_members(b[:cut]) == text[:int(off[d][cuts[2]])]


def test_writer_blocks_handed_back_to_the_host(voted, tmp_path):
    """blocks whose size the (test-only) hook zeroes go down the sink's host deflate with the raw
    bytes fetched for exactly them; the records are the same"""
    pick = lambda first, n: [b for b in range(n) if (first + b) % 7 == 3]  # noqa: E731
    ref, dev, flushed, g, off, cuts = _write_both(voted, tmp_path, "h", force=pick)
    want = [k for k in range(g.blocks) if k % 7 == 3]
    assert want and g.raw_fetched == want and g.fallback_blocks == len(want)
    for d in range(2):
        a, b = open(ref[d], "rb").read(), open(dev[d], "rb").read()
        assert _gunzip_members(a) == _gunzip_members(b)
        assert b.endswith(EOF_BLOCK)
        assert _gunzip_members(b[:flushed[True][d]]) == _gunzip_members(a[:flushed[False][d]])


def test_host_adds_and_device_adds_interleave_in_order(voted, tmp_path):
    """add -> add_device -> add -> close: the host text's remainder goes in front of the device
    text (bsdc_bgzf_sink_take_tail) and the device remainder in front of the next host text; the
    files equal those of the writer that got all three parts as records."""
    db, cons, recs, off = voted
    F = cons.status.shape[0]
    em = np.concatenate([[0], np.cumsum((cons.status & 1) != 0)])
    part = lambda a, b: bam.take_records(recs, np.arange(2 * em[a], 2 * em[b]))  # noqa: E731
    ref = [str(tmp_path / ("m_ref%d.fq.gz" % d)) for d in (1, 2)]
    mix = [str(tmp_path / ("m_mix%d.fq.gz" % d)) for d in (1, 2)]
    w = bam.FastqWriter(ref[0], ref[1], 5, gpu=bam.GpuBgzf(0))
    for a, b in ((0, 500), (500, 1700), (1700, F)):
        w.add(part(a, b), 4)
    w.close(4)
    w = bam.FastqWriter(mix[0], mix[1], 5, gpu=bam.GpuBgzf(0))
    w.add(part(0, 500), 4)
    w.add_device([[(db.fastq.text[d], int(off[d][500]), int(off[d][1700]), db.fastq.event)] for d in range(2)], 4)
    w.add(part(1700, F), 4)
    w.close(4)
    for d in range(2):
        assert open(ref[d], "rb").read() == open(mix[d], "rb").read(), d
        assert len(gzip.decompress(open(mix[d], "rb").read())) == int(off[d][-1])


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


def _read(paths):
    return [open(p, "rb").read() for p in paths]


@pytest.fixture(scope="module")
def long_bam(tmp_path_factory):
    """a 1,500-family coordinate-sorted C2 BAM with long-span templates (tests/test_long_span.py)"""
    from test_long_span import _long_input
    tmp = tmp_path_factory.mktemp("long")
    _, p, fa, span = _long_input(tmp, n_fam=1500)
    assert (span > 20_000).sum() >= 20
    return tmp, p, fa


def _step5(capsys, long_bam, tag, out, *more):
    tmp, p, fa = long_bam
    fq = [str(tmp / ("%s_%d.fq.gz" % (tag, d))) for d in (1, 2)]
    bam_out = str(tmp / (tag + ".bam")) if out else "-"
    info = _cli(capsys, ["step5", "-r", fa, p, bam_out, "--fastq1", fq[0], "--fastq2", fq[1], "--threads", "4",
                         "--chunk-mb", "1"] + list(more))
    return info, fq, bam_out


@pytest.mark.parametrize("more", [(), ("--filter-min-base-quality", "20", "--filter-min-reads", "2", "1", "1")],
                         ids=["plain", "filtered"])
def test_cli_step5_fastq_only(capsys, long_bam, more):
    """BAM '-': the pair equals the --gpu-bgzf run's byte for byte and the default run's text; the
    deferral's cuts and its second pass fire"""
    base, fq0, _ = _step5(capsys, long_bam, "d%d" % len(more), False, *more)
    ref, fq1, _ = _step5(capsys, long_bam, "b%d" % len(more), False, "--gpu-bgzf", "true", *more)
    info, fq2, _ = _step5(capsys, long_bam, "f%d" % len(more), False, "--gpu-fastq", "true", *more)
    assert info["spliced_families"] > 0 and info["spilled_bytes"] > 0 and info.get("deferred_records", 0) > 0
    assert _read(fq2) == _read(fq1)
    assert [gzip.decompress(x) for x in _read(fq2)] == [gzip.decompress(x) for x in _read(fq0)]
    for k in ("records_in", "families", "families_emitted", "records_out", "spliced_families"):
        assert info[k] == ref[k] == base[k], k
    g = info["gpu_fastq"]
    # (both passes' counters; every piece between two cuts of this small input is shorter than a
    # block, so whole blocks are few or none here: test_cli_molecular and the writer tests have them)
    assert g["fallback_blocks"] == 0 and g["blocks"] >= 0 and g["text_bytes"] == 65280 * g["blocks"]
    assert g["compressed_bytes"] <= g["text_bytes"]
    if more:
        assert info["filter"] == base["filter"] and info["filter"]["kept"] < info["filter"]["templates"]


def test_cli_step5_with_a_bam(capsys, long_bam):
    """an output BAM given too: it is the BAM of the run without the option, the pair the --gpu-bgzf run's"""
    _, fq0, b0 = _step5(capsys, long_bam, "wd", True)
    _, fq1, _ = _step5(capsys, long_bam, "wb", False, "--gpu-bgzf", "true")
    info, fq2, b2 = _step5(capsys, long_bam, "wf", True, "--gpu-fastq", "true")
    assert open(b0, "rb").read() == open(b2, "rb").read()
    assert _read(fq2) == _read(fq1)
    assert info["gpu_fastq"]["fallback_blocks"] == 0


def test_cli_molecular(capsys, tmp_path):
    from test_molecular_stream import grouped_bam
    _, p = grouped_bam(tmp_path, n_fam=1500)
    runs = {}
    for tag, more in (("d", ()), ("b", ("--gpu-bgzf", "true")), ("f", ("--gpu-fastq", "true"))):
        fq = [str(tmp_path / ("%s_%d.fq.gz" % (tag, d))) for d in (1, 2)]
        runs[tag] = (_cli(capsys, ["molecular", p, "-", "--fastq1", fq[0], "--fastq2", fq[1], "--threads", "4",
                                   "--chunk-mb", "1"] + list(more)), _read(fq))
    assert runs["f"][1] == runs["b"][1]
    assert [gzip.decompress(x) for x in runs["f"][1]] == [gzip.decompress(x) for x in runs["d"][1]]
    assert runs["f"][0]["records_out"] == runs["d"][0]["records_out"] > 0
    assert runs["f"][0]["gpu_fastq"]["fallback_blocks"] == 0 and runs["f"][0]["gpu_fastq"]["blocks"] > 0

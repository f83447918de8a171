"""The host side of the device FASTQ path, no GPU: bsdc_bgzf_sink_append under an open FastqWriter,
bam.fastq_offsets against the host writer's text family by family, and the size helpers and
argument checks of libbsdc's bsdc_fastq_format / bsdc_bgzf_crc32 (which touch no device)."""
import gzip

import numpy as np
import pytest

from bsseqconsensusreads_amd import bam
import fastq_inputs as FI


def _append(w, d, data: bytes):
    a = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
    assert w.lib.bsdc_bgzf_sink_append(w.sinks[d], a.ctypes.data, len(data)) == 0


def _members(raw: bytes):
    """the BGZF blocks of a file: [(offset, block bytes)]"""
    out, o = [], 0
    while o < len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04" and raw[o + 12:o + 14] == b"BC"
        bs = int.from_bytes(raw[o + 16:o + 18], "little") + 1
        out.append((o, raw[o:o + bs]))
        o += bs
    assert o == len(raw)
    return out


def test_sink_append_between_adds(tmp_path):
    """0, 1, 65279, 65280 and 65281 appended bytes between ordinary adds, a flush, a close: the
    files gunzip to the concatenation in order; the flush's offsets are block boundaries and cut
    the files at what had been added by then."""
    x = FI.make(32, 40, seed=3, written="all")
    recs = [FI.records(x, np.arange(a, b)) for a, b in ((0, 10), (10, 11), (11, 25), (25, 30), (30, 38), (38, 40))]
    texts = [FI.host_text(x, np.arange(a, b), str(tmp_path), "t%d" % a) for a, b in
             ((0, 10), (10, 11), (11, 25), (25, 30), (30, 38), (38, 40))]
    rng = np.random.default_rng(1)
    blobs = [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in (0, 1, 65279, 65280, 65281)]
    p = (str(tmp_path / "a1.fq.gz"), str(tmp_path / "a2.fq.gz"))
    w = bam.FastqWriter(p[0], p[1], 4)
    want = [b"", b""]
    cut = None
    for k in range(6):
        w.add(recs[k], 2)
        for d in range(2):
            want[d] += texts[k][d]
        if k < 5:
            for d in range(2):
                _append(w, d, blobs[k] if d == 0 else blobs[4 - k])
                want[d] += blobs[k] if d == 0 else blobs[4 - k]
        if k == 2:
            cut = (w.flush(2), [len(t) for t in want])
    w.close(2)
    for d in range(2):
        raw = open(p[d], "rb").read()
        assert gzip.decompress(raw) == want[d]
        assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
        assert cut[0][d] in [o for o, _ in _members(raw)]
        assert gzip.decompress(raw[:cut[0][d]]) == want[d][:cut[1][d]]


def test_sink_append_refuses_bad_arguments(tmp_path):
    w = bam.FastqWriter(str(tmp_path / "b1.fq.gz"), str(tmp_path / "b2.fq.gz"), 1)
    try:
        assert w.lib.bsdc_bgzf_sink_append(w.sinks[0], None, 5) != 0
        assert w.lib.bsdc_bgzf_sink_append(w.sinks[0], None, -1) != 0
        assert w.lib.bsdc_bgzf_sink_append(None, None, 0) != 0
        assert w.lib.bsdc_bgzf_sink_append(w.sinks[0], None, 0) == 0
    finally:
        w.close()
    assert gzip.open(str(tmp_path / "b1.fq.gz")).read() == b""


@pytest.mark.parametrize("with_filt", [False, True])
def test_host_offsets_equal_the_writers_text(tmp_path, with_filt):
    """bam.fastq_offsets == the running sum of the bytes bam.write_fastq (format_fastq) writes for
    each family alone, and its total == the size of the text of all kept families at once."""
    x = FI.make(32, 300, seed=2)
    assert set(np.diff(x.names.off)) >= set(range(1, 255))
    assert {0, 1, 2, 7, 30} <= set(x.length.reshape(-1).tolist())
    keep = x.kept(with_filt)
    assert not keep[0] and not keep[-1] and not keep[40:57].any() and keep.any()
    off = bam.fastq_offsets(x.status, x.length, x.filt if with_filt else None, x.names.off)
    size = np.zeros((2, x.n_fam), np.int64)
    for f in np.nonzero(keep)[0]:
        t = FI.host_text(x, np.asarray([f]), str(tmp_path), "f")
        size[:, f] = len(t[0]), len(t[1])
    whole = FI.host_text(x, np.nonzero(keep)[0], str(tmp_path), "w")
    for d in range(2):
        assert off[d].shape == (x.n_fam + 1,) and off[d][0] == 0
        assert np.array_equal(np.diff(off[d]), size[d])
        assert int(off[d][-1]) == len(whole[d])
        for f in np.nonzero(keep)[0][:50]:  # and a family's range of the whole text is its own text
            assert whole[d][off[d][f]:off[d][f + 1]].startswith(b"@" + x.names[int(f)] + b"/%d\n" % (d + 1))


def test_text_bound_and_scratch_size():
    from bsseqconsensusreads_amd import _lib
    lib = _lib.load()
    x = FI.make(32, 300, seed=2)
    bound = lib.bsdc_fastq_text_bound(x.n_fam, int(x.names.off[-1]), x.stride)
    assert bound == int((8 + np.diff(x.names.off)).sum()) + 2 * x.n_fam * x.stride
    for o in bam.fastq_offsets(x.status, x.length, None, x.names.off):
        assert int(o[-1]) <= bound
    assert lib.bsdc_fastq_text_bound(-1, 0, 16) < 0
    assert lib.bsdc_fastq_tmp_bytes(0) >= 16 and lib.bsdc_fastq_tmp_bytes(1_700_000) >= 16 * (1_700_000 // 1024 + 1)
    assert lib.bsdc_fastq_tmp_bytes(-1) < 0
    # no device is touched before the arguments are checked
    assert lib.bsdc_fastq_format(None, None, 0, None, None, None, None, None, None, None, 0, 0, None, None) == -22
    assert lib.bsdc_bgzf_crc32(None, 0, 1, None, None) == -22


def test_sink_take_tail(tmp_path):
    """the tail (what encode or append left short of a block) moves out whole; too small a buffer is refused"""
    w = bam.FastqWriter(str(tmp_path / "c1.fq.gz"), str(tmp_path / "c2.fq.gz"), 1)
    try:
        _append(w, 0, b"abc" * 100)
        buf = np.zeros(65536, np.uint8)
        assert w.lib.bsdc_bgzf_sink_take_tail(w.sinks[0], buf.ctypes.data, 10) < 0
        assert w.lib.bsdc_bgzf_sink_take_tail(w.sinks[0], buf.ctypes.data, 65536) == 300
        assert buf[:300].tobytes() == b"abc" * 100
        assert w.lib.bsdc_bgzf_sink_take_tail(w.sinks[0], buf.ctypes.data, 65536) == 0
        assert w.lib.bsdc_bgzf_sink_take_tail(w.sinks[1], None, 0) == 0
    finally:
        w.close()
    assert gzip.open(str(tmp_path / "c1.fq.gz")).read() == b""


STEP5 = ["step5", "-r", "g.fa", "in.bam"]


@pytest.mark.parametrize("argv,word", [
    (STEP5 + ["out.bam", "--gpu-fastq", "true"], "--fastq1"),
    (STEP5 + ["-", "--fastq1", "a", "--fastq2", "b", "--gpu-fastq", "true", "--gpus", "2"], "--gpus 2"),
    (STEP5 + ["-", "--fastq1", "a", "--fastq2", "b", "--gpu-fastq", "true", "--stream", "false"], "--stream false"),
    (["molecular", "in.bam", "-", "--fastq1", "a", "--fastq2", "b", "--gpu-fastq", "true", "--stream", "false"],
     "--stream false"),
])
def test_cli_refuses_gpu_fastq(capsys, argv, word):
    from bsseqconsensusreads_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--gpu-fastq" in err and word in err, err


def test_cli_accepts_gpu_fastq_with_the_filter():
    from bsseqconsensusreads_amd import cli
    a = cli.parse(STEP5 + ["-", "--fastq1", "a", "--fastq2", "b", "--gpu-fastq", "true", "--filter-min-base-quality", "20",
                           "--filter-min-reads", "2", "1", "1"])
    assert a.gpu_fastq == "true" and cli.filter_params(a).min_reads == (2, 1, 1)
    a = cli.parse(["molecular", "in.bam", "o.bam", "--fastq1", "a", "--fastq2", "b", "--gpu-fastq", "true"])
    assert a.gpu_fastq == "true"
    assert cli.parse(STEP5 + ["out.bam"]).gpu_fastq == "false"


def test_stream_refuses_gpu_fastq_without_its_needs(tmp_path):
    """the Python surface: no FASTQ pair, and a runner stream"""
    from bsseqconsensusreads_amd import stream
    job = stream.StreamJob("in.bam", "g.fa", str(tmp_path / "o.bam"), None, gpu_fastq=True)
    with pytest.raises(ValueError, match="gpu_fastq"):
        stream.run(job, engine=object())
    job = stream.StreamJob("in.bam", "g.fa", None, ("a", "b"), gpu_fastq=True)
    with pytest.raises(ValueError, match="gpu_fastq"):
        stream.run(job, runner=object())

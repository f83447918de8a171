"""The BGZF inflate's host twin (libbsdc bsdc_bgzf_inflate_host: the kernel's own decoding functions
run sequentially, csrc/bsdc_inflate.hip) against zlib on the blocks of tests/inflate_inputs.py --
valid ones byte for byte, corrupt ones by status code, guard bytes around every block's window
intact -- and the reader's inflater hook (libbsdc_io bsdc_bam_stream_set_inflater) with a zlib
stand-in.  No GPU: the corrupt inputs go through here before tests/test_gpu_inflate.py runs them
on one."""
import ctypes as C
import zlib

import numpy as np
import pytest

from bsseqconsensusreads_amd import _lib as L
from bsseqconsensusreads_amd import bam, cli

import inflate_inputs as I

GUARD = 64


def layout(blocks):
    """(comp bytes, block table, out size): the blocks' windows GUARD bytes apart."""
    comp = b"".join(b.comp for b in blocks)
    d = (L.InflateBlockC * len(blocks))()
    o, dst = 0, GUARD
    for i, b in enumerate(blocks):
        d[i].src, d[i].clen, d[i].isize, d[i].dst = o, len(b.comp), b.isize, dst
        o += len(b.comp)
        dst += b.isize + GUARD
    return comp, d, dst


def check(blocks, d, out, status, twin_status=None):
    """status and bytes of every block; nothing outside the valid blocks' windows was written."""
    seen = np.ones(out.shape[0], bool)
    for i, b in enumerate(blocks):
        lo = int(d[i].dst)
        if b.want is not None:
            assert status[i] == 0, (b.name, int(status[i]))
            assert out[lo:lo + b.isize].tobytes() == b.want, b.name
            seen[lo:lo + b.isize] = False
        else:
            assert status[i] == b.code, (b.name, int(status[i]), b.code)
        if twin_status is not None:
            assert status[i] == twin_status[i], b.name
    assert (out[seen] == 0xA5).all(), "bytes outside the valid blocks' windows were written"


def host_inflate(blocks):
    lib = L.load()
    comp, d, n_out = layout(blocks)
    ca = np.frombuffer(comp + b"\0", np.uint8)
    out = np.full(n_out, 0xA5, np.uint8)
    status = np.full(len(blocks), -1, np.int32)
    assert lib.bsdc_bgzf_inflate_host(ca.ctypes.data, len(comp), d, len(blocks), out.ctypes.data, n_out,
                                      status.ctypes.data) == 0
    return d, out, status


def test_valid_blocks_equal_zlib():
    v = I.valid()
    assert len(v) > 60
    check(v, *host_inflate(v))
    m = I.many()
    assert len(m) == 260 and sum(b.isize == 0 for b in m) > 20
    check(m, *host_inflate(m))


def test_corrupt_blocks_get_their_codes_and_zlib_rejects_them_too():
    x = I.corrupt()
    assert {b.code for b in x} >= set(range(1, 13))
    for b in x:  # the fixtures hold their edge: zlib rejects the bytes, or disagrees with the isize
        try:
            assert len(I.ref(b.comp)) != b.isize, b.name
        except zlib.error:
            pass
    check(x, *host_inflate(x))


def test_valid_blocks_between_corrupt_ones_stay_exact():
    v, x = I.valid(), I.corrupt()
    mixed = []
    for i, b in enumerate(x):
        mixed += [b, v[(5 * i) % len(v)]]
    check(mixed, *host_inflate(mixed))


def test_descriptors_outside_the_buffers_are_refused():
    lib = L.load()
    b = I.valid()[0]
    ca = np.frombuffer(b.comp, np.uint8)
    out = np.full(b.isize + 2 * GUARD, 0xA5, np.uint8)
    bad = [(-1, len(b.comp), b.isize, GUARD), (1, len(b.comp), b.isize, GUARD), (0, -1, b.isize, GUARD),
           (0, len(b.comp), 65537, 0), (0, len(b.comp), -1, GUARD), (0, len(b.comp), b.isize, -1),
           (0, len(b.comp), b.isize, 2 * GUARD + 1), (0, 1 << 30, b.isize, GUARD)]
    d = (L.InflateBlockC * len(bad))()
    for i, t in enumerate(bad):
        d[i].src, d[i].clen, d[i].isize, d[i].dst = t
    status = np.full(len(bad), -1, np.int32)
    assert lib.bsdc_bgzf_inflate_host(ca.ctypes.data, len(b.comp), d, len(bad), out.ctypes.data, out.shape[0],
                                      status.ctypes.data) == 0
    assert (status == L.INFLATE_ERANGE).all() and (out == 0xA5).all()


# ---- the reader's hook, with zlib standing in for the GPU ----------------------------------------
class ZlibInflater:
    """bam.GpuInflate's interface on the CPU: the hook's blocks through zlib."""

    def __init__(self, fail_at=None, corrupt_at=None):
        self.blocks = self.fills = 0
        self.fail_at, self.corrupt_at = fail_at, corrupt_at
        self.callback = bam.INFLATE_FN(self._call)

    def _call(self, user, comp, n_comp, blk, nblk, out, n_out):
        c = np.ctypeslib.as_array(C.cast(comp, C.POINTER(C.c_uint8)), shape=(n_comp,))
        o = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(n_out,))
        d = C.cast(blk, C.POINTER(L.InflateBlockC))
        assert nblk > 0 and d[0].dst == 0
        for i in range(nblk):
            b = d[i]
            assert b.isize > 0 and 0 <= b.src and b.src + b.clen <= n_comp and b.dst + b.isize <= n_out
            data = zlib.decompress(c[b.src:b.src + b.clen].tobytes(), -15)
            assert len(data) == b.isize
            o[b.dst:b.dst + b.isize] = np.frombuffer(data, np.uint8)
            if self.corrupt_at == self.blocks:
                o[b.dst + b.isize // 2] ^= 1
            self.blocks += 1
        self.fills += 1
        return 1 if self.fail_at is not None and self.blocks > self.fail_at else 0


@pytest.fixture(scope="module")
def sorted_bam(tmp_path_factory):
    from test_stream import _sorted_bam
    return _sorted_bam(tmp_path_factory.mktemp("inflate"), n_fam=1500)[1]


def nonempty_blocks(path):
    data, o, n = open(path, "rb").read(), 0, 0
    while o < len(data):
        bsize = int.from_bytes(data[o + 16:o + 18], "little") + 1
        n += int.from_bytes(data[o + bsize - 4:o + bsize], "little") > 0
        o += bsize
    return n


def _chunks(path, **kw):
    out = []
    for ch in bam.stream_chunks(path, 2, kw.pop("chunk_bytes", 60_000), **kw):
        raw = ch.decode(2)[1]
        out.append((raw.n, raw.pos.copy(), raw.flag.copy(), raw.seq.copy(), raw.qual.copy(),
                    [raw.names[int(k)] for k in raw.name_id]))
    return out


def _same(a, b):
    assert len(a) == len(b) and len(a) > 3
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[5] == y[5]
        for k in range(1, 5):
            assert np.array_equal(x[k], y[k])


@pytest.mark.parametrize("read_size", [8 << 20, 20_000])
def test_hooked_stream_yields_the_same_chunks(sorted_bam, read_size):
    """every block goes through the hook (the header's too: setting it rewinds the stream), also
    when the fills are small and blocks straddle them"""
    z = ZlibInflater()
    _same(_chunks(sorted_bam, read_size=read_size), _chunks(sorted_bam, read_size=read_size, inflater=z))
    assert z.blocks == nonempty_blocks(sorted_bam)
    assert z.fills == 1 if read_size > 1 << 20 else z.fills > 10
    a = list(bam.stream_bam(sorted_bam, 2, 60_000, read_size=read_size))
    b = list(bam.stream_bam(sorted_bam, 2, 60_000, read_size=read_size, inflater=ZlibInflater()))
    assert len(a) == len(b) and all(x[1].n == y[1].n and np.array_equal(x[1].seq, y[1].seq) for x, y in zip(a, b))


def test_hooked_range_stream_yields_the_same_chunks(sorted_bam):
    """bsdc_bam_stream_open_range with bytes to skip in the first block and to drop from the last"""
    c1 = bam.find_cut(sorted_bam, 0, threads=2, slack=2000)
    c2 = bam.find_cut(sorted_bam, c1["end"][0] + 1, threads=2, slack=2000)
    assert c1 is not None and c2 is not None
    rng = c1["start"] + c2["end"]
    assert rng[1] > 0 and rng[3] > 0 and rng[2] > rng[0]
    z = ZlibInflater()
    a = _chunks(sorted_bam, rng=rng, read_size=30_000, chunk_bytes=20_000)
    _same(a, _chunks(sorted_bam, rng=rng, read_size=30_000, chunk_bytes=20_000, inflater=z))
    assert z.blocks > 2 and 0 < sum(x[0] for x in a)


@pytest.mark.parametrize("how", ["fail", "corrupt"])
def test_a_failing_or_lying_inflater_is_a_corrupt_block(sorted_bam, how):
    z = ZlibInflater(fail_at=3) if how == "fail" else ZlibInflater(corrupt_at=3)
    with pytest.raises(OSError, match="corrupt BGZF block"):
        _chunks(sorted_bam, read_size=20_000, inflater=z)


def test_hooked_stream_of_a_truncated_file_fails_loudly(sorted_bam, tmp_path):
    data = open(sorted_bam, "rb").read()
    t = str(tmp_path / "t.bam")
    open(t, "wb").write(data[: len(data) * 2 // 3])
    with pytest.raises(OSError, match="truncated BGZF block"):
        _chunks(t, read_size=8192, inflater=ZlibInflater())


def test_inflater_is_set_before_the_first_chunk(sorted_bam):
    lib, st, h = bam._load(), bam._P(), bam._P()
    assert lib.bsdc_bam_stream_open(sorted_bam.encode(), 2, 20_000, C.byref(st)) == 0
    try:
        assert lib.bsdc_bam_stream_next_raw(st, 20_000, 2000, C.byref(h)) == 0 and h
        assert lib.bsdc_bam_stream_set_inflater(st, ZlibInflater().callback, None) == -22
        lib.bsdc_bam_stream_recycle(st, h)
    finally:
        lib.bsdc_bam_stream_close(st)


def test_cli_option():
    assert cli.parse(["step5", "-r", "g.fa", "in.bam", "out.bam"]).gpu_inflate == "false"
    assert cli.parse(["step5", "-r", "g.fa", "in.bam", "out.bam", "--gpu-inflate", "true"]).gpu_inflate == "true"
    assert cli.parse(["molecular", "in.bam", "out.bam", "--gpu-inflate", "true"]).gpu_inflate == "true"
    with pytest.raises(SystemExit):
        cli.parse(["step5", "-r", "g.fa", "in.bam", "out.bam", "--gpu-inflate", "true", "--gpus", "2"])
    from bsseqconsensusreads_amd import stream
    assert stream.StreamJob("a", "b", "c").gpu_inflate is False
    assert [f.name for f in stream.dataclasses.fields(stream.StreamJob)][-1] == "gpu_inflate"

"""The BGZF inflate kernel (libbsdc bsdc_bgzf_inflate, csrc/bsdc_inflate.hip) against zlib on the
blocks of tests/inflate_inputs.py, its corrupt blocks against the host twin's status codes (the
same lists tests/test_inflate_host.py runs on the CPU first), bam.GpuInflate on the project's own
writer's blocks, and `cli step5 | molecular --gpu-inflate true` against the same runs without it:
byte-identical files."""
import numpy as np
import pytest
import torch

from bsseqconsensusreads_amd import _lib as L
from bsseqconsensusreads_amd import bam, cli
from helpers import assert_bam_matches_oracle

import inflate_inputs as I
from test_inflate_host import check, host_inflate, layout, nonempty_blocks

pytestmark = pytest.mark.gpu


class Device:
    """the launch's buffers on the GPU, kept between launches"""

    def __init__(self, blocks, lay=None):  # lay: a (comp, table, out size) other than layout()'s
        comp, d, self.n_out = lay or layout(blocks)
        self.blocks, self.d, self.n_comp = blocks, d, len(comp)
        self.comp = torch.from_numpy(np.frombuffer(comp + b"\0", np.uint8).copy()).cuda()
        self.blk = torch.from_numpy(np.frombuffer(bytes(d), np.uint8).copy()).cuda()
        self.out = torch.empty(self.n_out, dtype=torch.uint8, device="cuda")
        self.status = torch.empty(len(blocks), dtype=torch.int32, device="cuda")

    def run(self):
        self.out.fill_(0xA5)
        self.status.fill_(-1)
        assert L.load().bsdc_bgzf_inflate(self.comp.data_ptr(), self.n_comp, self.blk.data_ptr(), len(self.blocks),
                                          self.out.data_ptr(), self.n_out, self.status.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return self.d, self.out.cpu().numpy(), self.status.cpu().numpy()


def test_valid_blocks_equal_zlib(engine):
    v = I.valid()
    check(v, *Device(v).run())


def test_260_blocks_twice_on_the_same_buffers(engine):
    m = I.many()
    dev = Device(m)
    check(m, *dev.run())
    check(m, *dev.run())


def test_corrupt_blocks_get_the_host_twins_codes(engine):
    """corrupt blocks between valid ones: the twin's codes, the neighbours exact, the guards intact"""
    v, x = I.valid(), I.corrupt()
    mixed = []
    for i, b in enumerate(x):
        mixed += [b, v[(5 * i) % len(v)]]
    _, _, twin = host_inflate(mixed)
    check(mixed, *Device(mixed).run(), twin_status=twin)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from test_gpu_stream import _inputs
    return _inputs(tmp_path_factory.mktemp("gpuinflate"), "C2", 1500, 0.0, 23)


def test_gpu_inflate_on_the_writers_own_blocks(engine, inputs, tmp_path):
    """a small step-5 output BAM written by the project's writer (GPU-deflated blocks too), read
    back through bam.GpuInflate == the host inflate"""
    inp, fa = inputs
    for gz in (False, True):
        out = str(tmp_path / ("o%d.bam" % gz))
        bam.step5_stream(inp, fa, out, engine=engine, threads=4, level=5, chunk_bytes=200_000, gpu_bgzf=gz)
        g = bam.GpuInflate(engine.device)
        a = list(bam.stream_bam(out, 2, 100_000))
        b = list(bam.stream_bam(out, 2, 100_000, inflater=g))
        assert g.error is None and g.blocks == nonempty_blocks(out) and g.bytes_out > g.bytes_in > 0
        assert len(a) == len(b) > 0
        for (_, x), (_, y) in zip(a, b):
            assert x.n == y.n and np.array_equal(x.seq, y.seq) and np.array_equal(x.qual, y.qual)


def _cli(argv, capsys):
    import json
    assert cli.main(argv) == 0
    return json.loads(capsys.readouterr().err.strip().splitlines()[-1])


def test_cli_step5_writes_the_same_files(inputs, tmp_path, capsys):
    inp, fa = inputs
    p = lambda n: str(tmp_path / n)  # noqa: E731
    base = ["step5", "-r", fa, inp]
    tail = ["--stream", "true", "--threads", "4", "--chunk-mb", "1"]
    ia = _cli(base + [p("a.bam"), "--fastq1", p("a1.fq.gz"), "--fastq2", p("a2.fq.gz")] + tail, capsys)
    ib = _cli(base + [p("b.bam"), "--fastq1", p("b1.fq.gz"), "--fastq2", p("b2.fq.gz"), "--gpu-inflate", "true"] + tail,
              capsys)
    assert "gpu_inflate" not in ia and ib["gpu_inflate"]["blocks"] == nonempty_blocks(inp)
    for x in (".bam", "1.fq.gz", "2.fq.gz"):
        assert open(p("a" + x), "rb").read() == open(p("b" + x), "rb").read(), x
    assert assert_bam_matches_oracle(p("b.bam"), inp, fa, "gpu inflate") == ib["records_out"] > 0
    _cli(base + [p("c.bam"), "--gpu-inflate", "true", "--gpu-bgzf", "true"] + tail, capsys)
    _, ra = bam.read_bam(p("a.bam"))
    _, rc = bam.read_bam(p("c.bam"))
    assert ra.n == rc.n and np.array_equal(ra.seq, rc.seq) and np.array_equal(ra.qual, rc.qual)


def test_step5_stream_with_small_chunks_and_fills(engine, inputs, tmp_path):
    """60 KB chunks and fills smaller than the file: many hook calls, the same bytes"""
    inp, fa = inputs
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    kw = dict(engine=engine, threads=4, level=5, chunk_bytes=60_000, slack=2000, read_size=50_000)
    ia = bam.step5_stream(inp, fa, a, **kw)
    ib = bam.step5_stream(inp, fa, b, gpu_inflate=True, **kw)
    assert ia["chunks"] == ib["chunks"] > 3 and ib["gpu_inflate"]["fills"] > 3
    assert ib["gpu_inflate"]["blocks"] == nonempty_blocks(inp)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_cli_molecular_writes_the_same_file(engine, tmp_path, capsys):
    from test_molecular_stream import grouped_bam
    _, inp = grouped_bam(tmp_path, n_fam=1500, messy=0.1, seed=29)
    p = lambda n: str(tmp_path / n)  # noqa: E731
    tail = ["--threads", "4", "--chunk-mb", "1"]
    _cli(["molecular", inp, p("a.bam")] + tail, capsys)
    ib = _cli(["molecular", inp, p("b.bam"), "--gpu-inflate", "true"] + tail, capsys)
    assert ib["gpu_inflate"]["blocks"] == nonempty_blocks(inp)
    assert open(p("a.bam"), "rb").read() == open(p("b.bam"), "rb").read()
    # (--chunk-mb counts whole MiB: the 60 KB chunks go through the call the CLI makes)
    ic = bam.molecular_stream(inp, p("c.bam"), engine=engine, threads=4, chunk_bytes=60_000, gpu_inflate=True)
    assert ic["chunks"] > 3 and ic["gpu_inflate"]["blocks"] == nonempty_blocks(inp)
    assert open(p("a.bam"), "rb").read() == open(p("c.bam"), "rb").read()

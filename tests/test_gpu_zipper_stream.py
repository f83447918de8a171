"""cli zipper --stream true on the GPU (csrc/bsdc_zipper.hip's bsdc_zip_gather, zipper_stream.py;
DESIGN.md 3.11 "Streaming", 8.12): the gather against its host twin byte for byte, the streaming
driver against the host twins' file, and the command end to end with step 5 behind it."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import zipper_ref as ZR
import zipper_stream_inputs as SI
from bsseqconsensusreads_amd import cli, zipper, zipper_stream
from test_gpu_zipper import _fasta
from test_zipper_host import split_input

pytestmark = pytest.mark.gpu
GUARD = 0xA5
PAD = 256  # guard bytes behind dst + cap and behind off[n]


def _dev(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.size else np.zeros(8, np.uint8)).to(dev)


def device_gather(engine, order, off, ln, src, cap, shift=0):
    """bsdc_zip_gather -> (rc, off [n + 1 + guard words], the buffer of shift + cap + PAD bytes prefilled with GUARD)"""
    lib, dev = engine.lib, engine.device
    n = int(order.shape[0])
    pad = lambda x, dt: np.ascontiguousarray(x, dt) if n else np.zeros(1, dt)  # noqa: E731
    o, so, sl = pad(order, np.uint32), pad(off, np.int64), pad(ln, np.int32)
    d_o, d_so, d_sl, d_src = _dev(o, dev), _dev(so, dev), _dev(sl, dev), _dev(src, dev)
    buf = torch.full((shift + cap + PAD,), GUARD, dtype=torch.uint8, device=dev)
    d_off = torch.full((n + 1 + 4,), -7, dtype=torch.int64, device=dev)
    tmp = torch.empty(int(lib.bsdc_zip_gather_tmp_bytes(n)), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    rc = lib.bsdc_zip_gather(d_o.data_ptr(), o.ctypes.data, n, d_so.data_ptr(), so.ctypes.data, d_sl.data_ptr(), sl.ctypes.data,
                             d_src.data_ptr(), int(src.shape[0]), d_off.data_ptr(), buf.data_ptr() + shift, cap, tmp.data_ptr(),
                             C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc, d_off.cpu().numpy(), buf.cpu().numpy()


@pytest.mark.parametrize("n", [0, 1, 2, 14, 3000])
def test_gather_equals_the_twin(engine, n):
    src, off, ln = SI.gather_case(n)
    for name, order in SI.gather_orders(n).items():
        cap = int(ln.sum())
        want_off, want = zipper_stream.gather_host(order, off, ln, src, cap=cap)
        for shift in (0, 4, 8):
            rc, got_off, buf = device_gather(engine, order, off, ln, src, cap, shift)
            assert rc == 0, engine.lib.bsdc_zip_last_error().decode()
            assert np.array_equal(got_off[:n + 1], want_off) and (got_off[n + 1:] == -7).all(), (name, shift)
            bad = np.nonzero(buf[shift:shift + cap] != want[:cap])[0]
            assert bad.size == 0, "%s shift %d: byte %d (record %d)" % (
                name, shift, bad[0], int(np.searchsorted(want_off, bad[0], "right")) - 1)
            assert (buf[:shift] == GUARD).all() and (buf[shift + cap:] == GUARD).all(), (name, shift)


def test_gather_refusals(engine):
    src, off, ln = SI.gather_case(14)
    order = np.arange(14, dtype=np.uint32)
    err = lambda: engine.lib.bsdc_zip_last_error().decode()  # noqa: E731
    rc, _, buf = device_gather(engine, order, off, ln, src, int(ln.sum()) - 1)
    assert rc == -22 and "below the records' bytes" in err() and (buf == GUARD).all()
    bad = order.copy()
    bad[2] = 99
    rc, _, buf = device_gather(engine, bad, off, ln, src, int(ln.sum()))
    assert rc == -22 and "order[2] is not below n" in err() and (buf == GUARD).all()
    far = off.copy()
    far[13] += 8
    rc, _, buf = device_gather(engine, order, far, ln, src, int(ln.sum()))
    assert rc == -22 and "leave src" in err() and (buf == GUARD).all()
    assert engine.lib.bsdc_zip_gather_tmp_bytes(-1) < 0


@pytest.mark.parametrize("which", ["third", "template"])
@pytest.mark.parametrize("name", ["ties", "contigs3"])
def test_stream_on_the_device_equals_the_host_twins(engine, tmp_path, name, which):
    a, u = SI.case(name)
    p = lambda x: str(tmp_path / x)  # noqa: E731
    SI.write_bam(p("a.bam"), SI.TEXT_A, SI.REFS, b"".join(a))
    SI.write_bam(p("u.bam"), SI.TEXT_U, [], b"".join(u))
    kw = dict(tags_to_reverse=["Consensus"], tags_to_remove=["RX"], level=1)
    want = zipper.zipper(p("a.bam"), p("u.bam"), p("h.bam"), host=True, **kw)
    chunk = SI.budget(a, u) // 3 + 1 if which == "third" else 40
    info = zipper.zipper(p("a.bam"), p("u.bam"), p("o.bam"), stream=True, chunk_bytes=chunk, tmp_dir=str(tmp_path), **kw)
    assert ZR.read_bam(p("o.bam"))[:3] == ZR.read_bam(p("h.bam"))[:3]
    for k in ("records_in", "unmapped_records_in", "records_out", "unmapped_dropped", "templates_without_aligned", "raw_bytes"):
        assert info[k] == want[k], k
    templates = len({ZR.parse_records(r)[0]["name"] for r in a})
    assert info["runs"] == templates if which == "template" else info["runs"] in (3, 4)
    assert info["spill_bytes"] == info["raw_bytes"] and info["merge_rounds"] >= 1 and info["peak_record_bytes"] > 0
    host = zipper.zipper(p("a.bam"), p("u.bam"), p("s.bam"), stream=True, host=True, chunk_bytes=chunk, tmp_dir=str(tmp_path), **kw)
    assert {k: v for k, v in host.items() if k != "compressed_bytes"} == {k: v for k, v in info.items() if k != "compressed_bytes"}


def test_cli_stream_end_to_end_and_step5(engine, tmp_path):
    text, refs, recs, aligned, unmapped = split_input(tmp_path, "C2")
    p = lambda n: str(tmp_path / n)  # noqa: E731
    ZR.write_bam(p("a.bam"), text.replace("SO:coordinate", "SO:unsorted"), refs, b"".join(aligned))
    ZR.write_bam(p("u.bam"), "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:A\tLB:L\n", [], b"".join(unmapped))  # (step-1 order: ALIGNED's)
    base = ["zipper", p("a.bam"), p("u.bam")]
    assert cli.main(base + [p("w.bam"), "--level", "1", "--stream", "false"]) == 0
    # the Python API takes the small chunk that --chunk-mb cannot state; cli with 1 MiB is one run on this input
    info = zipper.zipper(p("a.bam"), p("u.bam"), p("o.bam"), level=1, stream=True, chunk_bytes=len(b"".join(aligned)) // 5,
                         tmp_dir=str(tmp_path))
    assert info["runs"] >= 5
    assert cli.main(base + [p("c.bam"), "--level", "1", "--stream", "true", "--chunk-mb", "1", "--tmp-dir", str(tmp_path),
                            "--info", p("i.json")]) == 0
    whole = ZR.read_bam(p("w.bam"))[:3]
    assert ZR.read_bam(p("o.bam"))[:3] == whole and ZR.read_bam(p("c.bam"))[:3] == whole
    assert json.load(open(p("i.json")))["runs"] >= 1
    fa = _fasta(tmp_path, "C2")
    s5 = ["step5", "--reference", fa, "--threads", "4", "--compression", "1", "--stream", "true"]
    assert cli.main(s5 + [p("w.bam"), p("c_whole.bam")]) == 0
    assert cli.main(s5 + [p("o.bam"), p("c_stream.bam")]) == 0
    assert open(p("c_stream.bam"), "rb").read() == open(p("c_whole.bam"), "rb").read()

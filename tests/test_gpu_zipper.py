"""cli zipper on the GPU (csrc/bsdc_zipper.hip): bsdc_zip_sort and
bsdc_zip_format against their host twins on the edge inputs, the command end to end on a split
step-5 input, and step 5 on the file it writes."""
import ctypes as C

import numpy as np
import pytest
import torch

import zipper_inputs as ZI
import zipper_ref as ZR
from bsseqconsensusreads_amd import bam, cli, synth, zipper
from bsseqconsensusreads_amd import records as R
from test_zipper_host import GUARD, prepare, rule6, split_input, twin

pytestmark = pytest.mark.gpu
PAD = 256  # guard bytes behind dst + cap


def _dev(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.size else np.zeros(8, np.uint8)).to(dev)


@pytest.mark.parametrize("name", ZI.SORTS)
def test_sort_equals_the_twin(engine, name):
    lib, dev = engine.lib, engine.device
    ref, pos, flag = ZI.sort_case(name, lib.bsdc_zip_sort_tile())
    n = int(ref.shape[0])
    keys, pay = zipper.sort_keys(ref, pos, flag), (np.arange(n, dtype=np.uint32) * 5 + 1)
    for max_ref, max_pos in ((int(ref.max()) if n else 0, int(pos.max()) if n else 0), (1 << 20, (1 << 31) - 2)):
        want_k, want_v = zipper.sort_host(keys, pay, max_ref, max_pos)
        dk, dv = _dev(keys, dev), _dev(pay, dev)
        tmp = torch.full((int(lib.bsdc_zip_sort_tmp_bytes(n)) + PAD,), GUARD, dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev)
        rc = lib.bsdc_zip_sort(dk.data_ptr(), dv.data_ptr(), n, max_ref, max_pos, tmp.data_ptr(), C.c_void_p(s.cuda_stream))
        s.synchronize()
        assert rc == 0, lib.bsdc_zip_last_error().decode()
        assert np.array_equal(dk.cpu().numpy().view(np.uint64)[:n], want_k), name
        assert np.array_equal(dv.cpu().numpy().view(np.uint32)[:n], want_v), name
        assert (tmp[-PAD:] == GUARD).all(), name + ": scratch past bsdc_zip_sort_tmp_bytes"


def device_format(engine, a, t, tags, idx, cap, dst_shift=0):
    """bsdc_zip_format -> (rc, off, the buffer of dst_shift + cap + PAD bytes, prefilled with GUARD)"""
    lib, dev = engine.lib, engine.device
    n = t.n
    one = np.zeros(1, zipper._lib.ZIP_REC)
    d_idx, d_tab = _dev(idx if n else np.zeros(1, np.uint32), dev), _dev(t.tab if n else one, dev)
    d_rec, d_part = _dev(a.buf, dev), _dev(t.part, dev)
    buf = torch.full((dst_shift + cap + PAD,), GUARD, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    tmp = torch.empty(int(lib.bsdc_zip_format_tmp_bytes(n)), dtype=torch.uint8, device=dev)
    tab_h = np.ascontiguousarray(t.tab) if n else one
    s = torch.cuda.current_stream(dev)
    rc = lib.bsdc_zip_format(d_idx.data_ptr(), n, d_tab.data_ptr(), tab_h.ctypes.data, d_rec.data_ptr(), a.buf.ctypes.data,
                             int(a.buf.shape[0]), d_part.data_ptr(), t.part.ctypes.data, int(t.part.shape[0]), C.byref(tags),
                             off.data_ptr(), buf.data_ptr() + dst_shift, cap, tmp.data_ptr(), C.c_void_p(s.cuda_stream))
    s.synchronize()
    return rc, off.cpu().numpy(), buf.cpu().numpy()


@pytest.mark.parametrize("setting", sorted(ZI.SETTINGS))
@pytest.mark.parametrize("name", ZI.NAMES)
def test_format_equals_the_twin(engine, name, setting):
    ar, ur = ZI.case(name)
    want_off, want, _ = twin(ar, ur, setting)
    a, t, tags, _ = prepare(ar, ur, setting)
    _, idx = zipper.sort_host(t.keys, t.idx, t.max_ref, t.max_pos)
    cap = zipper.bound(t.tab)  # exactly the bound: the guard starts at dst + cap
    for shift in ((0, 1, 2, 3) if name == "all" else (0,)):
        rc, off, buf = device_format(engine, a, t, tags, idx, cap, shift)
        assert rc == 0, engine.lib.bsdc_zip_last_error().decode()
        assert np.array_equal(off, want_off), name
        total = int(off[-1])
        got = buf[shift:shift + total]
        bad = np.nonzero(got != want[:total])[0]
        assert bad.size == 0, "%s / %s: byte %d (record %d): %d vs %d" % (
            name, setting, bad[0], int(np.searchsorted(off, bad[0], "right")) - 1, got[bad[0]], want[bad[0]])
        assert (buf[:shift] == GUARD).all() and (buf[shift + total:] == GUARD).all(), name + ": bytes outside the records"


def test_launcher_refusals(engine):
    ar, ur = ZI.case("names")
    a, t, tags, _ = prepare(ar, ur, "none")
    err = lambda: engine.lib.bsdc_zip_last_error().decode()  # noqa: E731
    rc, _, buf = device_format(engine, a, t, tags, t.idx, zipper.bound(t.tab) - 1)
    assert rc == -22 and "below bsdc_zip_bytes_bound" in err() and (buf == GUARD).all()
    ea, eu, word = ZI.error_case("unknown_type")
    a, t, tags, _ = prepare(ea, eu, "none")
    rc, _, buf = device_format(engine, a, t, tags, t.idx, zipper.bound(t.tab))
    assert rc == -22 and "(read %s)" % word in err() and "unknown type" in err() and (buf == GUARD).all()
    assert engine.lib.bsdc_zip_sort_tmp_bytes(-1) < 0 and engine.lib.bsdc_zip_format_tmp_bytes(-1) < 0


def _fasta(tmp, cfg, n_fam=200, seed=5):
    s = synth.generate(cfg, n_fam, seed=seed, device="cpu", genome_len=100_000)  # (split_input's set)
    codes = R.unpack_nibbles(s.ref.packed, s.ref.n_nibbles)
    fa = str(tmp / "g.fa")
    open(fa, "w").write(">%s\n%s\n" % (s.ref.names[0], R.NT16_TO_ASCII[codes].tobytes().decode()))
    return fa


def test_cli_end_to_end_and_step5(engine, tmp_path):
    text, refs, recs, aligned, unmapped = split_input(tmp_path, "C2")
    p = lambda n: str(tmp_path / n)  # noqa: E731
    ZR.write_bam(p("a.bam"), text.replace("SO:coordinate", "SO:unsorted"), refs, b"".join(aligned))
    ZR.write_bam(p("u.bam"), "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:A\tLB:L\n", [], b"".join(unmapped[::-1]))
    assert cli.main(["zipper", p("a.bam"), p("u.bam"), p("o.bam"), "--threads", "4", "--level", "1", "--info", p("i.json")]) == 0
    want = rule6(recs)
    otext, orefs, data, nblk = ZR.read_bam(p("o.bam"))  # (zlib inflates every block; CRC32 and ISIZE hold; one EOF block)
    assert otext.split("\n")[0] == "@HD\tVN:1.6\tSO:coordinate" and orefs == refs and nblk > 2
    assert data == b"".join(ZR.encode(r) for r in want)
    import json
    info = json.load(open(p("i.json")))
    assert info["records_in"] == info["records_out"] == len(want) and info["raw_bytes"] == len(data)
    assert info["unmapped_dropped"] == 0 and info["templates_without_aligned"] == 0
    # the host twins' file holds the same stream
    zipper.zipper(p("a.bam"), p("u.bam"), p("h.bam"), threads=2, level=1, host=True)
    assert ZR.read_bam(p("h.bam"))[:3] == (otext, orefs, data)
    _, back = bam.read_bam(p("o.bam"), threads=4)
    assert back.n == len(want) and np.array_equal(back.pos, [r["pos"] for r in want])
    assert np.array_equal(back.flag, [r["flag"] for r in want])
    assert [back.names[int(k)] for k in back.name_id] == [r["name"] for r in want]
    assert [back.aux[k] for k in range(back.n)] == [r["aux"] for r in want]
    # a tag list reaches the kernel: Consensus flips nothing here (no per-base tags), a removal removes
    assert cli.main(["zipper", p("a.bam"), p("u.bam"), p("r.bam"), "--tags-to-remove", "RX", "--tags-to-reverse", "Consensus",
                     "--level", "1"]) == 0
    got = ZR.parse_records(ZR.read_bam(p("r.bam"))[2])
    assert [g["aux"] for g in got] == [w["aux"].replace(ZI.tag("RX", "Z", "ACG-TTA"), b"") for w in want]
    # an aligned read without a partner fails the command
    ZR.write_bam(p("u2.bam"), "@HD\tVN:1.6\n", [], b"".join(unmapped[1:]))
    assert cli.main(["zipper", p("a.bam"), p("u2.bam"), p("x.bam")]) == 1
    # together with step 5: the file is what step 5 wants
    fa = _fasta(tmp_path, "C2")
    ZR.write_bam(p("e.bam"), text, refs, b"".join(ZR.encode(r) for r in want))
    hdr, raw = bam.read_bam(p("e.bam"), threads=4)
    bam.write_bam(p("orig.bam"), hdr, bam.records_to_bam(raw), level=1, threads=4)
    base = ["step5", "--reference", fa, "--threads", "4", "--compression", "1", "--stream", "true"]
    assert cli.main(base + [p("orig.bam"), p("c_orig.bam")]) == 0
    assert cli.main(base + [p("o.bam"), p("c_zip.bam")]) == 0
    assert open(p("c_zip.bam"), "rb").read() == open(p("c_orig.bam"), "rb").read()
    assert bam.read_bam(p("c_zip.bam"), threads=2)[1].n > 100

"""cli zipper --stream true on the host twins (zipper_stream.py; DESIGN.md 3.11 "Streaming"): the
file of the whole-file path and of the pure-Python restatement at every chunk size, the order
errors, the memory bound, the temporary files, the prefix scan and bsdc_zip_gather_host."""
import functools
import os

import numpy as np
import pytest

import zipper_inputs as ZI
import zipper_ref as ZR
import zipper_stream_inputs as SI
from bsseqconsensusreads_amd import _lib, cli, zipper, zipper_stream

GUARD = 0xA5
SETTINGS = {"none": {}, "tags": dict(tags_to_reverse=["Consensus"], tags_to_remove=["RX"])}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("zs")


@functools.lru_cache(maxsize=None)
def _files(work, name):
    a, u = SI.case(name)
    pa, pu = str(work / (name + ".a.bam")), str(work / (name + ".u.bam"))
    SI.write_bam(pa, SI.TEXT_A, SI.REFS, b"".join(a))
    SI.write_bam(pu, SI.TEXT_U, [], b"".join(u))
    return pa, pu, SI.budget(a, u)


@functools.lru_cache(maxsize=None)
def _whole(work, name, setting):
    """the whole-file path's file read back, its info, and the restatement's records"""
    pa, pu, _ = _files(work, name)
    po = str(work / ("%s.%s.whole.bam" % (name, setting)))
    info = zipper.zipper(pa, pu, po, host=True, level=1, **SETTINGS[setting])
    a, u = SI.case(name)
    kw = dict(reverse=["Consensus"], remove=["RX"]) if setting == "tags" else {}
    want, counts = ZR.zip_records(ZR.parse_records(b"".join(a)), ZR.parse_records(b"".join(u)), **kw)
    return ZR.read_bam(po)[:3], info, b"".join(ZR.encode(r) for r in want), counts


def _chunk(which, total):
    return {"all": 10 * total + 1, "half": total // 2 + 1, "third": total // 3 + 1, "template": 40, "byte": 1}[which]


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("which", ["all", "half", "third", "template", "byte"])
@pytest.mark.parametrize("name", SI.CASES)
def test_stream_equals_the_whole_file_path(work, tmp_path, name, which, setting):
    pa, pu, total = _files(work, name)
    (text, refs, data), winfo, want, counts = _whole(work, name, setting)
    assert data == want
    po, tmp = str(tmp_path / "o.bam"), tmp_path / "tmp"
    tmp.mkdir()
    info = zipper.zipper(pa, pu, po, host=True, level=1, stream=True, chunk_bytes=_chunk(which, total), tmp_dir=str(tmp),
                         info=str(tmp_path / "i.json"), **SETTINGS[setting])
    assert ZR.read_bam(po)[:3] == (text, refs, data)  # (read_bam: valid BGZF, CRC32 and ISIZE hold, one EOF block)
    for k in ("records_in", "unmapped_records_in", "records_out", "unmapped_dropped", "templates_without_aligned", "raw_bytes"):
        assert info[k] == winfo[k], k
    assert info["templates_without_aligned"] == counts["templates_without_aligned"]
    assert os.listdir(str(tmp)) == []
    n_templates = len({ZR.parse_records(r)[0]["name"] for r in SI.case(name)[0]})
    if which == "all":
        assert info["runs"] == 1 and info["spill_bytes"] == 0 and info["merge_rounds"] == 0
    elif which in ("template", "byte"):
        assert info["runs"] == max(n_templates, 1)
    elif n_templates:
        # (a chunk leaves once it has reached the budget: no more runs than this; one large template makes fewer)
        assert 2 <= info["runs"] <= (2 if which == "half" else 3) + (name != "big")
        assert info["runs"] >= (2 if which == "half" or name == "big" else 3)
    if info["runs"] > 1:
        assert info["spill_bytes"] == info["raw_bytes"] and info["merge_rounds"] >= 1
    import json
    assert json.load(open(str(tmp_path / "i.json"))) == info


def test_counts_of_the_lonely_templates(work):
    assert _whole(work, "contigs3", "none")[3]["templates_without_aligned"] == 7
    assert _whole(work, "empty", "none")[3]["templates_without_aligned"] == 5


def _order_inputs(kind):
    a, u = SI.case("sec_supp")
    if kind == "swapped":  # two templates of ALIGNED change places
        recs = ZR.parse_records(b"".join(a))
        t1 = [r for r in a if ZR.parse_records(r)[0]["name"] == b"p0010"]
        t2 = [r for r in a if ZR.parse_records(r)[0]["name"] == b"p0020"]
        i1, i2 = a.index(t1[0]), a.index(t2[0])
        assert recs and i1 < i2
        a = a[:i1] + t2 + a[i1 + len(t1):i2] + t1 + a[i2 + len(t2):]
        return a, u, "p0011"  # (p0020 is found early; the template behind it is not found behind p0020)
    if kind == "reversed":  # UNMAPPED in reverse record order
        return a, u[::-1], "p0001"  # (the first template is found, at the end)
    if kind == "missing":
        return a, [r for r in u if ZR.parse_records(r)[0]["name"] != b"p0030"], "p0030"
    if kind == "twice":
        k = next(i for i, r in enumerate(u) if ZR.parse_records(r)[0]["name"] == b"p0040")
        return a, u[:k + 1] + [u[k]] + u[k + 1:], "p0040"
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["swapped", "reversed", "missing", "twice"])
def test_order_and_partner_errors(tmp_path, kind):
    a, u, word = _order_inputs(kind)
    pa, pu, po, tmp = str(tmp_path / "a.bam"), str(tmp_path / "u.bam"), str(tmp_path / "o.bam"), tmp_path / "tmp"
    tmp.mkdir()
    SI.write_bam(pa, SI.TEXT_A, SI.REFS, b"".join(a))
    SI.write_bam(pu, SI.TEXT_U, [], b"".join(u))
    for chunk in (1, 1 << 30):
        with pytest.raises(ValueError) as e:
            zipper.zipper(pa, pu, po, host=True, level=1, stream=True, chunk_bytes=chunk, tmp_dir=str(tmp))
        assert os.listdir(str(tmp)) == []
        if kind == "twice":
            assert "twice" in str(e.value) and repr(word) in str(e.value)
        else:
            assert "--stream false" in str(e.value) and "template order" in str(e.value) and repr(word) in str(e.value)
    if kind in ("swapped", "reversed"):
        info = zipper.zipper(pa, pu, po, host=True, level=1)
        assert info["records_in"] == len(a)
    else:
        with pytest.raises(ValueError, match="twice" if kind == "twice" else "no partner"):
            zipper.zipper(pa, pu, po, host=True, level=1)


def test_an_end_missing_inside_its_template_has_no_partner(tmp_path):
    a, u = [ZI.rec("x", 99, 0, 1), ZI.rec("x", 147, 0, 9)], [ZI.rec("x", 77)]
    pa, pu = str(tmp_path / "a.bam"), str(tmp_path / "u.bam")
    SI.write_bam(pa, SI.TEXT_A, SI.REFS, b"".join(a))
    SI.write_bam(pu, SI.TEXT_U, [], b"".join(u))
    with pytest.raises(ValueError, match="aligned read 'x' \\(flag 147\\) has no partner"):
        zipper.zipper(pa, pu, str(tmp_path / "o.bam"), host=True, stream=True, tmp_dir=str(tmp_path))


def test_peak_record_bytes_is_bounded(tmp_path):
    """Counted: both inputs' pieces and carries, the chunk's records, its partners' aux and its
    formatted output (phase 1); the windows, the round's records gathered from them and the round's
    sorted output (phase 2)."""
    a, u = SI.case("bound")
    pa, pu, po = str(tmp_path / "a.bam"), str(tmp_path / "u.bam"), str(tmp_path / "o.bam")
    SI.write_bam(pa, SI.TEXT_A, SI.REFS, b"".join(a))
    SI.write_bam(pu, SI.TEXT_U, [], b"".join(u))
    chunk = 16384
    assert SI.budget(a, u) >= 40 * chunk  # (the bytes the budget counts: ALIGNED's records and their partners' aux)
    info = zipper.zipper(pa, pu, po, host=True, level=1, stream=True, chunk_bytes=chunk, tmp_dir=str(tmp_path))
    want, _ = ZR.zip_records(ZR.parse_records(b"".join(a)), ZR.parse_records(b"".join(u)))
    largest = max(len(ZR.encode(r)) for r in want)
    print("runs %d rounds %d peak %d bound %d" % (info["runs"], info["merge_rounds"], info["peak_record_bytes"],
                                                   4 * chunk + info["runs"] * largest))
    assert ZR.read_bam(po)[2] == b"".join(ZR.encode(r) for r in want)
    assert info["runs"] > 20
    assert info["peak_record_bytes"] <= 4 * chunk + info["runs"] * largest


def test_prefix_scan_at_every_cut():
    recs = [ZI.rec("r1", 99, 0, 1, aux=ZI.ALN), ZI.rec("r2", 147, 1, 2), ZI.rec("last", 83, 2, 3, l_seq=9, aux=ZI.CONS)]
    data = b"".join(recs)
    whole = len(recs[0]) + len(recs[1])
    for cut in range(whole, len(data) + 1):
        buf = zipper._aligned_copy(data[:cut])
        src, used = zipper.scan_prefix(buf, cut)
        n = 3 if cut == len(data) else 2
        assert src.shape[0] == n and used == (len(data) if n == 3 else whole), cut
        assert list(src["off"]) == [0, len(recs[0]), whole][:n] and list(src["len"]) == [len(r) for r in recs][:n]
        assert np.array_equal(src, zipper.scan(zipper._aligned_copy(data[:used]), used))
    src, used = zipper.scan_prefix(zipper._aligned_copy(b""), 0)
    assert src.shape[0] == 0 and used == 0
    # a record whose lengths leave it is an error, whole or cut
    bad = bytearray(recs[0])
    bad[20:24] = (10 ** 6).to_bytes(4, "little")  # l_seq
    for cut in (len(bad), 40):
        with pytest.raises(ValueError, match="malformed lengths"):
            zipper.scan_prefix(zipper._aligned_copy(bytes(bad[:cut])), cut)
    # the existing scan still refuses the cut record
    with pytest.raises(ValueError, match="truncated"):
        zipper.scan(zipper._aligned_copy(data[:-1]), len(data) - 1)


GATHER_N = [0, 1, 2, 14, 3000]


@pytest.mark.parametrize("n", GATHER_N)
def test_gather_host_equals_slice_and_join(n):
    src, off, ln = SI.gather_case(n)
    for name, order in SI.gather_orders(n).items():
        want = b"".join(src[int(off[k]):int(off[k]) + int(ln[k])].tobytes() for k in order)
        got_off, dst = zipper_stream.gather_host(order, off, ln, src, cap=len(want), fill=GUARD)
        assert np.array_equal(got_off, np.concatenate([[0], np.cumsum(ln[order].astype(np.int64))])), name
        assert dst[:len(want)].tobytes() == want, name
        assert (dst[len(want):] == GUARD).all(), name
    if n >= 14:
        assert {int(o) % 4 for o in off} == {0, 1, 2, 3} and {int(o) % 4 for o in got_off[:-1]} == {0, 1, 2, 3}


def test_gather_host_refusals():
    lib = _lib.load()
    src, off, ln = SI.gather_case(14)
    order = np.arange(14, dtype=np.uint32)
    total = int(ln.sum())
    dst = np.full(total + 64, GUARD, np.uint8)
    out = np.zeros(15, np.int64)
    call = lambda o=order, n=14, so=off, sl=ln, s=src, sb=None, of=out, d=dst, cap=total: lib.bsdc_zip_gather_host(  # noqa: E731
        None if o is None else o.ctypes.data, n, None if so is None else so.ctypes.data, None if sl is None else sl.ctypes.data,
        None if s is None else s.ctypes.data, int(src.shape[0]) if sb is None else sb, None if of is None else of.ctypes.data,
        None if d is None else d.ctypes.data, cap)
    err = lambda: lib.bsdc_zip_last_error().decode()  # noqa: E731
    assert call() == 0 and not (dst[:total] == GUARD).all()
    dst[:] = GUARD
    for kw, word in ((dict(o=None), "order is null"), (dict(so=None), "null"), (dict(sl=None), "null"), (dict(s=None), "src is null"),
                     (dict(of=None), "off is null"), (dict(d=None), "dst is null"), (dict(n=-1), "negative"),
                     (dict(sb=int(off[-1]) + int(ln[-1]) - 1), "leave src"), (dict(cap=total - 1), "below the records' bytes")):
        assert call(**kw) == -22 and word in err(), (kw, err())
        assert (dst == GUARD).all()
    bad = order.copy()
    bad[3] = 14
    assert call(o=bad) == -22 and "order[3] is not below n" in err() and (dst == GUARD).all()
    neg = off.copy()
    neg[5] = -4
    assert call(so=neg) == -22 and "record 5" in err() and (dst == GUARD).all()


def test_cli_stream(tmp_path, work, monkeypatch):
    pa, pu, _ = _files(work, "contigs3")
    (text, refs, data), _, _, _ = _whole(work, "contigs3", "none")
    real = zipper.zipper
    monkeypatch.setattr(zipper, "zipper", lambda *a, **k: real(*a, host=True, **k))
    tmp = tmp_path / "t"
    tmp.mkdir()
    assert cli.main(["zipper", pa, pu, str(tmp_path / "o.bam"), "--stream", "true", "--chunk-mb", "1", "--tmp-dir", str(tmp),
                     "--level", "1", "--info", str(tmp_path / "i.json")]) == 0
    assert ZR.read_bam(str(tmp_path / "o.bam"))[:3] == (text, refs, data)
    import json
    assert json.load(open(str(tmp_path / "i.json")))["runs"] == 1
    with pytest.raises(SystemExit):
        cli.parse(["zipper", pa, pu, "o.bam", "--stream", "maybe"])
    a = cli.parse(["zipper", pa, pu, "o.bam"])
    assert a.stream == "false" and a.chunk_mb == 1024 and a.tmp_dir is None

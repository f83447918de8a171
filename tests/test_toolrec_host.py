"""The tool-stage record writer's host twin (bsdc_toolrec_host, csrc/bsdc_toolrec.hip)
against the Python restatement tests/toolrec_ref.py, byte for byte, on the fabricated sets of
tests/toolrec_inputs.py; its bytes read back by the project's BAM reader; the pin to the reference
tools on tests/golden/tool12_families.json.gz; its refusals; the header; the CLI's parsing; and the
twin under the sanitizers as a stand-alone program.  No GPU: test_gpu_toolrec.py runs the same sets
through the kernel."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import toolrec_inputs as TI
import toolrec_ref as TR
from bsseqconsensusreads_amd import _lib, bam, bgzf, cli, toolrec
from bsseqconsensusreads_amd import records as R
from helpers import golden_inputs, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5C


def twin(c: TI.Case, extra=64):
    t = c.tables()
    n_dump = c.dump_seq.shape[0] // 4 * 4
    cap = t.bound(n_dump) + extra
    off, buf = toolrec.host(t, c.rec_off, c.dump_pos, c.dump_len, c.dump_tags, c.dump_seq, c.dump_qual, cap=cap, fill=GUARD)
    return off, buf


def twin_call(c: TI.Case, n_dump=None, cap=None, alloc=None):
    """bsdc_toolrec_host with n_dump and cap as given (default: the dump's own size, the bound) on a
    buffer of `alloc` GUARD bytes -> (rc, off, buf)"""
    t = c.tables()
    n = t.n
    rec = np.zeros((max(n, 1), 4), np.uint32)
    rec[:n, 0] = c.rec_off
    n_dump = c.dump_seq.shape[0] // 4 * 4 if n_dump is None else n_dump
    cap = t.bound(n_dump) if cap is None else cap
    buf, off = np.full(max(cap, 1) if alloc is None else alloc, GUARD, np.uint8), np.zeros(n + 1, np.int64)
    o = toolrec._consensus_c(c.dump_pos, c.dump_len, c.dump_tags, c.dump_seq, c.dump_qual)
    rc = _lib.load().bsdc_toolrec_host(C.byref(o), rec.ctypes.data, n, n_dump, t.tab.ctypes.data, t.names.ctypes.data,
                                       t.names.shape[0], t.cigar.ctypes.data, t.cigar.shape[0], t.aux.ctypes.data,
                                       t.aux.shape[0], off.ctypes.data, buf.ctypes.data, cap)
    return rc, off, buf


def test_exports_and_layout():
    lib = _lib.load()
    assert lib.bsdc_abi_version() == 19
    for k in ("bsdc_toolrec_bytes_bound", "bsdc_toolrec_tmp_bytes", "bsdc_toolrec_format", "bsdc_toolrec_host",
              "bsdc_toolrec_last_error"):
        assert k in _lib.EXPORTS and hasattr(lib, k)
    assert np.dtype(_lib.TOOLREC_REC).itemsize == 56
    assert lib.bsdc_toolrec_bytes_bound(0, 0, 0, 0, 0) == 0 and lib.bsdc_toolrec_bytes_bound(-1, 0, 0, 0, 0) < 0
    assert lib.bsdc_toolrec_bytes_bound(2, 10, 3, 7, 8) == 2 * 54 + 10 + 12 + 7 + 12


@pytest.mark.parametrize("name", TI.NAMES)
def test_twin_equals_the_restatement(name):
    c = TI.build_named(name)
    recs = c.recs
    off, buf = twin(c)
    want_off, want = TR.stream(recs)
    assert np.array_equal(off, want_off), name
    total = int(off[-1])
    got = buf[:total].tobytes()
    if got != want:
        k = next(i for i in range(len(recs)) if got[off[i]:off[i + 1]] != want[off[i]:off[i + 1]])
        a, b = got[off[k]:off[k + 1]], want[off[k]:off[k + 1]]
        j = next(i for i in range(len(a)) if a[i] != b[i])
        raise AssertionError("%s: record %d differs at byte %d: %s vs %s" % (name, k, j, a[j:j + 8].hex(), b[j:j + 8].hex()))
    assert (buf[total:] == GUARD).all(), name + ": bytes past the end"


def test_sets_hold_their_edges():
    """what the sets are for, read off the restatement"""
    sizes = np.diff(TR.stream(TI.make("place"))[0])
    assert sizes.max() > 65280 and set((np.cumsum(sizes) % 4).tolist()) == {0, 1, 2, 3}
    assert {len(r["name"]) for r in TI.make("place")} >= set(range(1, 9)) | {254}
    assert max(len(r["seq"]) for r in TI.make("lens")) == TI.MAX_LEN == 65529
    assert TR.new_cigar([TI.op(1, 0)], 7) == [TI.op(1, 0)]
    assert TR.new_cigar([TI.op(3, 4), TI.op(20, 0), TI.op(9, 0), TI.op(2, 4)], 15) == [16, TI.op(20, 0), TI.op(8, 0), 16]
    assert TR.reg2bin(-1, 0) == 4680 and TR.reg2bin(0, 1) == 4681
    assert TR.reg2bin((1 << 14) - 5, (1 << 14) + 6) == 585 and TR.reg2bin((1 << 17) - 100, (1 << 17) + 111) == 73
    assert TR.new_aux(b"XBBC\x06\0\0\0RDCLAC" + b"RDC\x01", 7) == b"XBBC\x06\0\0\0RDCLAC" + b"RDC\x01LAC\x01"
    assert TR.new_aux(b"RDC\x01MIZ1\0", 0) == b"RDC\x01MIZ1\0"
    _later_sets_hold_their_edges()


def _bin(r, ops):
    n = TI.ref_len(ops)
    return TR.reg2bin(r["pos"], r["pos"] + (n if n > 0 else 1))


def _later_sets_hold_their_edges():
    """test_sets_hold_their_edges, the sets that came later"""
    # longcigar: the ops a lane reads in a second round decide the bin
    recs = TI.make("longcigar")
    second = 0
    for r in recs:
        ops = TR.new_cigar(r["cigar"], r["tags"])
        assert ops == TI.new_ops(r)
        if len(ops) > 64:
            assert _bin(r, ops) != _bin(r, ops[:64]), r["name"]
            second += 1
    n_out = {len(TR.new_cigar(r["cigar"], r["tags"])) for r in recs}
    assert second >= 40 and {63, 64, 65, 66, 128, 129, 130, 131, 1000, 1002, 65533, 65535} <= n_out
    assert max(n_out) == 65535 and max(len(TR.strip_clips(r["cigar"])) for r in recs) == TI.MAX_OPS == 65533
    for n in TI.LONG_OPS:  # RD drops a last op of length 1 and shortens a longer one, at every count
        ends = {(r["tags"], r["cigar"][-1 - (r["cigar"][-1] & 15 == TI.S)] >> 4) for r in recs
                if len(TR.strip_clips(r["cigar"])) == n}
        assert {(7, 1), (7, 5), (15, 1), (15, 5), (0, 1), (6, 5)} <= ends, n
    lanes = set()
    for r in recs:
        lanes |= {j % 64 for j, o in enumerate(TR.new_cigar(r["cigar"], r["tags"])) if (o & 15) in TR.REF_OPS and j >= 64}
    assert lanes == set(range(64))
    # hugeref: the sum's high half decides the bin
    recs = TI.make("hugeref")
    low_alone = 0
    for r in recs:
        ops = TR.new_cigar(r["cigar"], r["tags"])
        n = TI.ref_len(ops)
        assert n >= 1 << 32 and r["pos"] in (0, 1000) and _bin(r, ops) == 0
        low = n & 0xFFFFFFFF
        low_alone += TR.reg2bin(r["pos"], r["pos"] + (low if low > 0 else 1)) != 0
        if low < 1 << 20:  # one lane's ops pass 2^32 alone, and it is not the lane that writes the bin
            per = [sum(o >> 4 for j, o in enumerate(ops) if j % 64 == k and (o & 15) in TR.REF_OPS) for k in range(64)]
            assert max(per) >= 1 << 32 and per[1] < 1 << 32
    assert low_alone >= 5
    # phases: every combination at every residue of the record's start
    recs = TI.make("phases")
    off = TR.stream(recs)[0]
    assert np.array_equal(np.diff(off), [TI.size_of(r) for r in recs])
    seen = {(int(off[k]) & 3, len(r["name"]), len(r["seq"]), len(r["aux"]), r["tags"]) for k, r in enumerate(recs) if k & 1}
    P = TI.PHASES
    assert seen == {(h, a, b, c, d) for h in range(4) for a in P["nl"] for b in P["L"] for c in P["al"] for d in P["tags"]}
    assert {b & 7 for b in P["L"]} == {7, 0, 1} and len({bytes(r["qual"]) for r in recs}) > len(recs) - 8
    # tight: the last record's bases end the dump, or a multiple of 4 does, with nothing behind
    for L in TI.TIGHT:
        c = TI.build_named("tight_%d" % L)
        assert int(c.dump_len[-1]) == L and c.dump_seq.shape[0] == c.dump_qual.shape[0] == int(c.rec_off[-1]) + (L + 3) // 4 * 4
    # the shared entries: the records outgrow the bound
    c = TI.shared_case()
    total = sum(len(TR.record_bytes(TI.record_of(c, r))) for r in range(c.n))
    cap = c.tables().bound(c.dump_seq.shape[0])
    assert c.n == 200 and total > cap + 4000 and total == int(TI.layout_sizes(c).sum())
    e = c.tables().tab
    assert (e["name_off"] == 0).all() and (e["cig_off"] == 0).all() and (e["aux_off"] == 0).all()
    assert (e["name_len"] == 8).all() and (e["n_cig"] == 3).all() and (e["aux_len"] == 40).all()
    assert len(set(c.rec_off.tolist())) == c.n
    # the carry: one tile of workgroup sums, one more, and two more
    assert [TI.scan_groups(n) for n in TI.CARRY_COUNTS] == [256, 257, 258]
    assert TI.CARRY_COUNTS == (262144, 262145, 262144 + 1025)
    assert [TI.scan_groups(int(n.split("_")[1])) for n in ("counts_1023", "counts_1024", "counts_1025")] == [1, 1, 2]


def test_twin_stops_at_cap_with_shared_entries():
    """cap = the bound exactly, the records' total beyond it: the offsets are whole, the bytes
    below cap are the restatement's, and no byte at or past cap is written"""
    c = TI.shared_case()
    want_off, want = TR.stream([TI.record_of(c, r) for r in range(c.n)])
    cap = c.tables().bound(c.dump_seq.shape[0])
    total = int(want_off[-1])
    k = int(np.searchsorted(want_off, cap, "right")) - 1
    assert cap < total and cap % 4 == 2 and want_off[k] + 4 <= cap <= want_off[k + 1] - 4
    rc, off, buf = twin_call(c, cap=cap, alloc=total + 64)
    assert rc == 0, _lib.load().bsdc_toolrec_last_error().decode()
    assert np.array_equal(off, want_off)
    assert buf[:cap].tobytes() == want[:cap]
    assert (buf[cap:] == GUARD).all()


@pytest.fixture(scope="module")
def carry_twin():
    """the largest carry case through the twin once"""
    c = TI.carry_case(TI.CARRY_COUNTS[-1])
    return c, twin(c)


def test_carry_case_twin_equals_the_restatement(carry_twin):
    """the twin is what the kernel is compared with on the carry cases: its offsets against the
    layout rule in numpy, its bytes against the restatement on 2,000 records picked at random"""
    c, (off, buf) = carry_twin
    sizes = TI.layout_sizes(c)
    assert np.array_equal(off[1:], np.cumsum(sizes)) and off[0] == 0
    assert (buf[int(off[-1]):] == GUARD).all()
    assert set(c.dump_tags.tolist()) == {0, 6, 7, 15, 8, 4, 12} and set(c.tables().tab["n_cig"].tolist()) == {0, 1, 2}
    for r in np.random.default_rng(1).choice(c.n, 2000, replace=False):
        want = TR.record_bytes(TI.record_of(c, int(r)))
        assert buf[int(off[r]):int(off[r + 1])].tobytes() == want, int(r)


def _write(path, recs_bytes, hdr):
    w = bgzf.BamWriter(str(path), hdr, 1)
    try:
        w.add_raw(recs_bytes, 2)
    finally:
        w.close(2)


HDR = bam.BamHeader("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c0\tLN:1073741824\n@SQ\tSN:c1\tLN:1073741824\n@SQ\tSN:c2\tLN:1073741824\n",
                    ["c0", "c1", "c2"], np.asarray([1 << 30] * 3, np.int64))


@pytest.mark.parametrize("name", ["cigar", "aux", "bin", "counts_65"])
def test_reader_gives_back_the_fields(name, tmp_path):
    recs = TI.make(name)
    off, buf = twin(TI.build(recs))
    p = tmp_path / "t.bam"
    _write(p, buf[:int(off[-1])].tobytes(), toolrec.header(HDR))
    h, out = bam.read_bam(str(p), 2)
    assert out.n == len(recs)
    assert toolrec.hd_line(h.text) == "@HD\tVN:1.6\tSO:unsorted\tGO:query\tSS:unsorted:template-coordinate"
    for k, r in enumerate(recs):
        t = r["tags"]
        assert out.names[int(out.name_id[k])] == r["name"]
        assert (int(out.flag[k]), int(out.tid[k]), int(out.mapq[k]), int(out.next_tid[k]), int(out.next_pos[k]),
                int(out.tlen[k]), int(out.pos[k])) == (r["flag"], r["ref_id"], r["mapq"], r["next_ref_id"], r["next_pos"],
                                                         r["tlen"], r["pos"]), k
        assert np.array_equal(out.record_seq(k), r["seq"]) and np.array_equal(out.record_qual(k), r["qual"]), k
        assert [int(x) for x in out.record_cigar(k)] == TR.new_cigar(r["cigar"], t), k
        assert out.aux[k] == TR.new_aux(r["aux"], t), k
        if t & 2:
            assert (int(out.rd_tag[k]), int(out.la_tag[k])) == (t & 1, 1), k


def test_aux_of_a_decoded_bam_is_walked(tmp_path):
    """the `aux` set as a real input gives it: written as a BAM and read back, so that the records'
    aux lie in the decoder's packed table (the path every file takes) -- RD / LA of any type and
    value are cut from the converted records, payloads that read RDC / LAC stay"""
    recs = TI.make("aux")
    c = TI.build(recs)
    p = tmp_path / "in.bam"
    bam.write_bam(str(p), HDR, bam.records_to_bam(c.raw), level=1, threads=2)
    _, back = bam.read_bam(str(p), 2)
    assert hasattr(back.aux, "off") and back.n == len(recs)
    assert (back.rd_tag < 0).sum() > 0 and any(b"LAZ" in r["aux"] for r in recs)
    t = toolrec.tables(back, np.arange(back.n), c.conv)
    off, buf = toolrec.host(t, c.rec_off, c.dump_pos, c.dump_len, c.dump_tags, c.dump_seq, c.dump_qual)
    want_off, want = TR.stream(recs)
    assert np.array_equal(off, want_off) and buf[:int(off[-1])].tobytes() == want


def test_header_rules():
    assert toolrec.hd_line(toolrec.header(bam.BamHeader("@SQ\tSN:a\tLN:5\n", ["a"], np.asarray([5]))).text) == \
        "@HD\tVN:1.6\tSO:unsorted\tGO:query\tSS:unsorted:template-coordinate"
    h = toolrec.header(bam.BamHeader("@HD\tVN:1.5\tSO:coordinate\tGO:none\n@SQ\tSN:a\tLN:5\n@PG\tID:x\n", ["a"], np.asarray([5])))
    assert h.text == "@HD\tVN:1.5\tSO:unsorted\tGO:query\tSS:unsorted:template-coordinate\n@SQ\tSN:a\tLN:5\n@PG\tID:x\n"
    assert h.ref_names == ["a"]


def _dump_from_tool2(raw, t2):
    """A stage dump as the fused step leaves it, made of the restatement's tool-2 records: the tag
    bits from the records' own lengths and positions, never from their cigars."""
    n = len(t2.src)
    src = np.asarray(t2.src, np.int64)
    L = np.asarray([len(t2.record(k)["seq"]) for k in range(n)], np.int64)
    size = (L + 5) // 4 * 4
    rec_off = (np.cumsum(size) - size).astype(np.uint32)
    ds, dq = np.zeros(int(size.sum()) + 16, np.uint8), np.zeros(int(size.sum()) + 16, np.uint8)
    tags = np.zeros(n, np.uint8)
    for k in range(n):
        r = t2.record(k)
        o = int(rec_off[k])
        ds[o:o + L[k]], dq[o:o + L[k]] = r["seq"], r["qual"]
        ops = TR.strip_clips(int(x) for x in raw.record_cigar(int(src[k])))
        l_in = sum(x >> 4 for x in ops if (x & 15) in (0, 1, 7, 8))
        if r["la"] == 1:  # converted: a base in front, RD takes the last one, tool 2 may append one
            tags[k] = 2 | 4 | r["rd"] | (8 if L[k] - l_in - 1 + r["rd"] else 0)
        else:
            pre = int(raw.pos[int(src[k])]) - r["pos"]
            tags[k] = (4 if pre else 0) | (8 if L[k] - l_in - pre else 0)
    return rec_off, np.asarray(t2.pos, np.int32), L.astype(np.uint16), tags, ds, dq


def test_golden_tool2_records_are_pinned(tmp_path):
    """the reference tools' own output on the golden families: seq, qual, pos, cigar and RD / LA of
    every record, matched by name and flag"""
    from oracle import oracle
    g = load_golden("tool12_families.json.gz")
    raw, ref = golden_inputs(g)
    t2 = oracle.run(raw, ref).tool2
    rec_off, pos, L, tags, ds, dq = _dump_from_tool2(raw, t2)
    assert (tags & 2).any() and (tags & 8).any() and ((tags & 6) == 4).any()
    t = toolrec.tables(raw, np.asarray(t2.src, np.int64), (tags & 2) != 0)
    off, buf = toolrec.host(t, rec_off, pos, L, tags, ds, dq)
    p = tmp_path / "g.bam"
    names = [c["name"] for c in g["header"]["references"]]
    hdr = bam.BamHeader("".join("@SQ\tSN:%s\tLN:%d\n" % (c["name"], c["length"]) for c in g["header"]["references"]),
                        names, np.asarray([c["length"] for c in g["header"]["references"]], np.int64))
    _write(p, buf[:int(off[-1])].tobytes(), toolrec.header(hdr))
    _, out = bam.read_bam(str(p), 2)
    want = {(x["name"], x["flag"]): x for x in g["tool2"]}
    assert out.n == len(g["tool2"]) == len(want)
    for k in range(out.n):
        x = want[(out.names[int(out.name_id[k])].decode(), int(out.flag[k]))]
        assert int(out.pos[k]) == x["pos"], x["name"]
        assert [int(v) for v in out.record_cigar(k)] == [(l << 4) | op for op, l in x["cigar"]], x["name"]
        assert R.decode_seq(out.record_seq(k)) == x["seq"], x["name"]
        assert (out.record_qual(k) + 33).astype(np.uint8).tobytes().decode() == x["qual"], x["name"]
        tg = {a[0]: a[2] for a in x["tags"]}
        got = {a[0]: a[2] for a in R.parse_aux(out.aux[k])}
        assert got == tg, x["name"]
        assert tg.get("RD", -1) == int(out.rd_tag[k]) and tg.get("LA", -1) == int(out.la_tag[k])


def _host_call(**bad):
    c = TI.build(TI.make("counts_1"))
    t = toolrec.tables(c.raw, np.arange(1), c.conv)
    lib = _lib.load()
    o = toolrec._consensus_c(c.dump_pos, c.dump_len, c.dump_tags, c.dump_seq, c.dump_qual)
    for k in ("dump_pos", "dump_len", "dump_tags", "dump_seq", "dump_qual"):
        if bad.get(k):
            setattr(o, k, None)
    rec = np.zeros((1, 4), np.uint32)
    n_dump = c.dump_seq.shape[0] // 4 * 4
    cap = t.bound(n_dump)
    buf, off = np.zeros(cap + 8, np.uint8), np.zeros(2, np.int64)
    tab = t.tab.copy()
    for k, v in bad.get("entry", {}).items():
        tab[k] = v
    a = dict(out=C.byref(o), rec=rec.ctypes.data, n=1, n_dump=n_dump, tab=tab.ctypes.data, names=t.names.ctypes.data,
             nb=t.names.shape[0], cig=t.cigar.ctypes.data, no=t.cigar.shape[0], aux=t.aux.ctypes.data, ab=t.aux.shape[0],
             off=off.ctypes.data, dst=buf.ctypes.data, cap=cap)
    a.update({k: v for k, v in bad.items() if k in a})
    rc = lib.bsdc_toolrec_host(a["out"], a["rec"], a["n"], a["n_dump"], a["tab"], a["names"], a["nb"], a["cig"], a["no"],
                               a["aux"], a["ab"], a["off"], a["dst"], a["cap"])
    return rc, lib.bsdc_toolrec_last_error().decode()


def test_twin_refuses_bad_arguments():
    assert _host_call()[0] == 0
    for k in ("dump_pos", "dump_len", "dump_tags", "dump_seq", "dump_qual"):
        rc, msg = _host_call(**{k: True})
        assert rc == -22 and k + " is null" in msg, msg
    for k, word in (("out", "out"), ("rec", "rec"), ("tab", "tab"), ("names", "names"), ("cig", "cigar"), ("aux", "aux"),
                    ("off", "off"), ("dst", "dst")):
        rc, msg = _host_call(**{k: None})
        assert rc == -22 and word + " is null" in msg, msg
    for k, word in (("n", "n_rec"), ("n_dump", "n_dump"), ("nb", "name_bytes"), ("no", "n_ops"), ("ab", "aux_bytes")):
        rc, msg = _host_call(**{k: -1})
        assert rc == -22 and word in msg, msg
    rc, msg = _host_call(n_dump=8)  # the record's dump slot leaves the dump
    assert rc == -22 and "record 0" in msg and "dump slot" in msg, msg
    rc, msg = _host_call(cap=10)
    assert rc == -22 and "below bsdc_toolrec_bytes_bound" in msg
    for tab, word in (({"name_len": 0}, "name_len"), ({"name_off": 1 << 20}, "name"), ({"n_cig": 65534}, "n_cig"),
                      ({"cig_off": 5}, "cigar"), ({"aux_len": -1}, "aux_len"), ({"aux_off": 1 << 30}, "aux")):
        rc, msg = _host_call(entry=tab)
        assert rc == -22 and "record 0" in msg and word in msg, msg


def test_cli_parsing(capsys):
    a = cli.parse(["step5", "-r", "g.fa", "in.bam", "out.bam", "--groupsort-bam", "g.bam"])
    assert a.groupsort_bam == "g.bam"
    assert cli.parse(["step5", "-r", "g.fa", "in.bam", "out.bam"]).groupsort_bam is None
    assert cli.parse(["step5", "-r", "g.fa", "in.bam", "-", "--fastq1", "a", "--fastq2", "b", "--groupsort-bam", "g.bam",
                      "--gpu-fastq", "true", "--gpu-image", "true", "--gpu-inflate", "true", "--metrics", "m.json",
                      "--filter-min-base-quality", "20"]).groupsort_bam == "g.bam"
    for argv, word in ((["molecular", "in.bam", "out.bam", "--groupsort-bam", "g.bam"], "--groupsort-bam"),
                       (["step5", "-r", "g.fa", "in.bam", "out.bam", "--groupsort-bam", "g.bam", "--gpus", "2"], "--gpus 2")):
        with pytest.raises(SystemExit):
            cli.parse(argv)
        err = capsys.readouterr().err
        assert "--groupsort-bam" in err and word in err
        assert "unrecognized" not in err
    with pytest.raises(SystemExit):
        cli.parse(["molecular", "in.bam", "out.bam", "--groupsort-bam", "g.bam"])
    assert "runs no tools" in capsys.readouterr().err
    from bsseqconsensusreads_amd import stream
    assert stream.StreamJob("a", "b", "c").groupsort_bam is None
    with pytest.raises(ValueError, match="groupsort_bam"):
        stream.run(stream.StreamJob("a.bam", "r.fa", "o.bam", groupsort_bam="g.bam"), runner=object())
    with pytest.raises(ValueError, match="groupsort_bam"):
        stream.run(stream.StreamJob("a.bam", "r.fa", "o.bam", groupsort_bam="g.bam", rng=(0, 1)), engine=object())
    with pytest.raises(ValueError, match="groupsort_bam"):
        stream.run(stream.StreamJob("a.bam", None, "o.bam", groupsort_bam="g.bam", molecular=0), engine=object())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_twin_under_sanitizers(tmp_path):
    """tests/sanitize/toolrec_twin_main.cpp: the twin on heap buffers of their exact sizes under
    -fsanitize=address,undefined (host code, its own main)."""
    exe = str(tmp_path / "toolrec_twin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-x", "c++", os.path.join(ROOT, "tests", "sanitize", "toolrec_twin_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "toolrec twin ok" in r.stdout

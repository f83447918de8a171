"""The tool-stage record writer on the GPU (bsdc_toolrec_format, csrc/bsdc_toolrec.hip; DESIGN.md 3.10,
8.11) and cli step5 --groupsort-bam: the kernel against its host twin byte for byte on the fabricated
sets; the records of every kernel route against oracle/'s tool-2 records; the files of the
streaming and the whole-file path; and the closure -- callduplex alone on the written file gives
the fused step's consensus."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest
import torch

import toolrec_inputs as TI
from bsseqconsensusreads_amd import _lib, bam, cli, pipeline, stream, synth, toolrec
from bsseqconsensusreads_amd import records as R
from oracle import oracle
from test_gpu_parity import force_large, force_parts
from test_toolrec_host import GUARD, twin

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.size else np.zeros(8, np.uint8)).to(dev)


def device_format(engine, c: TI.Case, extra=64, cap=None, null=None, *, dst_shift=0, n_dump=None, alloc=None, fetch=True):
    """bsdc_toolrec_format on a fabricated case -> (rc, off, buf); the buffer prefilled with GUARD.
    dst_shift: the destination starts that many bytes into the buffer (which is 8 bytes longer);
    n_dump: what the call is told in place of the dump's size (the device buffers keep theirs);
    alloc: the buffer's size where cap is not to decide it; fetch=False: off and buf stay on the device."""
    lib, dev = engine.lib, engine.device
    t = c.tables()
    n = t.n
    n_have = c.dump_seq.shape[0] // 4 * 4
    n_dump = n_have if n_dump is None else n_dump
    assert 0 <= n_dump <= n_have and 0 <= dst_shift < 8
    cap = t.bound(n_dump) + extra if cap is None else cap
    rec = np.zeros((max(n, 1), 4), np.uint32)
    rec[:n, 0] = c.rec_off
    d = {k: _dev(v, dev) for k, v in dict(pos=c.dump_pos, len=c.dump_len, tags=c.dump_tags, seq=c.dump_seq[:n_have],
                                          qual=c.dump_qual[:n_have], rec=rec, tab=t.tab, names=t.names, cigar=t.cigar,
                                          aux=t.aux).items()}
    o = _lib.ConsensusC()
    o.dump_pos, o.dump_len, o.dump_tags = d["pos"].data_ptr(), d["len"].data_ptr(), d["tags"].data_ptr()
    o.dump_seq, o.dump_qual = d["seq"].data_ptr(), d["qual"].data_ptr()
    if null:
        setattr(o, null, None)
    size = (max(cap, 16) + (8 if dst_shift else 0)) if alloc is None else alloc
    assert size >= dst_shift + cap  # (whatever the kernel does up to cap stays inside the allocation)
    buf = torch.full((size,), GUARD, dtype=torch.uint8, device=dev)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    tmp = torch.empty(int(lib.bsdc_toolrec_tmp_bytes(n)), dtype=torch.uint8, device=dev)
    tab_h = np.ascontiguousarray(t.tab) if n else np.zeros(1, _lib.TOOLREC_REC)
    s = torch.cuda.current_stream(dev)
    rc = lib.bsdc_toolrec_format(C.byref(o), d["rec"].data_ptr(), n, n_dump, d["tab"].data_ptr(), tab_h.ctypes.data,
                                 d["names"].data_ptr(), t.names.shape[0], d["cigar"].data_ptr(), t.cigar.shape[0],
                                 d["aux"].data_ptr(), t.aux.shape[0], off.data_ptr(), buf.data_ptr() + dst_shift, cap,
                                 tmp.data_ptr(), C.c_void_p(s.cuda_stream))
    s.synchronize()
    if not fetch:
        return rc, off, buf
    return rc, off.cpu().numpy(), buf.cpu().numpy()


@pytest.mark.parametrize("name", TI.NAMES)
def test_kernel_equals_the_twin(engine, name):
    c = TI.build_named(name)
    want_off, want = twin(c)
    rc, off, buf = device_format(engine, c)
    assert rc == 0, engine.lib.bsdc_toolrec_last_error().decode()
    assert np.array_equal(off, want_off), name
    bad = np.nonzero(buf[:want.shape[0]] != want)[0]
    assert bad.size == 0, "%s: byte %d (record %d): %d vs %d" % (
        name, bad[0], int(np.searchsorted(off, bad[0], "right")) - 1, buf[bad[0]], want[bad[0]])
    assert (buf[int(off[-1]):] == GUARD).all(), name + ": bytes past the end"


def test_launcher_refusals(engine):
    c = TI.build(TI.make("counts_1"))
    err = lambda: engine.lib.bsdc_toolrec_last_error().decode()  # noqa: E731
    for k in ("dump_pos", "dump_len", "dump_tags", "dump_seq", "dump_qual"):
        rc, _, buf = device_format(engine, c, null=k)
        assert rc == -22 and k + " is null" in err() and (buf == GUARD).all()
    rc, _, buf = device_format(engine, c, cap=16)
    assert rc == -22 and "below bsdc_toolrec_bytes_bound" in err() and (buf == GUARD).all()
    assert engine.lib.bsdc_toolrec_tmp_bytes(-1) < 0 and engine.lib.bsdc_toolrec_bytes_bound(0, 0, -1, 0, 0) < 0
    lib = engine.lib
    o = _lib.ConsensusC()
    assert lib.bsdc_toolrec_format(C.byref(o), None, -1, 0, None, None, None, 0, None, 0, None, 0, None, None, 0, None,
                                   None) == -22


def parse(data: bytes):
    """BAM record bytes -> [dict(name, flag, pos, cigar, seq, qual, aux)]"""
    out, i = [], 0
    while i < len(data):
        bs, tid, pos, lrn, mapq, b, nc, flag, L = struct.unpack_from("<iiiBBHHHi", data, i)
        o = i + 36
        name = data[o:o + lrn - 1]
        o += lrn
        cig = list(struct.unpack_from("<%dI" % nc, data, o))
        o += 4 * nc
        p = np.frombuffer(data, np.uint8, (L + 1) // 2, o)
        seq = np.stack([p >> 4, p & 15], 1).reshape(-1)[:L]
        o += (L + 1) // 2
        qual = np.frombuffer(data, np.uint8, L, o)
        o += L
        out.append(dict(name=name, flag=flag, pos=pos, cigar=cig, seq=seq, qual=qual, aux=data[o:i + 4 + bs]))
        i += 4 + bs
    assert i == len(data)
    return out


def piece_bytes(pieces) -> bytes:
    out = []
    for x in pieces:
        a = x.rec if x.event is None else x.rec[:int(x.foff[-1])].cpu().numpy()
        out.append(a[:int(x.foff[-1])].tobytes())
    return b"".join(out)


def assert_records_equal_oracle(recs, src, ref, raw, what):
    """recs[i] is input record src[i] after the tools; oracle/'s tool-2 records by input record"""
    t2 = ref.tool2
    at = {int(s): k for k, s in enumerate(t2.src)}
    assert sorted(at) == sorted(int(s) for s in src), what + ": the records written"
    for r, s in zip(recs, src):
        w = t2.record(at[int(s)])
        ctx = "%s: input record %d" % (what, int(s))
        assert r["pos"] == w["pos"] and r["flag"] == int(raw.flag[int(s)]), ctx
        assert np.array_equal(r["seq"], w["seq"]) and np.array_equal(r["qual"], w["qual"]), ctx
        assert r["cigar"] == [int(x) for x in w["cigar"]], ctx
        tg = {t: v for t, _, v in R.parse_aux(r["aux"])}
        if w["la"] >= 0:
            assert (tg.get("RD"), tg.get("LA")) == (w["rd"], w["la"]), ctx


@pytest.mark.parametrize("route", ["c0", "c2", "large", "parts"])
def test_routes_equal_oracle(engine, monkeypatch, route):
    cfg, n = {"c0": ("C0", 600), "c2": ("C2", 2000), "large": ("C2", 300), "parts": ("C3", 60)}[route]
    s = synth.generate(cfg, n, seed=41, device="cpu", genome_len=300_000)
    raw = synth.messify(s.raw, frac=0.1, seed=2) if route in ("c2", "large") else s.raw
    seen = []
    if route == "large":
        force_large(monkeypatch, "lds")
    if route == "parts":
        force_parts(monkeypatch, 20000, seen)
    engine.load_reference(s.ref)
    cons, _ = pipeline.run_step5(engine, raw, toolrec="device")
    if route == "parts":
        assert sum(fb.split_fams.shape[0] for fb in seen) > 0
    ref = oracle.run(raw, s.ref)
    recs = parse(piece_bytes(cons.toolrec))
    assert len(recs) == cons.fam_src.shape[0] == sum(x.n_rec for x in cons.toolrec)
    assert_records_equal_oracle(recs, cons.fam_src, ref, raw, route)
    if route == "c0":  # tool 2 acts: prepended and appended bases
        lens = np.asarray([len(r["seq"]) for r in recs]) - raw.l_seq[cons.fam_src]
        assert (lens == 2).any() or (lens == 1).any()
    # the host twin's bytes of the same run
    host, _ = pipeline.run_step5(engine, raw, toolrec="host")
    assert piece_bytes(host.toolrec) == piece_bytes(cons.toolrec)


def _bam_stream(path):
    data = open(path, "rb").read()
    assert data.endswith(stream.EOF_BLOCK), path + ": no EOF block"
    out, i = [], 0
    while i < len(data):  # every BGZF block inflates with zlib, its CRC32 and ISIZE hold
        bsize = struct.unpack_from("<H", data, i + 16)[0] + 1
        raw = zlib.decompress(data[i + 18:i + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", data, i + bsize - 8)
        assert zlib.crc32(raw) == crc and len(raw) == isize
        out.append(raw)
        i += bsize
    return b"".join(out)


def _split(bamstream):
    """-> (header text, record bytes)"""
    assert bamstream[:4] == b"BAM\1"
    lt = struct.unpack_from("<i", bamstream, 4)[0]
    text = bamstream[8:8 + lt].decode()
    o = 8 + lt
    nref = struct.unpack_from("<i", bamstream, o)[0]
    o += 4
    for _ in range(nref):
        ln = struct.unpack_from("<i", bamstream, o)[0]
        o += 4 + ln + 4
    return text, bamstream[o:]


def _inputs(tmp, far):
    if far:
        from test_long_span import _long_input
        raw, p, fa, span = _long_input(tmp, n_fam=1500, genome_len=4_000_000)
        assert (span > 20_000).sum() >= 20
        return raw, p, fa
    s = synth.generate("C2", 1500, seed=43, device="cpu", genome_len=300_000)
    raw = R.take(s.raw, np.lexsort((s.raw.pos, s.raw.tid)))
    codes = R.unpack_nibbles(s.ref.packed, s.ref.n_nibbles)
    fa = str(tmp / "g.fa")
    open(fa, "w").write(">%s\n%s\n" % (s.ref.names[0], R.NT16_TO_ASCII[codes].tobytes().decode()))
    hdr = bam.BamHeader("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n@RG\tID:A\tLB:L\n" % (s.ref.names[0], len(codes)),
                        [s.ref.names[0]], np.asarray([len(codes)], np.int64))
    p = str(tmp / "in.bam")
    bam.write_bam(p, hdr, bam.records_to_bam(raw), level=1, threads=4)
    return raw, p, fa


@pytest.mark.parametrize("far", [False, True])
def test_files(engine, tmp_path, far):
    raw, inp, fa = _inputs(tmp_path, far)
    p = lambda n: str(tmp_path / n)  # noqa: E731
    base = ["step5", "--reference", fa, inp, "--threads", "4", "--chunk-mb", "1", "--compression", "1"]
    fq = lambda t: ["--fastq1", p(t + "1.fq.gz"), "--fastq2", p(t + "2.fq.gz")]  # noqa: E731
    assert cli.main(base[:4] + [p("plain.bam")] + base[4:] + fq("plain")) == 0
    assert cli.main(base[:4] + [p("out.bam")] + base[4:] + fq("out") + ["--groupsort-bam", p("g.bam")]) == 0
    for a in ("%s.bam", "%s1.fq.gz", "%s2.fq.gz"):  # the other outputs do not change
        assert open(p(a % "out"), "rb").read() == open(p(a % "plain"), "rb").read(), a
    text, recs_bytes = _split(_bam_stream(p("g.bam")))
    assert toolrec.hd_line(text) == "@HD\tVN:1.6\tSO:unsorted\tGO:query\tSS:unsorted:template-coordinate"
    assert "@PG" not in text and "@RG\tID:A" in text
    # the whole-file path's stream, byte for byte
    assert cli.main(base[:4] + [p("w.bam")] + base[4:] + ["--stream", "false", "--groupsort-bam", p("gw.bam")]) == 0
    assert _bam_stream(p("gw.bam")) == _bam_stream(p("g.bam"))
    # the record multiset is the oracle's
    _, whole = bam.read_bam(inp, threads=4)
    ref = oracle.run(whole, bam.read_fasta(fa, bam.read_bam_header(inp)), threads=8)
    recs = parse(recs_bytes)
    key = lambda name, flag: (bytes(name), int(flag))  # noqa: E731
    src_of = {key(whole.names[int(whole.name_id[k])], whole.flag[k]): k for k in range(whole.n)}
    src = [src_of[key(r["name"], r["flag"])] for r in recs]
    assert len(set(src)) == len(src)
    assert_records_equal_oracle(recs, src, ref, whole, "files far=%s" % far)
    # the same file with the other device paths on
    assert cli.main(base[:4] + [p("d.bam")] + base[4:] + ["--gpu-bam", "true", "--gpu-image", "true",
                                                          "--groupsort-bam", p("gd.bam")]) == 0
    assert _bam_stream(p("gd.bam")) == _bam_stream(p("g.bam"))
    if far:  # small chunks: the far templates are deferred, and the file is assembled from its pieces
        info = bam.step5_stream(inp, fa, p("x.bam"), engine=engine, threads=2, level=1, chunk_bytes=60_000, slack=2000,
                                read_size=16 << 10, defer=1000, groupsort_bam=p("gx.bam"))
        assert info["spliced_families"] > 20 and info["spilled_bytes"] > 0
        assert _bam_stream(p("gx.bam")) == _bam_stream(p("g.bam"))
        gi = info["groupsort_bam"]
        assert gi["records"] == len(recs) and gi["raw_bytes"] == len(recs_bytes)
        assert gi["compressed_bytes"] == len(open(p("gx.bam"), "rb").read())
        assert not [f for f in tmp_path.iterdir() if f.name.startswith(".")], "spill files left behind"
    # closure: callduplex alone on the file is the fused step's consensus
    _, back = bam.read_bam(p("g.bam"), threads=4)
    assert back.n == len(recs)
    engine.load_reference(bam.read_fasta(fa, bam.read_bam_header(inp)))
    c2 = pipeline.run_duplex(engine, back)
    name = lambda r, c, f: r.mi_names[int(c.fam_mi[f])]  # noqa: E731
    assert [name(back, c2, f) for f in range(len(c2.status))] == [name(whole, ref, f) for f in range(len(ref.status))]
    assert np.array_equal((c2.status & 1).astype(np.int32), ref.status) and np.array_equal(c2.length, ref.cons_len)
    fused, _ = pipeline.run_step5(engine, whole)
    assert np.array_equal(fused.status, c2.status) and np.array_equal(fused.length, c2.length)
    for f in range(len(ref.status)):
        for e in range(2):
            n = int(c2.length[f, e])
            assert np.array_equal(c2.seq[f, e, :n], fused.seq[f, e, :n]) and np.array_equal(c2.qual[f, e, :n], fused.qual[f, e, :n])


def test_split_ext_route_and_stream(engine, tmp_path, monkeypatch):
    """A tool-2 group whose extension partners land in different families (one 163 record's stale
    mate contig changed, as test_gpu_parity.test_split_extension_partner_falls_back builds it): the
    tools run as their own launches and the records come from the host twin, in the vote's family
    order -- as a route, and as a streamed file one of whose chunks has such a plan."""
    from bsseqconsensusreads_amd import batch
    s = synth.generate("C0", 400, seed=15, device="cpu", genome_len=100_000)
    raw = s.raw
    raw.next_tid[int(np.nonzero(raw.flag == 163)[0][7])] = 1
    assert batch.build_family_batch(raw, "full", s.ref).split_ext
    engine.load_reference(s.ref)
    cons, _ = pipeline.run_step5(engine, raw, toolrec="device")
    assert [x.event for x in cons.toolrec] == [None]  # the twin's bytes
    recs = parse(piece_bytes(cons.toolrec))
    assert_records_equal_oracle(recs, cons.fam_src, oracle.run(raw, s.ref), raw, "split_ext route")
    assert int(cons.toolrec[0].foff[-1]) == len(piece_bytes(cons.toolrec)) and cons.toolrec[0].fams == len(cons.status)
    # the file: two contigs, so that the stale mate contig is one the header knows
    rng = np.random.default_rng(3)
    codes = R.unpack_nibbles(s.ref.packed, s.ref.n_nibbles)
    names = [s.ref.names[0], "chrX2"]
    ref = R.Reference.from_contigs(names, {names[0]: R.NT16_TO_ASCII[codes].tobytes(),
                                           names[1]: rng.choice(np.frombuffer(b"ACGT", np.uint8), 5000).tobytes()},
                                   keep_letters=False)
    srt = R.take(raw, np.lexsort((raw.pos, raw.tid)))
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in zip(ref.names, ref.lengths)) + \
        "@RG\tID:A\tLB:L\n"
    p = lambda n: str(tmp_path / n)  # noqa: E731
    bam.write_bam(p("in.bam"), bam.BamHeader(text, list(ref.names), np.asarray(ref.lengths, np.int64)),
                  bam.records_to_bam(srt), level=1, threads=2)
    rc = R.unpack_nibbles(ref.packed, ref.n_nibbles)
    with open(p("g.fa"), "wb") as fh:
        for i, n in enumerate(ref.names):
            o, ln = int(ref.contig_off[i]), int(ref.contig_len[i])
            fh.write((">%s\n" % n).encode() + R.NT16_TO_ASCII[rc[o:o + ln]].tobytes() + b"\n")
    kinds = set()
    real = stream._add_toolrec

    def spy(g, pieces, a, b, threads):
        kinds.update("host" if x.event is None else "device" for x in pieces)
        return real(g, pieces, a, b, threads)
    monkeypatch.setattr(stream, "_add_toolrec", spy)
    info = bam.step5_stream(p("in.bam"), p("g.fa"), p("s.bam"), engine=engine, threads=2, level=1, chunk_bytes=60_000,
                            slack=2000, read_size=16 << 10, defer=0, groupsort_bam=p("gs.bam"))
    assert "host" in kinds, kinds  # a chunk with a split_ext plan went through the twin
    bam.step5(p("in.bam"), p("g.fa"), p("w.bam"), engine=engine, threads=2, level=1, groupsort_bam=p("gw.bam"))
    assert open(p("s.bam"), "rb").read() == open(p("w.bam"), "rb").read()
    assert _bam_stream(p("gs.bam")) == _bam_stream(p("gw.bam"))
    _, whole = bam.read_bam(p("in.bam"), threads=2)
    recs = parse(_split(_bam_stream(p("gs.bam")))[1])
    assert info["groupsort_bam"]["records"] == len(recs)
    key = lambda name, flag: (bytes(name), int(flag))  # noqa: E731
    src_of = {key(whole.names[int(whole.name_id[k])], whole.flag[k]): k for k in range(whole.n)}
    src = [src_of[key(r["name"], r["flag"])] for r in recs]
    assert_records_equal_oracle(recs, src, oracle.run(whole, bam.read_fasta(p("g.fa"), bam.read_bam_header(p("in.bam")))),
                                whole, "split_ext file")

"""The streaming writers' paths that only larger tests reach (bam.BamWriter / bam.FastqWriter):
fragments, flush cuts, raw appends, closing twice and after a failed add -- each on the host
deflate path and on the GPU-compressed path with oracle.BgzfStandIn in the GPU's place (every 7th
block of a job through the writer's host fallback).  Python classes only; what the files hold is
read back with bam.read_bam and gzip."""
import dataclasses
import gzip
import os
import struct

import numpy as np
import pytest

from bsseqconsensusreads_amd import bam, synth
from oracle import oracle
from test_bam import _cons_of, _header

EOF_BLOCK = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
FIELDS = ("flag", "tid", "pos", "mapq", "l_seq", "seq_off", "seq", "qual", "cig_off", "n_cig", "cigar", "next_tid",
          "next_pos", "tlen", "name_id", "mi_id", "mi_strand")
MODES = ("host", "standin")


def _gpu(mode):
    return oracle.BgzfStandIn() if mode == "standin" else None


def _read(path):
    return open(path, "rb").read()


def _record_bytes(data: bytes) -> bytes:
    """an inflated BAM's bytes past its header"""
    l_text, = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, p)
        p += 4 + l_name + 4
    return data[p:]


def _count_records(rec: bytes) -> int:
    """block_size-prefixed records filling `rec` exactly -> their count"""
    p = n = 0
    while p < len(rec):
        assert p + 4 <= len(rec)
        p += 4 + struct.unpack_from("<i", rec, p)[0]
        n += 1
    assert p == len(rec)
    return n


def _part(recs, lo, hi):
    return bam.take_records(recs, np.arange(lo, hi))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """(header, records, their three even cuts, write_bam's file read back, write_fastq's texts);
    680 families: the smallest round count whose FASTQ files pass three whole blocks (600 give 2.9)"""
    d = tmp_path_factory.mktemp("whole")
    s = synth.generate("C2", 680, seed=11, device="cpu", genome_len=300_000)
    recs = bam.duplex_records(_cons_of(oracle.run(s.raw, s.ref)), s.raw, "x")
    hdr = bam.output_header(_header(s.ref))
    whole = str(d / "whole.bam")
    bam.write_bam(whole, hdr, recs, 5, 2)
    fq = (str(d / "w1.fq.gz"), str(d / "w2.fq.gz"))
    bam.write_fastq(fq[0], fq[1], recs, 5, 2)
    texts = tuple(gzip.decompress(_read(p)) for p in fq)
    # at least 3 whole blocks per file, so that every writer below takes, puts and cuts whole blocks
    assert len(gzip.decompress(_read(whole))) >= 3 * 65280
    assert min(len(t) for t in texts) >= 3 * 65280
    cuts = [0, recs.n // 3 & ~1, 2 * recs.n // 3 & ~1, recs.n]
    return hdr, recs, cuts, bam.read_bam(whole), texts


def _assert_same(got, want):
    (hg, rg), (hw, rw) = got, want
    assert hg.text == hw.text and list(hg.ref_names) == list(hw.ref_names)
    assert np.array_equal(hg.ref_lens, hw.ref_lens)
    assert rg.n == rw.n
    for k in FIELDS:
        assert np.array_equal(getattr(rg, k), getattr(rw, k)), k
    for k in ("names", "aux"):
        assert np.array_equal(getattr(rg, k).buf, getattr(rw, k).buf), k
        assert np.array_equal(getattr(rg, k).off, getattr(rw, k).off), k


@pytest.mark.parametrize("mode", MODES)
def test_fragments_concatenate_to_the_whole_file(data, mode, tmp_path):
    """"first" / "next" fragments over a split of the records, concatenated, plus the EOF block,
    read back as write_bam's file; and a writer cut with flush() at the same records holds the
    fragments' bytes, its pieces ending at the offsets flush() returned."""
    hdr, recs, cuts, want, _ = data
    pieces = []
    for i in range(3):
        p = str(tmp_path / ("piece%d.bam" % i))
        w = bam.BamWriter(p, hdr, 5, gpu=_gpu(mode), fragment="first" if i == 0 else "next")
        mid = (cuts[i] + cuts[i + 1]) // 2 & ~1  # (two adds: on the GPU path a job is in flight at the second)
        w.add(_part(recs, cuts[i], mid), 2)
        w.add(_part(recs, mid, cuts[i + 1]), 2)
        w.close(2)
        pieces.append(_read(p))
        assert not pieces[-1].endswith(EOF_BLOCK)
    cat = str(tmp_path / "cat.bam")
    with open(cat, "wb") as f:
        f.write(b"".join(pieces) + EOF_BLOCK)
    _assert_same(bam.read_bam(cat), want)

    cut = str(tmp_path / "cut.bam")
    w = bam.BamWriter(cut, hdr, 5, gpu=_gpu(mode))
    offs = []
    for i in range(3):
        mid = (cuts[i] + cuts[i + 1]) // 2 & ~1
        w.add(_part(recs, cuts[i], mid), 2)
        w.add(_part(recs, mid, cuts[i + 1]), 2)
        offs.append(w.flush(2))
    w.close(2)
    got = _read(cut)
    assert offs == [len(pieces[0]), len(pieces[0]) + len(pieces[1]), sum(len(p) for p in pieces)]
    assert [got[:offs[0]], got[offs[0]:offs[1]], got[offs[1]:offs[2]]] == pieces
    assert got[offs[2]:] == EOF_BLOCK


@pytest.mark.parametrize("mode", MODES)
def test_bam_flush_returns_the_length_at_a_record_boundary(data, mode, tmp_path):
    hdr, recs, cuts, want, _ = data
    p = str(tmp_path / "f.bam")
    g = _gpu(mode)
    w = bam.BamWriter(p, hdr, 5, gpu=g)
    w.add(_part(recs, 0, cuts[2]), 2)
    if g is not None:
        assert w.pending is not None  # a job in flight: the flush must drain it before the tell
    off = w.flush(2)
    assert isinstance(off, int) and off == os.path.getsize(p)
    if g is not None:
        assert w.pending is None and g.job is None
    head = _read(p)
    assert _count_records(_record_bytes(gzip.decompress(head))) == cuts[2]
    w.add(_part(recs, cuts[2], recs.n), 2)
    w.close(2)
    assert _read(p)[:off] == head and os.path.getsize(p) > off
    _assert_same(bam.read_bam(p), want)


@pytest.mark.parametrize("mode", MODES)
def test_fastq_flush_returns_both_lengths_at_a_pair_boundary(data, mode, tmp_path):
    hdr, recs, cuts, _, texts = data
    p = (str(tmp_path / "f1.fq.gz"), str(tmp_path / "f2.fq.gz"))
    g = _gpu(mode)
    w = bam.FastqWriter(p[0], p[1], 5, gpu=g)
    w.add(_part(recs, 0, cuts[2]), 2)
    if g is not None:
        assert w.pending is not None
    offs = w.flush(2)
    assert isinstance(offs, tuple) and len(offs) == 2
    assert offs == (os.path.getsize(p[0]), os.path.getsize(p[1]))
    if g is not None:
        assert w.pending is None and g.job is None
    heads = [gzip.decompress(_read(x)[:o]) for x, o in zip(p, offs)]
    for h, t in zip(heads, texts):
        assert t.startswith(h) and h.endswith(b"\n")
    assert heads[0].count(b"\n") == heads[1].count(b"\n") == 4 * (cuts[2] // 2)  # the same pairs in both
    w.add(_part(recs, cuts[2], recs.n), 2)
    w.close(2)
    assert tuple(gzip.decompress(_read(x)) for x in p) == texts


@pytest.mark.parametrize("mode", MODES)
def test_raw_append_then_add_keeps_the_order(data, mode, tmp_path):
    hdr, recs, cuts, want, _ = data
    first = str(tmp_path / "first.bam")
    bam.write_bam(first, hdr, _part(recs, 0, cuts[1]), 1, 2)
    raw = _record_bytes(gzip.decompress(_read(first)))
    assert _count_records(raw) == cuts[1] and len(raw) > 65280
    p = str(tmp_path / "r.bam")
    w = bam.BamWriter(p, hdr, 5, gpu=_gpu(mode))
    w.add_raw(raw, 2)
    w.add_raw(b"", 2)
    w.add(_part(recs, cuts[1], recs.n), 2)
    w.close(2)
    _assert_same(bam.read_bam(p), want)


@pytest.mark.parametrize("mode", MODES)
def test_close_twice_and_after_a_failed_add(data, mode, tmp_path):
    hdr, recs, cuts, _, _ = data
    g = _gpu(mode)
    w = bam.BamWriter(str(tmp_path / "a.bam"), hdr, 5, gpu=g)
    f = bam.FastqWriter(str(tmp_path / "a1.fq.gz"), str(tmp_path / "a2.fq.gz"), 5, gpu=_gpu(mode))
    for x in (w, f):
        x.add(_part(recs, 0, cuts[1]), 2)
    two = _part(recs, cuts[1], cuts[1] + 2)
    bad = dataclasses.replace(two, names=bam.StringTable.from_list([b"n" * 255] * 2))
    with pytest.raises(OSError, match="too long for BAM"):
        w.add(bad, 2)
    bam.close_quietly(w, f, None)
    assert not w.h and not f.h
    assert w.pending is None and f.pending is None and (g is None or g.job is None)
    for x in (w, f):  # closed already: nothing to do, nothing raised
        x.close(2)
        x.close()
    bam.close_quietly(w, f)
    # what the good add wrote stands: the handles' files were closed, with their EOF blocks
    h, r = bam.read_bam(str(tmp_path / "a.bam"))
    assert r.n == cuts[1]
    assert gzip.decompress(_read(str(tmp_path / "a1.fq.gz"))).count(b"\n") == 4 * (cuts[1] // 2)


def test_moved_names_stay_importable_from_bam():
    """the codecs and writers live in bgzf.py; bam.<name> is the same object, and the streaming
    steps still resolve through the same module __getattr__"""
    from bsseqconsensusreads_amd import bgzf, stream
    for name in ("GpuBgzf", "GpuInflate", "_BgzfWriter", "BamWriter", "FastqWriter", "close_quietly"):
        assert getattr(bam, name) is getattr(bgzf, name), name
        assert name not in vars(bam), name
    assert bam.step5_stream is stream.step5_stream and bam.molecular_stream is stream.molecular_stream
    with pytest.raises(AttributeError):
        bam.no_such_name

"""cli zipper: bwameth's alignment of the step-1 FASTQ pair with MI, RX, RG
and the consensus tags put back from the step-1 BAM, unmapped records dropped, coordinate-sorted --
the file rules mergeAunA_consensus and mergeAunA_consensus_grepaligned leave (`samtools sort -n |
fgbio ZipperBams --unmapped .. --sort Coordinate`, then `samtools view -F 4`; main.snake.py:97-119),
the input of cli step5.  fgbio ZipperBams restated, parity unpinned.

* ``read_records`` -- a BAM's header and its record bytes as they lie in the file (both files are
  read whole), listed by bsdc_zip_scan_host.
* ``join``    -- every aligned record's partner: the UNMAPPED record of the same read name (bytes
  compared, by the rank of bam.table_ranks) and the same end (flag bits 0x40 / 0x80).
* ``tables``  -- the kept records' table (bsdc_zip_rec), the partners' aux bytes and the sort keys.
* ``header``  -- rule 7's header.
* ``zipper``  -- the driver: keys sorted (bsdc_zip_sort) and records written (bsdc_zip_format) on
  one GPU, then checksummed, deflated and packed there behind the BAM writer's sink.  host=True
  runs the host twins and the host deflate instead: for the tests, never chosen by cli.
  stream=True: the same file with bounded memory (zipper_stream.py: sorted runs, merged on the GPU).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import bam
from .toolrec import _ragged

CONSENSUS_REVERSE = ("ad", "ae", "bd", "be", "cd", "ce", "aq", "bq")  # the word Consensus in --tags-to-reverse
CONSENSUS_REVCOMP = ("ac", "bc")                                      # ... and in --tags-to-revcomp


def _block_raw(path: str, block: bytes, at: int) -> bytes:
    """One whole BGZF block (which starts at byte `at` of the file) inflated, its CRC32 and ISIZE checked."""
    raw = zlib.decompress(block[18:-8], -15)
    crc, isize = struct.unpack_from("<II", block, len(block) - 8)
    if len(raw) != isize or zlib.crc32(raw) != crc:
        raise OSError("%s: corrupt BGZF block at byte %d" % (path, at))
    return raw


def _inflate(path: str, threads: int = 0) -> bytes:
    """A BGZF file's uncompressed bytes (every block's CRC32 and ISIZE checked)."""
    data = open(path, "rb").read()
    cuts, i = [], 0
    while i < len(data):
        if i + 18 > len(data) or data[i:i + 4] != b"\x1f\x8b\x08\x04" or data[i + 12:i + 14] != b"BC":
            raise OSError("%s: not a BGZF block at byte %d" % (path, i))
        bsize = struct.unpack_from("<H", data, i + 16)[0] + 1
        if bsize < 26 or i + bsize > len(data):
            raise OSError("%s: truncated BGZF block at byte %d" % (path, i))
        cuts.append((i, bsize))
        i += bsize

    def one(c):
        a, n = c
        return _block_raw(path, data[a:a + n], a)
    if threads > 1 and len(cuts) > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(int(threads)) as ex:
            return b"".join(ex.map(one, cuts, chunksize=64))
    return b"".join(one(c) for c in cuts)


def _aligned_copy(b: bytes) -> np.ndarray:
    """bytes as a uint8 array in numpy's own (aligned) allocation, padded to a non-empty multiple of 4"""
    n = len(b)
    out = np.zeros(max((n + 3) // 4 * 4, 4), np.uint8)
    out[:n] = np.frombuffer(b, np.uint8)
    return out


@dataclass
class Records:
    """A BAM read whole: its header, its record bytes back to back (padded; n_bytes of them are
    records) and their list (_lib.ZIP_SRC)."""
    header: bam.BamHeader
    buf: np.ndarray
    n_bytes: int
    src: np.ndarray

    @property
    def n(self) -> int:
        return int(self.src.shape[0])

    def name(self, k: int) -> bytes:
        o = int(self.src["off"][k]) + 36
        return self.buf[o:o + int(self.src["name_len"][k])].tobytes()


def scan(buf: np.ndarray, n_bytes: int) -> np.ndarray:
    """The records of buf[:n_bytes] listed (bsdc_zip_scan_host)."""
    lib = _lib.load()
    n = int(lib.bsdc_zip_scan_host(buf.ctypes.data, int(n_bytes), None, 0))
    if n < 0:
        raise ValueError(lib.bsdc_zip_last_error().decode())
    src = np.zeros(n, _lib.ZIP_SRC)
    if n and lib.bsdc_zip_scan_host(buf.ctypes.data, int(n_bytes), src.ctypes.data, n) != n:
        raise ValueError(lib.bsdc_zip_last_error().decode())
    return src


def scan_prefix(buf: np.ndarray, n_bytes: int):
    """The whole records at the front of buf[:n_bytes] listed (bsdc_zip_scan_prefix_host) -> (their
    list, the bytes they take): a record cut by the end is left to the caller's next piece."""
    lib = _lib.load()
    used = C.c_int64(0)
    n = int(lib.bsdc_zip_scan_prefix_host(buf.ctypes.data, int(n_bytes), None, 0, C.byref(used)))
    if n < 0:
        raise ValueError(lib.bsdc_zip_last_error().decode())
    src = np.zeros(n, _lib.ZIP_SRC)
    if n and lib.bsdc_zip_scan_prefix_host(buf.ctypes.data, int(n_bytes), src.ctypes.data, n, C.byref(used)) != n:
        raise ValueError(lib.bsdc_zip_last_error().decode())
    return src, int(used.value)


def parse_header(path: str, data: bytes):
    """The BAM header at the front of the inflated bytes -> (BamHeader, the first record's byte)"""
    if data[:4] != b"BAM\1" or len(data) < 12:
        raise OSError("%s: not a BAM" % path)
    lt = struct.unpack_from("<i", data, 4)[0]
    text = data[8:8 + lt].split(b"\0", 1)[0].decode(errors="replace")
    o = 8 + lt
    nref = struct.unpack_from("<i", data, o)[0]
    o += 4
    names, lens = [], []
    for _ in range(nref):
        ln = struct.unpack_from("<i", data, o)[0]
        names.append(data[o + 4:o + 4 + ln - 1].decode())
        lens.append(struct.unpack_from("<i", data, o + 4 + ln)[0])
        o += 8 + ln
    return bam.BamHeader(text, names, np.asarray(lens, np.int64)), o


def read_records(path: str, threads: int = 0) -> Records:
    data = _inflate(path, threads)
    hdr, o = parse_header(path, data)
    buf = _aligned_copy(data[o:])
    n_bytes = len(data) - o
    try:
        src = scan(buf, n_bytes)
    except ValueError as e:
        raise OSError("%s: %s" % (path, e)) from None
    return Records(hdr, buf, n_bytes, src)


def tag_list(names: Optional[Sequence[str]], consensus: Tuple[str, ...]) -> Tuple[bytes, ...]:
    """--tags-to-* values as two-byte names, the word Consensus expanded, in order, once each."""
    out = []
    for x in names or ():
        for t in (consensus if x == "Consensus" else (x,)):
            b = t.encode() if isinstance(t, str) else bytes(t)
            if len(b) != 2:
                raise ValueError("a tag name has two letters: %r" % (x,))
            if b not in out:
                out.append(b)
    if len(out) > _lib.ZIP_MAX_TAGS:
        raise ValueError("more than %d tag names in one list" % _lib.ZIP_MAX_TAGS)
    return tuple(out)


def tags_struct(reverse=(), revcomp=(), remove=()) -> "_lib.ZipTagsC":
    t = _lib.ZipTagsC()
    for field, names in (("reverse", reverse), ("revcomp", revcomp), ("remove", remove)):
        arr = getattr(t, field)
        for k, b in enumerate(names):
            arr[2 * k], arr[2 * k + 1] = b[0], b[1]
        setattr(t, "n_" + field, len(names))
    return t


def _name_ranks(a: Records, u: Records):
    """Byte-order ranks of the read names of both files in one table -> (of a's records, of u's)"""
    off = np.concatenate([a.src["off"] + 36, u.src["off"] + 36 + a.buf.shape[0]])
    ln = np.concatenate([a.src["name_len"], u.src["name_len"]]).astype(np.int64)
    both = np.concatenate([a.buf, u.buf])
    o = np.zeros(ln.shape[0] + 1, np.int64)
    o[1:] = np.cumsum(ln)
    rank = bam.table_ranks(bam.StringTable(both[_ragged(off, ln)], o))
    return rank[:a.n], rank[a.n:]


def join(a: Records, u: Records):
    """Rule 1 -> (partner [a.n]: each aligned record's record of UNMAPPED, the templates of
    UNMAPPED with no aligned record).  Names are compared as bytes, whole: bsdc_fastq_write names
    the reads NAME/1 and NAME/2 and bwa mem trims that suffix, so ALIGNED carries NAME again; an
    aligner that keeps the suffix leaves reads without a partner, which is an error here."""
    ra, ru = _name_ranks(a, u)
    ka = ra * 4 + ((a.src["flag"].astype(np.int64) >> 6) & 3)
    ku = ru * 4 + ((u.src["flag"].astype(np.int64) >> 6) & 3)
    order = np.argsort(ku, kind="stable")
    kus = ku[order]
    dup = np.nonzero(kus[1:] == kus[:-1])[0]
    if dup.shape[0]:
        k = int(order[dup[0] + 1])
        raise ValueError("UNMAPPED holds read %r (flag %d) twice" % (u.name(k).decode(errors="replace"), int(u.src["flag"][k])))
    at = np.searchsorted(kus, ka)
    ok = at < kus.shape[0]
    ok[ok] = kus[at[ok]] == ka[ok]
    if not ok.all():
        k = int(np.nonzero(~ok)[0][0])
        raise ValueError("aligned read %r (flag %d) has no partner in UNMAPPED" % (
            a.name(k).decode(errors="replace"), int(a.src["flag"][k])))
    lonely = int(np.setdiff1d(np.unique(ru), np.unique(ra)).shape[0])
    return order[at] if a.n else np.zeros(0, np.int64), lonely


@dataclass
class Tables:
    """What the kernels read besides ALIGNED's record bytes: tab [n] (_lib.ZIP_REC, the kept
    records in ALIGNED's order), part (the partners' aux bytes, padded), keys / idx (the sort's
    input: idx = 0..n-1), the largest refID and pos."""
    tab: np.ndarray
    part: np.ndarray
    keys: np.ndarray
    idx: np.ndarray
    max_ref: int
    max_pos: int

    @property
    def n(self) -> int:
        return int(self.tab.shape[0])


def sort_keys(ref_id, pos, flag) -> np.ndarray:
    """refID << 32 | (pos + 1) << 1 | reverse"""
    return (np.asarray(ref_id).astype(np.uint64) << np.uint64(32)) | \
        ((np.asarray(pos).astype(np.int64) + 1).astype(np.uint64) << np.uint64(1)) | \
        ((np.asarray(flag).astype(np.uint64) >> np.uint64(4)) & np.uint64(1))


def tables(a: Records, u: Records, partner: np.ndarray) -> Tables:
    """Rules 2 and 6's inputs: the records of ALIGNED without flag 0x4, each with its partner's aux."""
    keep = np.nonzero((a.src["flag"] & 4) == 0)[0]
    p = u.src[np.asarray(partner, np.int64)[keep]]
    pl = (p["len"] - p["aux"]).astype(np.int64)
    return kept_tables(a, keep, pl, p["flag"], u.buf[_ragged(p["off"] + p["aux"], pl)])


def kept_tables(a: Records, keep: np.ndarray, pl: np.ndarray, pflag: np.ndarray, part: np.ndarray) -> Tables:
    """tables() of the kept records a.src[keep], given their partners' aux lengths, flags and aux
    bytes back to back (what a chunk of --stream true holds of UNMAPPED)."""
    s = a.src[keep]
    bad = np.nonzero((s["ref_id"] < 0) | (s["pos"] < -1))[0]
    if bad.shape[0]:
        raise ValueError("aligned read %r is mapped (no flag 0x4) but has no reference or position" % (
            a.name(int(keep[bad[0]])).decode(errors="replace"),))
    n = int(keep.shape[0])
    tab = np.zeros(n, _lib.ZIP_REC)
    tab["rec_off"], tab["rec_len"], tab["aux_start"] = s["off"], s["len"], s["aux"]
    tab["part_len"] = pl
    tab["part_off"] = np.cumsum(pl) - pl
    tab["flag_or"] = pflag & 0x200
    part = np.concatenate([part, np.zeros((-int(part.shape[0])) % 4 or (4 if part.shape[0] == 0 else 0), np.uint8)])
    return Tables(tab, part, sort_keys(s["ref_id"], s["pos"], s["flag"]), np.arange(n, dtype=np.uint32),
                  int(s["ref_id"].max()) if n else 0, int(s["pos"].max()) if n else 0)


def header(ha: bam.BamHeader, hu: bam.BamHeader) -> bam.BamHeader:
    """Rule 7: @HD VN:1.6 SO:coordinate; ALIGNED's @SQ lines and reference list; UNMAPPED's @RG
    lines; ALIGNED's @PG lines, then UNMAPPED's whose ID is new; both files' @CO lines."""
    la = [x for x in ha.text.split("\n") if x]
    lu = [x for x in hu.text.split("\n") if x]
    pg_id = lambda line: next((f[3:] for f in line.split("\t")[1:] if f.startswith("ID:")), None)  # noqa: E731
    pg = [x for x in la if x.startswith("@PG")]
    seen = {pg_id(x) for x in pg}
    for x in lu:
        if x.startswith("@PG") and pg_id(x) not in seen:
            pg.append(x)
            seen.add(pg_id(x))
    lines = ["@HD\tVN:1.6\tSO:coordinate"] + [x for x in la if x.startswith("@SQ")] + \
        [x for x in lu if x.startswith("@RG")] + pg + [x for x in la + lu if x.startswith("@CO")]
    return bam.BamHeader("\n".join(lines) + "\n", list(ha.ref_names), np.asarray(ha.ref_lens, np.int64))


def sort_host(keys: np.ndarray, idx: np.ndarray, max_ref: int, max_pos: int):
    """bsdc_zip_sort_host on copies -> (keys, idx) sorted"""
    lib = _lib.load()
    k = np.ascontiguousarray(keys, np.uint64).copy() if keys.shape[0] else np.zeros(1, np.uint64)
    v = np.ascontiguousarray(idx, np.uint32).copy() if idx.shape[0] else np.zeros(1, np.uint32)
    n = int(keys.shape[0])
    if lib.bsdc_zip_sort_host(k.ctypes.data, v.ctypes.data, n, int(max_ref), int(max_pos)) != 0:
        raise ValueError("bsdc_zip_sort_host failed: %s" % lib.bsdc_zip_last_error().decode())
    return k[:n], v[:n]


def bound(tab: np.ndarray) -> int:
    t = np.ascontiguousarray(tab) if tab.shape[0] else np.zeros(1, _lib.ZIP_REC)
    return int(_lib.load().bsdc_zip_bytes_bound(t.ctypes.data, int(tab.shape[0])))


def format_host(idx: np.ndarray, tab: np.ndarray, rec: np.ndarray, part: np.ndarray, tags, cap: Optional[int] = None,
                fill: Optional[int] = None):
    """bsdc_zip_format_host -> (off int64 [n + 1], the buffer uint8 [cap]): the records are buf[:off[n]]."""
    lib = _lib.load()
    n = int(tab.shape[0])
    t = np.ascontiguousarray(tab) if n else np.zeros(1, _lib.ZIP_REC)
    ix = np.ascontiguousarray(idx, np.uint32) if n else np.zeros(1, np.uint32)
    cap = bound(tab) if cap is None else int(cap)
    buf = np.empty(max(cap, 1), np.uint8) if fill is None else np.full(max(cap, 1), fill, np.uint8)
    off = np.zeros(n + 1, np.int64)
    rc = lib.bsdc_zip_format_host(ix.ctypes.data, n, t.ctypes.data, rec.ctypes.data, int(rec.shape[0]), part.ctypes.data,
                                  int(part.shape[0]), C.byref(tags), off.ctypes.data, buf.ctypes.data, cap)
    if rc != 0:
        raise ValueError("bsdc_zip_format_host failed (%d): %s" % (rc, lib.bsdc_zip_last_error().decode()))
    return off, buf


def format_device(device, t: Tables, rec: np.ndarray, tags):
    """The sort and the record writer on the GPU -> (the records' uint8 device tensor, their byte
    count, an event behind the kernels)."""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    n = t.n
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    with torch.cuda.device(dev):
        one = np.zeros(1, _lib.ZIP_REC)
        d_keys = up(t.keys if n else np.zeros(1, np.uint64))
        d_idx = up(t.idx if n else np.zeros(1, np.uint32))
        d_tab = up(t.tab if n else one)
        d_rec, d_part = up(rec), up(t.part)
        cap = bound(t.tab)
        dst = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        tmp = torch.empty(int(max(lib.bsdc_zip_sort_tmp_bytes(n), lib.bsdc_zip_format_tmp_bytes(n))), dtype=torch.uint8,
                          device=dev)
        st = torch.cuda.current_stream(dev)
        tab_h = np.ascontiguousarray(t.tab) if n else one
        rc = lib.bsdc_zip_sort(d_keys.data_ptr(), d_idx.data_ptr(), n, t.max_ref, t.max_pos, tmp.data_ptr(),
                               C.c_void_p(st.cuda_stream))
        if rc == 0:
            rc = lib.bsdc_zip_format(d_idx.data_ptr(), n, d_tab.data_ptr(), tab_h.ctypes.data, d_rec.data_ptr(),
                                     rec.ctypes.data, int(rec.shape[0]), d_part.data_ptr(), t.part.ctypes.data,
                                     int(t.part.shape[0]), C.byref(tags), off.data_ptr(), dst.data_ptr(), cap,
                                     tmp.data_ptr(), C.c_void_p(st.cuda_stream))
        if rc != 0:
            st.synchronize()
            raise ValueError("cli zipper's kernels failed (%d): %s" % (rc, lib.bsdc_zip_last_error().decode()))
        total = int(off[n].item())  # (synchronises the stream)
        ev = torch.cuda.Event()
        ev.record(st)
    return dst, total, ev


def zipper(aligned: str, unmapped: str, out: str, tags_to_reverse: Sequence[str] = (), tags_to_revcomp: Sequence[str] = (),
           tags_to_remove: Sequence[str] = (), threads: int = 0, level: int = 6, device=0, info: Optional[str] = None,
           host: bool = False, stream: bool = False, chunk_bytes: Optional[int] = None, tmp_dir: Optional[str] = None) -> dict:
    """ALIGNED.bam + UNMAPPED.bam -> OUT.bam (module docstring; rules in DESIGN.md 3.11).  Both
    inputs are read whole, unless `stream`: then memory is bounded by chunk_bytes (sorted runs under
    tmp_dir, merged on the GPU: zipper_stream.py).  -> the info dict (also written to `info` as JSON)."""
    from . import bgzf
    if stream:
        from . import zipper_stream
        return zipper_stream.zipper_stream(aligned, unmapped, out, tags_to_reverse, tags_to_revcomp, tags_to_remove, threads,
                                           level, device, info, host, chunk_bytes, tmp_dir)
    a, u = read_records(aligned, threads), read_records(unmapped, threads)
    tags = tags_struct(tag_list(tags_to_reverse, CONSENSUS_REVERSE), tag_list(tags_to_revcomp, CONSENSUS_REVCOMP),
                       tag_list(tags_to_remove, ()))
    partner, lonely = join(a, u)
    t = tables(a, u, partner)
    hdr = header(a.header, u.header)
    if host:
        _, idx = sort_host(t.keys, t.idx, t.max_ref, t.max_pos)
        off, buf = format_host(idx, t.tab, a.buf, t.part, tags)
        total = int(off[-1])
        w = bgzf.BamWriter(out, hdr, level)
        try:
            w.add_raw(buf[:total].tobytes(), threads)
        finally:
            w.close(threads)
    else:
        dst, total, ev = format_device(device, t, a.buf, tags)
        w = bgzf.BamWriter(out, hdr, level, bgzf.GpuBgzf(dst.device))
        try:
            if total:
                w.add_device([[(dst, 0, total, ev)]], threads)
        finally:
            w.close(threads)
    res = {"records_in": a.n, "unmapped_records_in": u.n, "records_out": t.n, "unmapped_dropped": a.n - t.n,
           "templates_without_aligned": lonely, "raw_bytes": total, "compressed_bytes": os.path.getsize(out)}
    if info is not None:
        with open(info, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")
    return res

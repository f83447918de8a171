"""cli zipper --stream true (DESIGN.md 3.11 "Streaming", 8.12): zipper.zipper's output with memory
bounded by chunk_bytes, whatever the inputs' size.

bwa mem keeps its input's template order, and its input is the FASTQ pair written in UNMAPPED's
order, so ALIGNED's templates are a subsequence of UNMAPPED's: the two files are walked in lockstep
and no name is ranked.

Phase 1, runs: both files are read a bounded number of BGZF blocks at a time (``Templates``), the
templates joined as they pass (``_Walk``), and ALIGNED's templates collected into chunks of about
chunk_bytes (``_Chunk``).  A chunk is sorted and written by the whole-file path's kernels
(bsdc_zip_sort, bsdc_zip_format).  The only chunk goes straight to OUT; of several, each becomes a
run file of records back to back.
Phase 2, merge (``_merge``): every run has a window of whole records; a round emits the records up to
the least last key of the runs that still have unread records, sorts the round's keys
(bsdc_zip_sort: stable, so ties stay in run order, which is ALIGNED's order) and moves the records
into place on the GPU (bsdc_zip_gather).
host=True runs the host twins throughout: for the tests, never chosen by cli.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import shutil
import struct
import tempfile
from typing import Optional

import numpy as np

from . import _lib
from . import zipper as Z
from .toolrec import _ragged

DEFAULT_CHUNK_BYTES = 1 << 30  # --chunk-mb 1024
MAX_RUNS = 1 << 16             # every run needs a window of at least one record at once
BGZF_BLOCK = 1 << 16


class _Blocks:
    """A BGZF file's uncompressed bytes, a bounded number of blocks at a time (each block's CRC32
    and ISIZE checked, as zipper._inflate does)."""

    def __init__(self, path: str, threads: int = 0):
        self.path, self.fh, self.at = path, open(path, "rb"), 0
        self.pool = None
        if threads > 1:
            from concurrent.futures import ThreadPoolExecutor
            self.pool = ThreadPoolExecutor(int(threads))

    def read(self, nblk: int) -> Optional[bytes]:
        """the next nblk blocks' bytes; None at the end of the file"""
        blocks = []
        while len(blocks) < nblk:
            head = self.fh.read(18)
            if not head:
                break
            if len(head) < 18 or head[:4] != b"\x1f\x8b\x08\x04" or head[12:14] != b"BC":
                raise OSError("%s: not a BGZF block at byte %d" % (self.path, self.at))
            bsize = struct.unpack_from("<H", head, 16)[0] + 1
            rest = self.fh.read(bsize - 18) if bsize >= 26 else b""
            if bsize < 26 or len(rest) != bsize - 18:
                raise OSError("%s: truncated BGZF block at byte %d" % (self.path, self.at))
            blocks.append((head + rest, self.at))
            self.at += bsize
        if not blocks:
            return None
        one = lambda b: Z._block_raw(self.path, b[0], b[1])  # noqa: E731
        return b"".join(self.pool.map(one, blocks) if self.pool and len(blocks) > 1 else map(one, blocks))

    def close(self):
        self.fh.close()
        if self.pool is not None:
            self.pool.shutdown()


def same_name_as_previous(buf: np.ndarray, src: np.ndarray) -> np.ndarray:
    """per record: its read name is the record's before it (bytes, whole); False for the first"""
    n = int(src.shape[0])
    same = np.zeros(n, bool)
    if n < 2:
        return same
    ln = src["name_len"].astype(np.int64)
    cand = np.nonzero(ln[1:] == ln[:-1])[0] + 1
    if cand.shape[0] == 0:
        return same
    l = ln[cand]  # (>= 1: the scan refuses an empty name)
    diff = buf[_ragged(src["off"][cand] + 36, l)] != buf[_ragged(src["off"][cand - 1] + 36, l)]
    same[cand] = np.add.reduceat(diff.astype(np.int64), np.cumsum(l) - l) == 0
    return same


class Piece:
    """Whole templates of one file: buf[:n_bytes] holds the records src; template t is records
    tstart[t] .. tstart[t + 1] - 1."""

    def __init__(self, buf, n_bytes, src, tstart):
        self.buf, self.n_bytes, self.src, self.tstart = buf, n_bytes, src, tstart
        first = src[tstart[:-1]]
        self.names = [buf[o:o + l].tobytes() for o, l in zip((first["off"] + 36).tolist(), first["name_len"].tolist())]
        self.t = 0  # the walk's cursor

    @property
    def nt(self) -> int:
        return len(self.names)


class Templates:
    """A BAM read a piece at a time: the header, then pieces of whole templates (a template = a
    maximal run of consecutive records with one read name).  The bytes behind the last whole
    template of a piece -- the template that may go on, and the cut record -- are carried to the next."""

    def __init__(self, path: str, threads: int, nblk: int):
        self.path, self.nblk, self.rd = path, max(int(nblk), 1), _Blocks(path, threads)
        self.eof, self.records, self.held = False, 0, 0
        data = b""
        while True:
            more = self.rd.read(self.nblk)
            if more is None:
                self.eof = True
            else:
                data += more
            try:
                self.header, o = Z.parse_header(path, data)
                if o <= len(data):
                    break
            except struct.error:
                pass
            if self.eof:
                raise OSError("%s: not a BAM" % path)
        self.carry = data[o:]
        self.held = len(self.carry)

    def next(self) -> Optional[Piece]:
        while True:
            more = None if self.eof else self.rd.read(self.nblk)
            if more is None:
                self.eof = True
                more = b""
            data = self.carry + more if more else self.carry
            self.held = len(data)
            if not data:
                return None
            buf = Z._aligned_copy(data)
            try:
                src, used = Z.scan_prefix(buf, len(data))
            except ValueError as e:
                raise OSError("%s: %s" % (self.path, e)) from None
            n = int(src.shape[0])
            if self.eof and used != len(data):
                raise OSError("%s: record %d: truncated" % (self.path, self.records + n))
            starts = np.nonzero(~same_name_as_previous(buf, src))[0]
            keep = n if self.eof else (int(starts[-1]) if n else 0)  # (the last template may go on)
            if keep == 0:
                self.carry = data
                continue
            cut = used if keep == n else int(src["off"][keep])
            self.carry = data[cut:]
            self.held = len(self.carry)
            self.records += keep
            return Piece(buf, cut, src[:keep], np.append(starts[starts < keep], keep).astype(np.int64))

    def close(self):
        self.rd.close()


def _check_twice(p: Piece):
    """rule 1's "twice" error inside the templates of a piece of UNMAPPED"""
    tid = np.repeat(np.arange(p.nt, dtype=np.int64), np.diff(p.tstart))
    k = tid * 4 + ((p.src["flag"].astype(np.int64) >> 6) & 3)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    dup = np.nonzero(ks[1:] == ks[:-1])[0]
    if dup.shape[0]:
        r = int(order[dup[0] + 1])
        o = int(p.src["off"][r]) + 36
        raise ValueError("UNMAPPED holds read %r (flag %d) twice" % (
            p.buf[o:o + int(p.src["name_len"][r])].tobytes().decode(errors="replace"), int(p.src["flag"][r])))


class _Chunk:
    """ALIGNED's templates collected for one run: their record bytes, their list, and per record the
    partner's aux length and flag; the kept records' partners' aux bytes.  `bytes` = the record bytes
    plus the partners' aux bytes, which is bsdc_zip_bytes_bound of the chunk and what chunk_bytes
    budgets: UNMAPPED's consensus tags are the larger part of an output record."""

    def __init__(self):
        self.rec, self.src, self.pl, self.pflag, self.part = [], [], [], [], []
        self.rec_bytes = self.part_bytes = 0

    @property
    def bytes(self) -> int:
        return self.rec_bytes + self.part_bytes

    def add(self, a: Piece, r0: int, r1: int, pl, pflag, poff, ubuf):
        b0 = int(a.src["off"][r0])
        b1 = int(a.src["off"][r1 - 1]) + int(a.src["len"][r1 - 1])
        s = a.src[r0:r1].copy()
        s["off"] += self.rec_bytes - b0
        self.rec.append(a.buf[b0:b1].copy())
        self.src.append(s)
        self.pl.append(pl)
        self.pflag.append(pflag)
        self.part.append(ubuf[_ragged(poff, pl)])
        self.rec_bytes += b1 - b0
        self.part_bytes += int(pl.sum())

    def tables(self, hdr):
        """-> (the chunk's aligned Records, its zipper.Tables)"""
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)  # noqa: E731
        data = cat(self.rec, np.uint8)
        buf = np.zeros(max((data.shape[0] + 3) // 4 * 4, 4), np.uint8)
        buf[:data.shape[0]] = data
        a = Z.Records(hdr, buf, int(data.shape[0]), cat(self.src, _lib.ZIP_SRC))
        keep = np.nonzero((a.src["flag"] & 4) == 0)[0]
        t = Z.kept_tables(a, keep, cat(self.pl, np.int64)[keep], cat(self.pflag, np.uint16)[keep], cat(self.part, np.uint8))
        return a, t


class _Walk:
    """The lockstep join (rule 1 on two files in one template order) and the cut into chunks."""

    def __init__(self, a: Templates, u: Templates, chunk_bytes: int, flush):
        self.a, self.u, self.chunk_bytes, self.flush = a, u, chunk_bytes, flush
        self.up: Optional[Piece] = None
        self.lonely = 0
        self.chunk = _Chunk()

    def _next_u(self) -> bool:
        self.up = self.u.next()
        if self.up is not None:
            _check_twice(self.up)
        return self.up is not None

    def held(self, ap: Optional[Piece]) -> int:
        """the record bytes of the inputs in memory: both files' pieces and carries"""
        return (ap.n_bytes if ap is not None else 0) + self.a.held + (self.up.n_bytes if self.up is not None else 0) + self.u.held

    def run(self):
        while True:
            ap = self.a.next()
            if ap is None:
                break
            while ap.t < ap.nt:
                self._segment(ap)
        # UNMAPPED's templates behind the last aligned one
        while True:
            if self.up is not None:
                self.lonely += self.up.nt - self.up.t
            if not self._next_u():
                break

    def _segment(self, ap: Piece):
        """ALIGNED's next templates of this piece whose templates of UNMAPPED lie in one piece of it"""
        ta, tu = [], []
        while ap.t < ap.nt:
            if self.up is None or self.up.t >= self.up.nt:
                if ta:
                    break  # (join what this piece of UNMAPPED gave before it goes)
                if not self._next_u():
                    raise ValueError(
                        "aligned read %r was not found in UNMAPPED behind the read before it: --stream true needs ALIGNED to "
                        "keep UNMAPPED's template order, as bwa mem leaves it (the read may also be missing from UNMAPPED); "
                        "--stream false takes ALIGNED in any order" % ap.names[ap.t].decode(errors="replace"))
                continue
            up = self.up
            if up.names[up.t] == ap.names[ap.t]:
                ta.append(ap.t)
                tu.append(up.t)
                ap.t += 1
            else:
                self.lonely += 1
            up.t += 1
        up = self.up
        ta, tu = np.asarray(ta, np.int64), np.asarray(tu, np.int64)
        # rule 1 inside the template pairs: key = the pair's number * 4 + the end
        r0, r1 = int(ap.tstart[ta[0]]), int(ap.tstart[ta[-1] + 1])
        na = np.diff(ap.tstart)[ta]
        ka = np.repeat(np.arange(ta.shape[0], dtype=np.int64), na) * 4 + ((ap.src["flag"][r0:r1].astype(np.int64) >> 6) & 3)
        ur = _ragged(up.tstart[tu], np.diff(up.tstart)[tu])  # UNMAPPED's records of the pairs
        ku = np.repeat(np.arange(tu.shape[0], dtype=np.int64), np.diff(up.tstart)[tu]) * 4 + \
            ((up.src["flag"][ur].astype(np.int64) >> 6) & 3)
        order = np.argsort(ku, kind="stable")
        kus = ku[order]
        at = np.searchsorted(kus, ka)
        ok = at < kus.shape[0]
        ok[ok] = kus[at[ok]] == ka[ok]
        if not ok.all():
            k = r0 + int(np.nonzero(~ok)[0][0])
            o = int(ap.src["off"][k]) + 36
            raise ValueError("aligned read %r (flag %d) has no partner in UNMAPPED" % (
                ap.buf[o:o + int(ap.src["name_len"][k])].tobytes().decode(errors="replace"), int(ap.src["flag"][k])))
        p = up.src[ur[order[at]]]
        kept = (ap.src["flag"][r0:r1] & 4) == 0
        pl = np.where(kept, (p["len"] - p["aux"]).astype(np.int64), 0)
        poff = p["off"] + p["aux"]
        # the templates into chunks: a chunk that has reached the budget leaves when the next template comes
        tb = np.concatenate([[0], np.cumsum(na)])  # the pairs' first records, from r0
        w = np.add.reduceat(ap.src["len"][r0:r1].astype(np.int64) + pl, tb[:-1])
        t, nt = 0, int(ta.shape[0])
        while t < nt:
            if self.chunk.bytes >= self.chunk_bytes:
                self.flush(self.chunk, False, self.held(ap))
                self.chunk = _Chunk()
            j = int(np.searchsorted(np.cumsum(w[t:]) + self.chunk.bytes, self.chunk_bytes, "left"))
            take = min(j + 1, nt - t)
            a0, a1 = int(tb[t]), int(tb[t + take])
            self.chunk.add(ap, r0 + a0, r0 + a1, pl[a0:a1], p["flag"][a0:a1], poff[a0:a1], up.buf)
            t += take


class _Run:
    """A run file behind its window: buf[:n_bytes] holds whole records src (keys: their sort keys),
    the first `cur` of them emitted already."""

    def __init__(self, path: str, size: int):
        self.path, self.size, self.pos = path, size, 0
        self.buf, self.src, self.keys, self.cur = None, np.zeros(0, _lib.ZIP_SRC), np.zeros(0, np.uint64), 0

    @property
    def unread(self) -> bool:
        return self.pos < self.size

    @property
    def left(self) -> int:
        return int(self.src.shape[0]) - self.cur

    def window_bytes(self) -> int:
        return int(self.src["len"][self.cur:].sum()) if self.left else 0

    def fill(self, budget: int):
        """an empty window takes the next whole records within `budget` bytes, or the next record"""
        with open(self.path, "rb") as fh:
            fh.seek(self.pos)
            data = fh.read(max(budget, 36))
            if len(data) >= 4:
                need = 4 + struct.unpack_from("<i", data, 0)[0]
                if need > len(data):
                    data += fh.read(need - len(data))
        self.buf = Z._aligned_copy(data)
        self.src, used = Z.scan_prefix(self.buf, len(data))
        if used == 0:
            raise OSError("%s: a run file is cut inside a record" % self.path)
        self.pos += used
        self.keys = Z.sort_keys(self.src["ref_id"], self.src["pos"], self.src["flag"])
        self.cur = 0


def gather_host(order: np.ndarray, src_off: np.ndarray, src_len: np.ndarray, src: np.ndarray, cap: Optional[int] = None,
                fill: Optional[int] = None):
    """bsdc_zip_gather_host -> (off int64 [n + 1], the buffer uint8 [cap])"""
    lib = _lib.load()
    n = int(order.shape[0])
    pad = lambda x, dt: np.ascontiguousarray(x, dt) if n else np.zeros(1, dt)  # noqa: E731
    o, so, sl = pad(order, np.uint32), pad(src_off, np.int64), pad(src_len, np.int32)
    cap = int(sl[o].sum()) if cap is None and n else int(cap or 0)
    dst = np.empty(max((cap + 3) // 4 * 4, 4), np.uint8) if fill is None else np.full(max((cap + 3) // 4 * 4, 4), fill, np.uint8)
    off = np.zeros(n + 1, np.int64)
    rc = lib.bsdc_zip_gather_host(o.ctypes.data, n, so.ctypes.data, sl.ctypes.data, src.ctypes.data, int(src.shape[0]),
                                  off.ctypes.data, dst.ctypes.data, cap)
    if rc != 0:
        raise ValueError("bsdc_zip_gather_host failed (%d): %s" % (rc, lib.bsdc_zip_last_error().decode()))
    return off, dst


def round_device(dev, keys: np.ndarray, src_off: np.ndarray, src_len: np.ndarray, src: np.ndarray, max_ref: int, max_pos: int):
    """One merge round on the GPU: the keys sorted with their position as payload (bsdc_zip_sort), the
    records moved into that order (bsdc_zip_gather) -> (the records' device tensor, their bytes, an event)"""
    import torch
    lib = _lib.load()
    n = int(keys.shape[0])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(dev)  # noqa: E731
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev)
        d_keys, d_idx = up(keys), up(np.arange(n, dtype=np.uint32))
        so, sl = np.ascontiguousarray(src_off, np.int64), np.ascontiguousarray(src_len, np.int32)
        d_so, d_sl, d_src = up(so), up(sl), up(src)
        cap = int(sl.sum())
        dst = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        tmp = torch.empty(int(max(lib.bsdc_zip_sort_tmp_bytes(n), lib.bsdc_zip_gather_tmp_bytes(n))), dtype=torch.uint8, device=dev)
        rc = lib.bsdc_zip_sort(d_keys.data_ptr(), d_idx.data_ptr(), n, max_ref, max_pos, tmp.data_ptr(), C.c_void_p(st.cuda_stream))
        if rc == 0:
            order = d_idx.cpu().numpy().view(np.uint32)  # (synchronises: the launcher checks a host copy)
            rc = lib.bsdc_zip_gather(d_idx.data_ptr(), order.ctypes.data, n, d_so.data_ptr(), so.ctypes.data, d_sl.data_ptr(),
                                     sl.ctypes.data, d_src.data_ptr(), int(src.shape[0]), off.data_ptr(), dst.data_ptr(), cap,
                                     tmp.data_ptr(), C.c_void_p(st.cuda_stream))
        if rc != 0:
            st.synchronize()
            raise ValueError("cli zipper's merge kernels failed (%d): %s" % (rc, lib.bsdc_zip_last_error().decode()))
        ev = torch.cuda.Event()
        ev.record(st)
    return dst, cap, ev


def _merge(runs, chunk_bytes: int, emit, note) -> int:
    """Phase 2 -> the rounds.  emit(keys, src_off, src_len, src): one round's records, the runs'
    segments back to back in run order, to be written in stable key order; note(bytes): the record
    bytes held."""
    budget = max(chunk_bytes // len(runs), 1)
    rounds = 0
    while True:
        for r in runs:
            if r.left == 0 and r.unread:
                r.fill(budget)
        live = [s for s, r in enumerate(runs) if r.left]
        if not live:
            return rounds
        # the bound: the least (last key, run) of the runs that have records behind their window
        bound = min(((int(runs[s].keys[-1]), s) for s in live if runs[s].unread), default=None)
        held = sum(runs[s].window_bytes() for s in live)
        keys, lens, segs = [], [], []
        for s in live:
            r = runs[s]
            k = r.keys[r.cur:]
            m = k.shape[0] if bound is None else int(np.searchsorted(k, np.uint64(bound[0]), "right" if s <= bound[1] else "left"))
            if m == 0:
                continue
            b0 = int(r.src["off"][r.cur])
            b1 = int(r.src["off"][r.cur + m - 1]) + int(r.src["len"][r.cur + m - 1])
            keys.append(k[:m])
            lens.append(r.src["len"][r.cur:r.cur + m])
            segs.append(r.buf[b0:b1])
            r.cur += m
        keys, lens = np.concatenate(keys), np.concatenate(lens).astype(np.int32)
        data = np.concatenate(segs)
        src = np.zeros((data.shape[0] + 3) // 4 * 4, np.uint8)
        src[:data.shape[0]] = data
        del data, segs
        note(held + 2 * int(src.shape[0]))  # the windows as they were, the round's records gathered from them and sorted
        emit(keys, np.cumsum(lens, dtype=np.int64) - lens, lens, src)
        rounds += 1


def zipper_stream(aligned: str, unmapped: str, out: str, tags_to_reverse=(), tags_to_revcomp=(), tags_to_remove=(),
                  threads: int = 0, level: int = 6, device=0, info: Optional[str] = None, host: bool = False,
                  chunk_bytes: Optional[int] = None, tmp_dir: Optional[str] = None) -> dict:
    """zipper.zipper(stream=True): see the module docstring.  chunk_bytes: any positive number of
    bytes (default DEFAULT_CHUNK_BYTES); tmp_dir: where the runs' directory is made (default: OUT's)."""
    from . import bgzf
    chunk_bytes = DEFAULT_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be positive")
    tags = Z.tags_struct(Z.tag_list(tags_to_reverse, Z.CONSENSUS_REVERSE), Z.tag_list(tags_to_revcomp, Z.CONSENSUS_REVCOMP),
                         Z.tag_list(tags_to_remove, ()))
    nblk = min(max(chunk_bytes // 8 // BGZF_BLOCK, 1), 1024)  # a piece of either input: an eighth of the budget, 64 MiB at most
    dev = None
    if not host:
        import torch
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    st = {"runs": [], "spill": 0, "peak": 0, "out": 0, "raw": 0, "w": None, "dir": None}

    def note(n: int):
        st["peak"] = max(st["peak"], int(n))

    def writer():
        if st["w"] is None:
            st["w"] = bgzf.BamWriter(out, Z.header(ta.header, tu.header), level, None if host else bgzf.GpuBgzf(dev))
        return st["w"]

    def put(records, total: int, ev=None):
        """a host array's or a device tensor's first `total` bytes join OUT"""
        st["raw"] += total
        if host:
            writer().add_raw(records[:total].tobytes(), threads)
        elif total:
            writer().add_device([[(records, 0, total, ev)]], threads)

    def flush(chunk: _Chunk, last: bool, held: int):
        a, t = chunk.tables(ta.header)
        st["out"] += t.n
        if host:
            _, idx = Z.sort_host(t.keys, t.idx, t.max_ref, t.max_pos)
            off, buf = Z.format_host(idx, t.tab, a.buf, t.part, tags)
            total, ev = int(off[-1]), None
        else:
            buf, total, ev = Z.format_device(dev, t, a.buf, tags)
        note(held + a.n_bytes + int(t.part.shape[0]) + total)
        if last and not st["runs"]:
            put(buf, total, ev)
            return
        if st["dir"] is None:
            st["dir"] = tempfile.mkdtemp(prefix="bsdc_zipper_", dir=tmp_dir or os.path.dirname(os.path.abspath(out)))
        if len(st["runs"]) >= MAX_RUNS:
            raise ValueError("more than %d sorted runs of %d bytes: each needs a window of one record in memory at once; "
                             "raise --chunk-mb" % (MAX_RUNS, chunk_bytes))
        path = os.path.join(st["dir"], "run%06d" % len(st["runs"]))
        with open(path, "wb") as fh:
            (buf[:total] if host else buf[:total].cpu().numpy()).tofile(fh)
        st["runs"].append(_Run(path, total))
        st["spill"] += total

    def emit(keys, src_off, src_len, src):
        max_ref, max_pos = int(keys.max() >> np.uint64(32)), int(((keys & np.uint64(0xffffffff)) >> np.uint64(1)).max()) - 1
        if host:
            _, order = Z.sort_host(keys, np.arange(keys.shape[0], dtype=np.uint32), max_ref, max_pos)
            off, dst = gather_host(order, src_off, src_len, src)
            put(dst, int(off[-1]))
        else:
            put(*round_device(dev, keys, src_off, src_len, src, max_ref, max_pos))

    ta = tu = None
    rounds = 0
    try:
        ta, tu = Templates(aligned, threads, nblk), Templates(unmapped, threads, nblk)
        walk = _Walk(ta, tu, chunk_bytes, flush)
        walk.run()
        flush(walk.chunk, True, 0)
        walk.chunk = None
        if st["runs"]:
            rounds = _merge(st["runs"], chunk_bytes, emit, note)
        writer()
    finally:
        try:
            if st["w"] is not None:
                st["w"].close(threads)
        finally:
            for t in (ta, tu):
                if t is not None:
                    t.close()
            if st["dir"] is not None:
                shutil.rmtree(st["dir"], ignore_errors=True)
    res = {"records_in": ta.records, "unmapped_records_in": tu.records, "records_out": st["out"],
           "unmapped_dropped": ta.records - st["out"], "templates_without_aligned": walk.lonely, "raw_bytes": st["raw"],
           "compressed_bytes": os.path.getsize(out), "runs": max(len(st["runs"]), 1), "merge_rounds": rounds,
           "spill_bytes": st["spill"], "peak_record_bytes": st["peak"]}
    if info is not None:
        with open(info, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")
    return res

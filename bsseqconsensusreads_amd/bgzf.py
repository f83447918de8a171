"""The BGZF codecs on the GPU and the streaming writers over them.

GpuBgzf deflates whole BGZF blocks (libbsdc bsdc_bgzf_*, csrc/bsdc_bgzf.hip), GpuInflate inflates
the input BAM's (bsdc_bgzf_inflate, csrc/bsdc_inflate.hip); BamWriter and FastqWriter are the C
writers of libbsdc_io (bam._load binds them) over one BGZF sink per file, deflating on the host
or, given a GpuBgzf, through it.  Three paths lead to a compressed block: the host's deflate
inside the sink, the GPU's deflate of host bytes (submit) and the GPU's deflate of text that never
left the device (submit_device); the last two are one job path here (GpuBgzf._launch, finish)."""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import bam
from .bam import _P, _ptr

BLOCK_BYTES = 65280  # the payload of a full BGZF block, as htslib and libbsdc_io cut it
FRAMED_MAX = 65536  # the largest framed block (header, deflate stream, CRC32, ISIZE)


class _GpuBuffers:
    """What the two codecs share: libbsdc, one device, a HIP stream of their own (so that they
    overlap the consensus kernels) and named buffers that grow on demand."""

    def __init__(self, device):
        import torch

        from . import _lib
        self.torch = torch
        self.lib = _lib.load()
        self.dev = torch.device(device)
        self.stream = torch.cuda.Stream(self.dev)
        self.buf = {}

    def _buf(self, name, n, dtype=None, pinned=False):
        torch = self.torch
        t = self.buf.get(name)
        if t is None or t.numel() < n:
            n = max(int(n * 1.25), 1)
            t = (torch.empty(n, dtype=dtype or torch.uint8, pin_memory=True) if pinned else
                 torch.empty(n, dtype=dtype or torch.uint8, device=self.dev))
            self.buf[name] = t
        return t


@dataclass
class BgzfJob:
    """A job in flight: what GpuBgzf.finish needs to collect it (GpuBgzf.job) and what a writer
    needs to put its blocks into the sinks (_BgzfWriter.pending).  Of device text both are one
    record; of host bytes the writer makes its own, from what its sinks gave at the take."""
    nb: list  # whole blocks per sink, laid out back to back (file 2's after file 1's)
    crc: Optional[np.ndarray]  # the blocks' CRC32s once the job is finished: the array the sinks filled at
    #                            the take, or a view of the pinned copy of the device's
    raw: Optional[int]  # where every block's bytes lie on the host (the staging slot), or None: they lie
    #                     in `din`, and finish() puts here where it fetched those of handed-back blocks
    event: object = None  # GpuBgzf's: recorded behind the kernels and the copy back of the sizes

    @property
    def nblk(self) -> int:
        return sum(self.nb)


class GpuBgzf(_GpuBuffers):
    """BGZF compression of a writer's whole blocks on one GPU (libbsdc bsdc_bgzf_*,
    csrc/bsdc_bgzf.hip): the bytes reach HBM from a pinned staging slot (submit) or lie there
    already (submit_device), one workgroup deflates each block of BLOCK_BYTES, the blocks come back
    packed (finish); the writer's sinks frame and write them.  Its own HIP stream, so it overlaps
    the consensus kernels; submit* returns at once, so the writer encodes the next records while
    the GPU compresses these."""

    MAX_BLOCKS = 1024  # blocks per kernel launch (the scratch: bsdc_bgzf_scratch_bytes of these)

    def __init__(self, device):
        super().__init__(device)  # device din / out / sizes / crc, pinned sizes_h / crc_h / out_h / raw0|1
        self.scratch = self.torch.empty(int(self.lib.bsdc_bgzf_scratch_bytes(self.MAX_BLOCKS)),
                                        dtype=self.torch.uint8, device=self.dev)
        self.slot = 0
        self.job = None  # the submitted, unfinished BgzfJob
        self.blocks = 0
        self.bytes_in = 0
        self.bytes_out = 0
        self.rem = []  # submit_device: each file's bytes past its last whole block, on the device
        self.fallback_blocks = 0  # submit_device: blocks the kernel handed back (sizes 0), deflated by the host
        self.raw_fetched = []  # their ordinals (counted over this object's blocks)
        # test hook, never set outside the tests: f(first ordinal, nblk) -> the job's blocks whose
        # size submit_device zeroes after the deflate, so that they take the sink's host deflate
        self.force_host = None

    def staging(self, nbytes: int):
        """the next pinned staging slot (two alternate: one may still feed the last submit)."""
        self.slot ^= 1
        return self._buf("raw%d" % self.slot, nbytes, pinned=True)

    def _launch(self, din, nb, raw=None):
        """On the stream, behind the fill of din: the nb blocks deflated and packed, their sizes
        (and, for device text, raw None, their CRC32s) copied back, the event recorded -> the job
        in flight.  Synchronises nothing."""
        crc = None
        torch, st = self.torch, self.stream.cuda_stream
        nblk = sum(nb)
        if nblk:
            n = nblk * BLOCK_BYTES
            out = self._buf("out", nblk * FRAMED_MAX)
            sizes = self._buf("sizes", nblk, torch.int32)
            sizes_h = self._buf("sizes_h", nblk, torch.int32, pinned=True)
            back = None
            if raw is None:
                d_crc = self._buf("crc", nblk, torch.int32)
                crc_h = self._buf("crc_h", nblk, torch.int32, pinned=True)
                if self.lib.bsdc_bgzf_crc32(din.data_ptr(), 0, nblk, d_crc.data_ptr(), st) != 0:
                    raise RuntimeError("bsdc_bgzf_crc32 failed")
                if self.force_host is not None:
                    back = np.asarray(self.force_host(self.blocks, nblk), np.int64)
            for b0 in range(0, nblk, self.MAX_BLOCKS):
                k = min(self.MAX_BLOCKS, nblk - b0)
                if self.lib.bsdc_bgzf_deflate(din.data_ptr(), n, b0, k, self.scratch.data_ptr(), sizes.data_ptr(),
                                              st) != 0:
                    raise RuntimeError("bsdc_bgzf_deflate failed")
                if back is not None and ((back >= b0) & (back < b0 + k)).any():
                    sizes[torch.from_numpy(back[(back >= b0) & (back < b0 + k)]).to(self.dev)] = 0
                if self.lib.bsdc_bgzf_pack(self.scratch.data_ptr(), sizes.data_ptr(), b0, k, out.data_ptr(), st) != 0:
                    raise RuntimeError("bsdc_bgzf_pack failed")
            sizes_h[:nblk].copy_(sizes[:nblk], non_blocking=True)
            if raw is None:
                crc_h[:nblk].copy_(d_crc[:nblk], non_blocking=True)
                crc = crc_h[:nblk].numpy().view(np.uint32)
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self.job = BgzfJob(list(nb), crc, raw, ev)
        return self.job

    def submit(self, raw, nblk: int):
        """launch the compression of nblk blocks from the pinned slot `raw` (staging()); one job in
        flight: finish() the last one first."""
        if self.job is not None:
            raise RuntimeError("GpuBgzf.submit with a job in flight")
        n = nblk * BLOCK_BYTES
        with self.torch.cuda.stream(self.stream):
            din = self._buf("din", n)
            din[:n].copy_(raw[:n], non_blocking=True)
            self._launch(din, [nblk], raw.data_ptr())

    def _remainders(self, n_files: int):
        """the first n_files files' remainders, each an empty device tensor until text leaves one"""
        self.rem += [self.torch.empty(0, dtype=self.torch.uint8, device=self.dev)
                     for _ in range(len(self.rem), n_files)]
        return self.rem

    def submit_device(self, pieces):
        """launch the compression of text that lies in HBM (bsdc_fastq_format's): pieces[d] = the
        byte ranges file d gains, in order, each (uint8 device tensor, a, b, event or None: the
        range is ready once the event is).  Behind each file's remainder the ranges are copied
        device to device into `din` (file 2's whole blocks after file 1's, as the writers' takes
        lay them out), bsdc_bgzf_crc32 runs with the deflate over the whole blocks, and each
        file's new remainder (< BLOCK_BYTES) stays on the device.  -> the job (one in flight, as
        submit's): its nb, its crc and, once finished, its raw are what the writer puts."""
        torch = self.torch
        if self.job is not None:
            raise RuntimeError("GpuBgzf.submit_device with a job in flight")
        rem = self._remainders(len(pieces))
        segs = [[rem[d]] + [t[a:b] for t, a, b, _ in ps] for d, ps in enumerate(pieces)]
        nb = [sum(int(x.numel()) for x in sg) // BLOCK_BYTES for sg in segs]
        with torch.cuda.stream(self.stream):
            for ps in pieces:
                for t, _, _, ev in ps:
                    if ev is not None:
                        self.stream.wait_event(ev)
                    t.record_stream(self.stream)
            din = self._buf("din", max(sum(nb) * BLOCK_BYTES, 16))
            pos = 0
            for d, sg in enumerate(segs):
                whole = nb[d] * BLOCK_BYTES
                rest = torch.empty(sum(int(x.numel()) for x in sg) - whole, dtype=torch.uint8, device=self.dev)
                at = 0  # the file's bytes placed so far: the first `whole` into din, the others into rest
                for x in sg:
                    k = int(x.numel())
                    head = min(k, max(whole - at, 0))
                    if head:
                        din[pos + at:pos + at + head].copy_(x[:head], non_blocking=True)
                    if k > head:
                        r0 = at + head - whole
                        rest[r0:r0 + k - head].copy_(x[head:], non_blocking=True)
                    at += k
                rem[d] = rest
                pos += whole
            return self._launch(din, nb)

    def finish(self):
        """wait for the job in flight, of either kind -> (packed blocks: a pinned uint8 array valid
        until the next finish, sizes int32[nblk]).  Of device text the bytes of the blocks whose
        size is 0 are fetched, for the sink's host deflate, and the job's raw says where they are."""
        job, self.job = self.job, None
        job.event.synchronize()
        nblk = job.nblk
        if nblk == 0:
            return np.zeros(0, np.uint8), np.zeros(0, np.int32)
        sizes_h = self.buf["sizes_h"][:nblk].numpy().copy()
        total = int(np.maximum(sizes_h, 0).sum(dtype=np.int64))
        out_h = self._buf("out_h", max(total, 1), pinned=True)
        if total:
            with self.torch.cuda.stream(self.stream):
                out_h[:total].copy_(self.buf["out"][:total], non_blocking=True)
            self.stream.synchronize()
        zero = np.nonzero(sizes_h == 0)[0]
        if job.raw is None and zero.shape[0]:
            raw = self._buf("raw_back", nblk * BLOCK_BYTES, pinned=True)
            with self.torch.cuda.stream(self.stream):
                for a in (int(b) * BLOCK_BYTES for b in zero):
                    raw[a:a + BLOCK_BYTES].copy_(self.buf["din"][a:a + BLOCK_BYTES], non_blocking=True)
            self.stream.synchronize()
            job.raw = raw.data_ptr()
            self.fallback_blocks += int(zero.shape[0])
            self.raw_fetched.extend(int(self.blocks + b) for b in zero)
        self.blocks += nblk
        self.bytes_in += nblk * BLOCK_BYTES
        self.bytes_out += total
        return out_h.numpy(), sizes_h

    def push_remainder(self, d: int, data: np.ndarray):
        """host bytes that precede file d's next device text: they join its (empty) remainder."""
        if int(self._remainders(d + 1)[d].numel()):
            raise RuntimeError("GpuBgzf.push_remainder: file %d has a device remainder already" % d)
        with self.torch.cuda.stream(self.stream):
            self.rem[d] = self.torch.from_numpy(np.ascontiguousarray(data).copy()).to(self.dev)

    def take_remainders(self):
        """the files' remainders brought to the host (uint8 arrays), the device's emptied: what a
        flush or the close appends to the sinks (bsdc_bgzf_sink_append)."""
        if self.job is not None:
            raise RuntimeError("GpuBgzf.take_remainders with a job in flight")
        with self.torch.cuda.stream(self.stream):
            host = [r.to("cpu", non_blocking=False).numpy() for r in self.rem]
        self.rem = []
        return host

    def counters(self) -> dict:
        return {"blocks": self.blocks, "text_bytes": self.bytes_in, "compressed_bytes": self.bytes_out,
                "fallback_blocks": self.fallback_blocks}

    def compress(self, data_ptr: int, nbytes: int):
        """host bytes [data_ptr, +nbytes) (whole blocks) -> (packed blocks, sizes int32[nblk])."""
        host = np.ctypeslib.as_array(C.cast(data_ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))
        raw = self.staging(nbytes)
        raw.numpy()[:nbytes] = host
        self.submit(raw, nbytes // BLOCK_BYTES)
        packed, sizes = self.finish()
        return packed[:int(np.maximum(sizes, 0).sum())].copy(), sizes


class GpuInflate(_GpuBuffers):
    """Inflate of the input BAM's BGZF blocks on one GPU (libbsdc bsdc_bgzf_inflate,
    csrc/bsdc_inflate.hip), as the streaming reader's inflater (stream_chunks(inflater=...),
    bsdc_bam_stream_set_inflater): per fill one call -- the compressed bytes and the block table go
    to HBM through pinned staging, one workgroup inflates each block, the bytes and the blocks'
    status come back, the stream is synchronised.  Non-zero when any block's status is (the reader
    then fails with its corrupt-BGZF error); the reader checks every block's CRC32 itself.  Its own
    HIP stream, so a fill overlaps the consensus kernels.  Counters: fills, blocks, bytes_in
    (compressed), bytes_out, seconds (inside the calls)."""

    def __init__(self, device):
        super().__init__(device)  # buffers: device comp / out / blk / status, pinned comp_h / out_h / blk_h / status_h
        self.fills = self.blocks = self.bytes_in = self.bytes_out = 0
        self.seconds = 0.0
        self.error = None  # the exception of a failed call (the reader reports a corrupt block)
        self.callback = bam.INFLATE_FN(self._call)

    def inflate(self, comp: np.ndarray, blk: np.ndarray, n_out: int):
        """comp: uint8 host bytes; blk: the block table as a uint8 view of nblk x 24 bytes
        (bsdc_inflate_block) -> (out: a pinned uint8 view of n_out bytes, valid until the next call,
        status int32[nblk])."""
        torch = self.torch
        nblk, n_comp = blk.shape[0] // 24, comp.shape[0]
        d_comp, h_comp = self._buf("comp", n_comp), self._buf("comp_h", n_comp, pinned=True)
        d_blk, h_blk = self._buf("blk", nblk * 24), self._buf("blk_h", nblk * 24, pinned=True)
        d_out, h_out = self._buf("out", n_out), self._buf("out_h", n_out, pinned=True)
        d_st = self._buf("status", nblk, torch.int32)
        h_st = self._buf("status_h", nblk, torch.int32, pinned=True)
        h_comp.numpy()[:n_comp] = comp
        h_blk.numpy()[:nblk * 24] = blk
        with torch.cuda.stream(self.stream):
            d_comp[:n_comp].copy_(h_comp[:n_comp], non_blocking=True)
            d_blk[:nblk * 24].copy_(h_blk[:nblk * 24], non_blocking=True)
            if self.lib.bsdc_bgzf_inflate(d_comp.data_ptr(), n_comp, d_blk.data_ptr(), nblk, d_out.data_ptr(), n_out,
                                          d_st.data_ptr(), self.stream.cuda_stream) != 0:
                raise RuntimeError("bsdc_bgzf_inflate failed")
            h_st[:nblk].copy_(d_st[:nblk], non_blocking=True)
            h_out[:n_out].copy_(d_out[:n_out], non_blocking=True)
        self.stream.synchronize()
        return h_out.numpy()[:n_out], h_st.numpy()[:nblk]

    def _call(self, user, comp, n_comp, blk, nblk, out, n_out) -> int:
        t0 = time.perf_counter()
        try:
            as_u8 = lambda p, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(int(n),))  # noqa: E731
            got, status = self.inflate(as_u8(comp, n_comp), as_u8(blk, 24 * nblk), int(n_out))
            bad = bool(status.any())
            if not bad:
                as_u8(out, n_out)[:] = got
            self.fills += 1
            self.blocks += int(nblk)
            self.bytes_in += int(n_comp)
            self.bytes_out += int(n_out)
            return 1 if bad else 0
        except BaseException as e:  # noqa: BLE001 -- nothing may unwind through the C caller
            self.error = e
            return -1
        finally:
            self.seconds += time.perf_counter() - t0

    def counters(self) -> dict:
        return {"fills": self.fills, "blocks": self.blocks, "bytes_in": self.bytes_in, "bytes_out": self.bytes_out,
                "seconds": round(self.seconds, 4)}


class _BgzfWriter:
    """What the streaming writers share: a C writer (bsdc_<kind>_writer) over one BGZF sink per
    file (bsdc_bgzf_sink).  On the host path an add deflates the whole blocks it fills.  With `gpu`
    (a GpuBgzf) an add only encodes; the whole blocks of every sink are taken back to back into one
    pinned staging slot and deflated on the GPU in one job (valid BGZF, other compressed bytes),
    which is written when the next add, a flush or the close drains it: one add's blocks compress
    while the next add encodes."""

    def __init__(self, kind: str, path: str, gpu: Optional["GpuBgzf"], *open_args):
        self.lib = bam._load()
        self.kind = kind
        self.path = path
        self.gpu = gpu
        self.pending = None  # the BgzfJob submitted to the GPU, not yet written
        self.sinks = []
        self.device_text = False  # add_device since the remainders were last brought back: they may hold bytes
        self.h = _P()
        if self._call("open", *open_args, C.byref(self.h)) != 0:
            raise self._err()

    def _call(self, what: str, *args):
        return getattr(self.lib, "bsdc_%s_writer_%s" % (self.kind, what))(*args)

    def _err(self):
        return OSError("%s: %s" % (self.path, self.lib.bsdc_io_last_error().decode()))

    def _drain(self, threads: int):
        job, self.pending = self.pending, None
        if job is None:
            return
        packed, sizes = self.gpu.finish()
        b = off = 0  # the blocks / packed bytes of the sinks before this one
        for sink, n in zip(self.sinks, job.nb):
            if n == 0:
                continue
            sz = np.ascontiguousarray(sizes[b:b + n])
            if self.lib.bsdc_bgzf_sink_put(sink, n, packed.ctypes.data + off, _ptr(sz), job.crc.ctypes.data + 4 * b,
                                           None if job.raw is None else job.raw + b * BLOCK_BYTES,
                                           int(threads)) != 0:
                raise self._err()
            off += int(np.maximum(sz, 0).sum(dtype=np.int64))
            b += n

    def add_device(self, pieces, threads: int = 0):
        """Bytes that bsdc_fastq_format / bsdc_bam_format left in HBM join the files: pieces[d] =
        file d's byte ranges (GpuBgzf.submit_device).  The protocol of add on the GPU path without
        encode and take: the job before is written, this one submitted; its whole blocks come back
        compressed with their CRC32s, the remainders stay on the device until a flush, the close or
        a host add."""
        if self.gpu is None:
            raise ValueError("%s.add_device needs a GpuBgzf" % type(self).__name__)
        self._drain(threads)
        # host bytes added before (the BAM header at the open, add, add_raw) left their remainder in
        # the sinks' tails: it goes in front of these bytes, as the device remainder (which add has
        # emptied), so the bytes stay in order
        for d, sink in enumerate(self.sinks):
            # (a BAM header of many @SQ lines may hold whole blocks: they join the job too)
            tail = np.empty(int(self.lib.bsdc_bgzf_sink_whole(sink)) + FRAMED_MAX, np.uint8)
            n = int(self.lib.bsdc_bgzf_sink_take_tail(sink, _ptr(tail), tail.shape[0]))
            if n < 0:
                raise self._err()
            if n:
                self.gpu.push_remainder(d, tail[:n])
        self.device_text = True
        self.pending = self.gpu.submit_device(pieces)

    def _remainders(self, threads: int):
        """the device remainders (< BLOCK_BYTES each) brought to the sinks' tails"""
        if not self.device_text:
            return
        self._drain(threads)
        for sink, r in zip(self.sinks, self.gpu.take_remainders()):
            if r.shape[0] and self.lib.bsdc_bgzf_sink_append(sink, _ptr(r), int(r.shape[0])) != 0:
                raise self._err()
        self.device_text = False

    def add(self, recs: bam.OutRecordsBam, threads: int = 0):
        self._remainders(threads)  # (host bytes after device bytes: in order)
        keep = []
        r = bam._records_struct(recs, keep)
        if self._call("add" if self.gpu is None else "encode", self.h, C.byref(r), int(threads)) != 0:
            raise self._err()
        if self.gpu is None:
            return
        nb = [int(self.lib.bsdc_bgzf_sink_whole(sink)) // BLOCK_BYTES for sink in self.sinks]
        if sum(nb):
            raw = self.gpu.staging(sum(nb) * BLOCK_BYTES)
            crc = np.empty(sum(nb), np.uint32)
            b = 0
            for sink, n in zip(self.sinks, nb):  # (file 2's blocks follow file 1's)
                if n and self.lib.bsdc_bgzf_sink_take(sink, n, raw.data_ptr() + b * BLOCK_BYTES,
                                                      crc.ctypes.data + 4 * b, int(threads)) != 0:
                    raise self._err()
                b += n
        self._drain(threads)
        if sum(nb):
            self.gpu.submit(raw, sum(nb))
            self.pending = BgzfJob(nb, crc, raw.data_ptr())

    def _flush(self, threads: int) -> tuple:
        self._remainders(threads)
        self._drain(threads)
        if self._call("flush", self.h, int(threads)) != 0:
            raise self._err()
        return tuple(int(self.lib.bsdc_bgzf_sink_tell(sink)) for sink in self.sinks)

    def close(self, threads: int = 0):
        if self.h:
            try:
                self._remainders(threads)
                self._drain(threads)
            finally:
                h, self.h = self.h, _P()
                self.sinks = []
                if self._call("close", h, int(threads)) != 0:
                    raise self._err()


class BamWriter(_BgzfWriter):
    """Streaming BAM writer (bsdc_bam_writer): header at open, records added in order, the same
    bytes as bam.write_bam of all the records at once -- or, with `gpu`, every whole block deflated
    on the GPU; add_device then takes records that bsdc_bam_format wrote in HBM (one file: pieces =
    [its byte ranges]), the file a writer fed the same records by add on the GPU path writes."""

    def __init__(self, path: str, header: bam.BamHeader, level: int = 6, gpu: Optional["GpuBgzf"] = None,
                 fragment: Optional[str] = None):
        """fragment: "first" (header, no EOF block) or "next" (neither) -- one rank's piece of a
        BAM that ranks.assemble concatenates."""
        keep = []
        super().__init__("bam", path, gpu, path.encode(), *bam._header_args(header, keep), int(level))
        self.sinks = [self.lib.bsdc_bam_writer_sink(self.h)]
        if fragment is not None and self.lib.bsdc_bam_writer_fragment(self.h, int(fragment == "first")) != 0:
            raise self._err()

    def flush(self, threads: int = 0) -> int:
        """Everything added so far written as whole BGZF blocks; -> the file's length, a point
        where it may be cut (ranks.py splices other pieces in there)."""
        return self._flush(threads)[0]

    def add_raw(self, data: bytes, threads: int = 0):
        """Raw BAM records (block_size-prefixed), as a stream chunk holds them (host deflate)."""
        if data:
            self._remainders(threads)  # (host bytes after device records: in order)
            buf = np.frombuffer(data, np.uint8)
            if self.lib.bsdc_bam_writer_raw(self.h, _ptr(buf), buf.shape[0], int(threads)) != 0:
                raise self._err()


def close_quietly(*writers):
    """Best-effort close of writers a failed step leaves open (BamWriter / FastqWriter / None):
    finishes their in-flight GPU BGZF job and releases the C writer's FILE and buffers, swallowing
    secondary errors (the step raises its first error anyway; the partial output is garbage)."""
    for w in writers:
        if w is None:
            continue
        try:
            w.close()
        except Exception:  # noqa: BLE001
            pass


class FastqWriter(_BgzfWriter):
    """Streaming paired-FASTQ writer (bsdc_fastq_writer): the bytes bam.write_fastq writes for all
    the records at once; every add holds whole pairs.  With `gpu`, the whole blocks of both files
    are deflated on the GPU in one job (BGZF-framed gzip)."""

    def __init__(self, path1: str, path2: str, level: int = 6, gpu: Optional["GpuBgzf"] = None,
                 fragment: bool = False):
        super().__init__("fastq", path1, gpu, path1.encode(), path2.encode(), int(level))
        self.sinks = [self.lib.bsdc_fastq_writer_sink(self.h, d) for d in range(2)]
        if fragment and self.lib.bsdc_fastq_writer_fragment(self.h) != 0:  # (no EOF blocks: ranks.assemble)
            raise self._err()

    def flush(self, threads: int = 0) -> Tuple[int, int]:
        """Everything added so far written as whole BGZF blocks; -> (length of file 1, of file 2)."""
        return self._flush(threads)

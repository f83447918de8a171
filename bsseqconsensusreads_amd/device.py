"""Device side of the step: family batches in HBM (torch tensors as plumbing), libbsdc launches.

The Engine owns one libbsdc context per GPU.  ``upload`` copies a FamilyBatch into HBM once;
``run`` enqueues the kernels on the current torch stream (so torch events time exactly them) and
``fetch`` brings the consensus (and the optional stage dump) back to the host.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass, replace
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .batch import FamilyBatch, wide_rows
from .filter import FilterParams
from .records import Reference


@dataclass
class ConsensusParams:
    """fgbio CallDuplexConsensusReads options, defaults from main.snake.py:163.
    min_consensus_base_quality: single-strand calls below it become (N, 2).  The duplex caller
    passes no such flag; fgbio's single-strand caller inside it masks below PhredScore.MinValue = 2
    (DESIGN.md 3.5).  Step 1 passes --min-consensus-base-quality=0 (main.snake.py:54):
    MOLECULAR_PARAMS."""

    error_rate_pre_umi: float = 45.0
    error_rate_post_umi: float = 30.0
    min_input_base_quality: int = 0
    consensus_call_overlapping_bases: bool = True
    min_reads: int = 0
    min_consensus_base_quality: int = 2

    def c_struct(self):
        return _lib.Params(self.error_rate_pre_umi, self.error_rate_post_umi, self.min_input_base_quality,
                           int(self.consensus_call_overlapping_bases), self.min_reads,
                           self.min_consensus_base_quality)


# fgbio CallMolecularConsensusReads as rule call_consensus_reads_molecular runs it (main.snake.py:54):
# --error-rate-pre-umi=45 --error-rate-post-umi=30 --min-input-base-quality=0
# --min-consensus-base-quality=0 --consensus-call-overlapping-bases=true (--min-reads=1: a column
# without an A/C/G/T read is a no-call, as in the duplex caller's single-strand caller)
MOLECULAR_PARAMS = ConsensusParams(min_consensus_base_quality=0)


def _dptr(t: torch.Tensor) -> int:
    return int(t.data_ptr())


@dataclass
class FastqText:
    """What Engine.fastq leaves on a DeviceBatch: the FASTQ text of its kept families in HBM
    (bsdc_fastq_format).  text[d]: file d's bytes (uint8, `cap[d]` of them allocated); off: int64
    [2, F + 1] on the device, the families' byte offsets per file, off[d, F] = the text's size;
    event: recorded after the launch; name_off: the host copy of the names' offsets (what
    bam.fastq_offsets takes).  Dropping the object releases the text."""

    text: tuple
    off: torch.Tensor
    cap: tuple
    event: "torch.cuda.Event"
    name_off: np.ndarray
    total: Optional[tuple] = None  # (file 1's bytes, file 2's), once fetched


@dataclass
class BamText:
    """What Engine.bam_records leaves on a DeviceBatch: the BAM records of its kept families in HBM
    (bsdc_bam_format).  rec: the bytes (uint8, `cap` of them allocated); off: int64 [F + 1] on the
    device, the families' byte offsets, off[F] = the records' size; event: recorded after the
    launch.  Dropping the object releases the records."""

    rec: torch.Tensor
    off: torch.Tensor
    cap: int
    event: "torch.cuda.Event"


@dataclass
class ToolrecText:
    """What Engine.toolrec leaves on a DeviceBatch: the BAM records of the batch's records after tool
    1 and tool 2 in HBM (bsdc_toolrec_format).  rec: the bytes (uint8, `cap` of them allocated); off:
    int64 [n_rec + 1] on the device, the records' byte offsets, off[n_rec] = their size; foff: int64
    [F + 1] on the device, off at each family's first record (and the size); event: recorded after
    the launch.  Dropping the object releases the records."""

    rec: torch.Tensor
    off: torch.Tensor
    foff: torch.Tensor
    cap: int
    event: "torch.cuda.Event"


class DeviceBatch:
    """A FamilyBatch resident in HBM plus its output buffers."""

    def __init__(self, fb: FamilyBatch, device: torch.device, dump: bool = False, tags: bool = False,
                 filt: bool = False):
        self.fb = fb
        self.n_fam, self.n_rec = fb.n_fam, fb.n_rec
        self.device = device
        self.t: Dict[str, torch.Tensor] = {}
        for k, v in fb.device_arrays().items():
            a = np.ascontiguousarray(v)
            if a.size == 0:
                a = np.zeros(1, dtype=a.dtype)
            # torch has no uint32/uint16 arithmetic we need; move raw bytes.  Pinned sources (the
            # engine's staging images) copy asynchronously on the stream; the engine double-buffers
            # them, and the batch before is fetched (stream synchronized) before a buffer is refilled
            h = torch.from_numpy(a.view(np.uint8))
            self.t[k] = h.to(device, non_blocking=h.is_pinned())
        F, Rn = fb.n_fam, fb.n_rec
        self.stride = fb.stride
        self.gather_host = None
        if fb.gather is not None:  # the images are made here in HBM (Engine.image), every byte of them
            self.t["seq"] = torch.empty(fb.n_slots // 2 + 64, dtype=torch.uint8, device=device)
            self.t["qual"] = torch.empty(fb.n_slots + 64, dtype=torch.uint8, device=device)
            self.gather_host = np.ascontiguousarray(fb.gather)  # (the launcher checks this copy)
            self.t["gather"] = torch.from_numpy(self.gather_host.view(np.uint8) if fb.n_rec else
                                                np.zeros(8, np.uint8)).to(device, non_blocking=True)
        self.n_slots = fb.n_slots
        self.status = torch.zeros(max(F, 1), dtype=torch.uint8, device=device)
        self.len = torch.zeros(max(2 * F, 1), dtype=torch.int16, device=device)
        self.seq = torch.zeros(max(F * self.stride, 16), dtype=torch.uint8, device=device)
        self.qual = torch.zeros(max(2 * F * self.stride, 16), dtype=torch.uint8, device=device)
        self.dump = dump
        if dump:
            cap = fb.n_slots + 16
            self.dump_pos = torch.zeros(max(Rn, 1), dtype=torch.int32, device=device)
            self.dump_len = torch.zeros(max(Rn, 1), dtype=torch.int16, device=device)
            self.dump_tags = torch.zeros(max(Rn, 1), dtype=torch.uint8, device=device)
            self.dump_seq = torch.zeros(cap, dtype=torch.uint8, device=device)
            self.dump_qual = torch.zeros(cap, dtype=torch.uint8, device=device)
        self.tags = tags
        if tags:  # single-strand reads + column statistics (BSDC_MODE_TAGS), rows (family, set)
            nss = max(4 * F * self.stride, 16)
            self.ss_len = torch.zeros(max(4 * F, 1), dtype=torch.int16, device=device)
            self.ss_base = torch.zeros(nss, dtype=torch.uint8, device=device)
            self.ss_qual = torch.zeros(nss, dtype=torch.uint8, device=device)
            self.ss_depth = torch.zeros(nss, dtype=torch.uint8, device=device)
            self.ss_err = torch.zeros(nss, dtype=torch.uint8, device=device)
            # families whose depths may pass a byte get exact u16 rows too (include/bsdc.h ss_wide)
            self.ss_wide, self.n_wide = wide_rows(fb.fam_off)
            if self.n_wide:
                nw = 4 * self.n_wide * self.stride
                self.t["ss_wide"] = torch.from_numpy(self.ss_wide.view(np.uint8)).to(device)
                self.ss_wdepth = torch.zeros(nw, dtype=torch.int16, device=device)
                self.ss_werr = torch.zeros(nw, dtype=torch.int16, device=device)
        self.fastq: Optional[FastqText] = None  # Engine.fastq
        self.bamrec: Optional[BamText] = None  # Engine.bam_records
        self.toolrec: Optional[ToolrecText] = None  # Engine.toolrec
        self.filt = self.masked = None
        if filt:  # bsdc_filter's outputs: reason bits per family, newly masked columns per end
            self.filt = torch.zeros(max(F, 1), dtype=torch.uint8, device=device)
            self.masked = torch.zeros(max(2 * F, 1), dtype=torch.int16, device=device)
        # HBM scratch: arenas of the large buckets beyond the LDS budget, one region per bucket (the
        # bucket dispatches run concurrently on the library's side streams), the split families'
        # fallback arenas and their parts' sums (FamilyBatch.scratch_layout; + slack: dword reads
        # may run a few bytes past the last arena, their bytes masked).  Every byte a kernel reads
        # there it wrote first: no zero fill
        need, _, poff = fb.scratch_layout()
        self.scratch = torch.empty(need, dtype=torch.uint8, device=device) if need else None
        self._b = _lib.FamilyBatchC()
        b = self._b
        b.n_rec, b.n_fam = Rn, F
        for k in ("fam_off", "rec", "rec_win", "cig_off", "cig_info", "cigar", "rt", "seq", "qual",
                  "small_fams", "large_fams", "split_parts", "split_part_recs", "split_fams"):
            setattr(b, k, _dptr(self.t[k]))
        b.n_split_parts, b.n_split_fams = int(fb.split_parts.shape[0]), int(fb.split_fams.shape[0])
        b.split_part_arena, b.split_partial_off = int(fb.split_part_arena), int(poff)
        for q in range(_lib.SMALL_BUCKETS):
            b.n_small[q] = int(fb.small_buckets[q].shape[0])
            b.small_arena[q] = int(fb.small_arenas[q])
        for q in range(_lib.LARGE_BUCKETS):
            b.n_large[q] = int(fb.large_buckets[q].shape[0])
            b.large_arena[q] = int(fb.large_arenas[q])
        b.max_len = fb.max_len
        self._o = _lib.ConsensusC()
        o = self._o
        o.stride = self.stride
        o.status, o.len, o.seq, o.qual = _dptr(self.status), _dptr(self.len), _dptr(self.seq), _dptr(self.qual)
        if dump:
            o.dump_pos, o.dump_len, o.dump_tags = _dptr(self.dump_pos), _dptr(self.dump_len), _dptr(self.dump_tags)
            o.dump_seq, o.dump_qual = _dptr(self.dump_seq), _dptr(self.dump_qual)
        o.scratch = _dptr(self.scratch) if self.scratch is not None else None
        if tags:
            o.ss_len, o.ss_base, o.ss_qual = _dptr(self.ss_len), _dptr(self.ss_base), _dptr(self.ss_qual)
            o.ss_depth, o.ss_err = _dptr(self.ss_depth), _dptr(self.ss_err)
            if self.n_wide:
                o.ss_wide = _dptr(self.t["ss_wide"])
                o.ss_wdepth, o.ss_werr = _dptr(self.ss_wdepth), _dptr(self.ss_werr)

    def release_host(self):
        """Drop the host copy of the batch (the device copy stays resident)."""
        self.fb = None

    def fetch_lengths(self):
        """-> (status [F], len [F, 2]): the small outputs only (bench bookkeeping)."""
        F = self.n_fam
        return (self.status[:F].cpu().numpy(),
                self.len[:2 * F].cpu().numpy().view(np.uint16).astype(np.int32).reshape(F, 2))

    def fetch(self, alloc=None, ss: bool = True, seqqual: bool = True, dump: bool = True):
        """dump=False leaves the stage dump of a dump batch in HBM (Engine.toolrec read it there).
        -> dict of numpy arrays (consensus and, if dumped, the post-tool records; after
        Engine.filter also "filt" [F] and "masked" [F, 2]).  ss=False leaves the single-strand rows
        of a tags batch in HBM (a filtered output without consensus tags, or one whose records
        Engine.bam_records wrote there).  seqqual=False (after Engine.fastq or Engine.bam_records,
        when no output is formatted on the host): "status", "len", ("filt", "masked"), "fastq_total"
        (the two texts' sizes, checked against the buffers) and "bam_off" only -- the bases and
        qualities stay in HBM, where the outputs were made of them; `ss` does not apply and `alloc`
        is refused.  After Engine.bam_records every form brings "bam_off" (int64 [F + 1], 8 bytes a
        family: where each family's records start, the last one their size).  The copies
        are queued together on the current stream into pinned host memory (torch's caching host
        allocator), then one synchronize.  With alloc(nbytes) -> uint8 array (a fleet worker's
        shared segment) the outputs land in that buffer instead, so they leave the worker by name."""
        F = self.n_fam
        if not seqqual:
            if alloc is not None:
                raise ValueError("fetch(seqqual=False) copies into pinned memory only: no alloc")
            return self._fetch_small()
        t = {"status": self.status[:F], "len": self.len[:2 * F], "seq": self.seq[:F * self.stride],
             "qual": self.qual[:2 * F * self.stride]}
        n = 4 * F * self.stride
        ss = ss and self.tags
        if self.filt is not None:
            t.update(filt=self.filt[:F], masked=self.masked[:2 * F])
        if self.bamrec is not None:
            t.update(bam_off=self.bamrec.off)
        if ss:
            t.update(ss_len=self.ss_len[:4 * F], ss_base=self.ss_base[:n], ss_qual=self.ss_qual[:n],
                     ss_depth=self.ss_depth[:n], ss_err=self.ss_err[:n])
            if self.n_wide:
                t.update(ss_wdepth=self.ss_wdepth, ss_werr=self.ss_werr)
        Rn = self.n_rec
        dump = dump and self.dump
        if dump:
            t.update(dump_pos=self.dump_pos[:Rn], dump_len=self.dump_len[:Rn], dump_tags=self.dump_tags[:Rn],
                     dump_seq=self.dump_seq, dump_qual=self.dump_qual)
        if alloc is None:
            h = {k: v.to("cpu", non_blocking=True) for k, v in t.items()}
            torch.cuda.current_stream(self.device).synchronize()
            a = {k: v.numpy() for k, v in h.items()}
        else:
            sizes = {k: (v.numel() * v.element_size() + 255) // 256 * 256 for k, v in t.items()}
            buf = alloc(max(1, sum(sizes.values())))
            a, o = {}, 0
            for k, v in t.items():
                nb = v.numel() * v.element_size()
                dst = torch.from_numpy(buf[o:o + nb]).view(v.dtype)
                dst.copy_(v)
                a[k] = dst.numpy()
                o += sizes[k]
            torch.cuda.current_stream(self.device).synchronize()
        out = {
            "status": a["status"],
            "len": a["len"].view(np.uint16).astype(np.int32).reshape(F, 2),
            "seq": a["seq"].reshape(F, 2, self.stride // 2),
            "qual": a["qual"].reshape(F, 2, self.stride),
            "stride": self.stride,
        }
        if self.filt is not None:
            out["filt"] = a["filt"]
            out["masked"] = a["masked"].view(np.uint16).astype(np.int32).reshape(F, 2)
        if self.bamrec is not None:
            out["bam_off"] = a["bam_off"].view(np.int64)
        if ss:
            out["ss_len"] = a["ss_len"].view(np.uint16).astype(np.int32).reshape(F, 4)
            out["ss_base"] = a["ss_base"].reshape(F, 4, self.stride)
            out["ss_qual"] = a["ss_qual"].reshape(F, 4, self.stride)
            out["ss_depth"] = a["ss_depth"].reshape(F, 4, self.stride)
            out["ss_err"] = a["ss_err"].reshape(F, 4, self.stride)
            out["ss_wide"] = self.ss_wide
            W = self.n_wide
            out["ss_wdepth"] = a["ss_wdepth"].view(np.uint16).reshape(W, 4, self.stride) if W else \
                np.zeros((0, 4, self.stride), np.uint16)
            out["ss_werr"] = a["ss_werr"].view(np.uint16).reshape(W, 4, self.stride) if W else \
                np.zeros((0, 4, self.stride), np.uint16)
        if dump:
            out["dump_pos"] = a["dump_pos"]
            out["dump_len"] = a["dump_len"].view(np.uint16).astype(np.int32)
            out["dump_tags"] = a["dump_tags"]
            out["dump_seq"] = a["dump_seq"]
            out["dump_qual"] = a["dump_qual"]
        return out

    def _fetch_small(self):
        F = self.n_fam
        if self.fastq is None and self.bamrec is None:
            raise ValueError("fetch(seqqual=False) needs Engine.fastq or Engine.bam_records on the batch first")
        t = {"status": self.status[:F], "len": self.len[:2 * F]}
        if self.fastq is not None:
            t.update(fastq_total=self.fastq.off[:, F].contiguous())
        if self.bamrec is not None:
            t.update(bam_off=self.bamrec.off)
        if self.filt is not None:
            t.update(filt=self.filt[:F], masked=self.masked[:2 * F])
        h = {k: v.to("cpu", non_blocking=True) for k, v in t.items()}
        torch.cuda.current_stream(self.device).synchronize()
        out = {"status": h["status"].numpy(), "len": h["len"].numpy().view(np.uint16).astype(np.int32).reshape(F, 2),
               "stride": self.stride}
        if self.filt is not None:
            out["filt"] = h["filt"].numpy()
            out["masked"] = h["masked"].numpy().view(np.uint16).astype(np.int32).reshape(F, 2)
        if self.bamrec is not None:
            out["bam_off"] = h["bam_off"].numpy()
        if self.fastq is not None:
            self.fastq.total = out["fastq_total"] = tuple(int(x) for x in h["fastq_total"].numpy())
            for d in range(2):
                assert 0 <= self.fastq.total[d] <= self.fastq.cap[d], (self.fastq.total, self.fastq.cap)
        return out


class PinnedPool:
    """A pinned host arena for the family images of one chunk's batches (materialize's `images`,
    bump-allocated): the streaming step materializes a whole chunk ahead of the GPU stage into
    one pool, the batches upload asynchronously from it, and the pool is reset for a later chunk
    once every upload from it is done (bam.step5_stream keeps three in rotation)."""

    SEGMENT = 64 << 20

    def __init__(self):
        self.segs = []  # pinned uint8 tensors; the last one is being filled
        self.used = 0  # bytes of the last segment handed out
        self.total = 0  # bytes handed out since the reset

    def images(self, n_slots: int):
        nq = n_slots
        ns = n_slots // 2 + 64
        need = (ns + 255) // 256 * 256 + nq
        if not self.segs or self.used + need > self.segs[-1].numel():
            self.segs.append(torch.empty(max(need, self.SEGMENT), dtype=torch.uint8, pin_memory=True))
            self.used = 0
        seg = self.segs[-1]
        a = self.used
        b = a + (ns + 255) // 256 * 256
        self.used = (b + nq + 255) // 256 * 256
        self.total += need
        return seg[a:a + ns].numpy(), seg[b:b + nq].numpy()

    def reset(self):
        """every batch materialized from the pool has been uploaded: hand its bytes out again
        (a pool that spilled over several segments becomes one that holds the largest chunk)."""
        if len(self.segs) > 1:
            size = int(max(self.total, sum(t.numel() for t in self.segs)) * 1.25)
            self.segs = [torch.empty(size, dtype=torch.uint8, pin_memory=True)]
        self.used = 0
        self.total = 0


class Engine:
    """One libbsdc context on one GPU."""

    def __init__(self, device_index: int = 0, params: Optional[ConsensusParams] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU: the bsdc product path runs on MI355X only (no CPU fallback)")
        self.lib = _lib.load()
        self.device_index = device_index
        self.device = torch.device("cuda", device_index)
        self.params = params or ConsensusParams()
        self._stage = [None, None]  # pinned family-image staging buffers (stage_images)
        self._stage_i = 0
        p = self.params.c_struct()
        h = C.c_void_p()
        rc = self.lib.bsdc_ctx_create(device_index, C.byref(p), C.byref(h))
        if rc != 0:
            raise RuntimeError("bsdc_ctx_create failed (%d)" % rc)
        self.ctx = h
        self.ref: Optional[Reference] = None
        self._metrics = None  # (accumulator in HBM, cycles): metrics_begin

    def set_params(self, params: ConsensusParams):
        """Replace the context's flags (bsdc_ctx_set_params); later launches use them."""
        p = params.c_struct()
        self._check(self.lib.bsdc_ctx_set_params(self.ctx, C.byref(p)), "bsdc_ctx_set_params")
        self.params = params

    @contextlib.contextmanager
    def flags(self, **changes):
        """`with engine.flags(min_consensus_base_quality=0): ...` -- the engine runs with these
        flags inside the block and its own afterwards (one context serving step 1 and step 5)."""
        old = self.params
        if all(getattr(old, k) == v for k, v in changes.items()):
            yield self
            return
        self.set_params(replace(old, **changes))
        try:
            yield self
        finally:
            self.set_params(old)

    def stage_images(self, n_slots: int):
        """Pinned host arrays (seq, qual) for the next batch's family images (materialize's
        `images`), alternating between two buffer pairs that grow on demand: a batch's images
        upload asynchronously while the next one is filled (pipeline.run_ranges)."""
        i = self._stage_i
        self._stage_i ^= 1
        st = self._stage[i]
        if st is None or st[1].numel() < n_slots:
            cap = int(n_slots * 1.25) + 4096
            st = (torch.empty(cap // 2 + 64, dtype=torch.uint8, pin_memory=True),
                  torch.empty(cap, dtype=torch.uint8, pin_memory=True))
            self._stage[i] = st
        return st[0].numpy(), st[1].numpy()

    def close(self):
        if self.ctx:
            self.lib.bsdc_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.lib.bsdc_last_error(self.ctx).decode()))

    def load_reference(self, ref: Reference):
        packed = np.ascontiguousarray(ref.packed)
        off = np.ascontiguousarray(ref.contig_off, dtype=np.int64)
        ln = np.ascontiguousarray(ref.contig_len, dtype=np.int64)
        rc = self.lib.bsdc_load_reference(self.ctx, packed.ctypes.data, ref.n_nibbles, off.ctypes.data,
                                          ln.ctypes.data, len(ref.names))
        self._check(rc, "bsdc_load_reference")
        self.ref = ref

    def upload(self, fb: FamilyBatch, dump: bool = False, tags: bool = False, filt: bool = False,
               raw_dev: Optional[torch.Tensor] = None) -> DeviceBatch:
        """filt: also the outputs of `filter` (which reads the tags' rows: tags is then on).  A batch
        without host images (fb.gather) needs raw_dev, its records' SEQ / QUAL bytes in HBM
        (upload_raw), and gets its images made there (image) on the current stream."""
        with torch.cuda.device(self.device):
            db = DeviceBatch(fb, self.device, dump, tags or filt, filt)
            if fb.gather is not None:
                if raw_dev is None:
                    raise ValueError("a batch without host images (FamilyBatch.gather) needs raw_dev (upload_raw)")
                self.image(db, raw_dev)
            return db

    def upload_raw(self, raw_bases: np.ndarray) -> torch.Tensor:
        """A chunk's records' SEQ / QUAL bytes (RawRecords.raw_bases) into HBM on the current stream,
        asynchronously from pinned memory: what `image` reads for each of the chunk's batches.  The
        tensor is allocated and used on one stream; dropping it after the last batch's launch frees
        it in stream order (torch's caching allocator)."""
        a = np.ascontiguousarray(raw_bases, np.uint8)
        h = torch.from_numpy(a if a.shape[0] else np.zeros(4, np.uint8))
        with torch.cuda.device(self.device):
            return h.to(self.device, non_blocking=h.is_pinned())

    def image(self, db: DeviceBatch, raw_dev: torch.Tensor, stream: Optional[torch.cuda.Stream] = None):
        """The batch's family images made in HBM from the records' bytes (bsdc_image_gather), enqueued
        on the stream the vote runs on, before it."""
        if db.gather_host is None:
            raise ValueError("the batch has host images (no FamilyBatch.gather)")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self.lib.bsdc_image_gather(self.ctx, C.c_void_p(_dptr(raw_dev)), int(raw_dev.numel()),
                                        C.c_void_p(_dptr(db.t["gather"])), C.c_void_p(db.gather_host.ctypes.data),
                                        db.n_rec, db.n_slots, C.c_void_p(_dptr(db.t["seq"])),
                                        C.c_void_p(_dptr(db.t["qual"])), C.c_void_p(s.cuda_stream))
        self._check(rc, "bsdc_image_gather")

    def run(self, db: DeviceBatch, mode: int, stream: Optional[torch.cuda.Stream] = None):
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self.lib.bsdc_run(self.ctx, C.byref(db._b), C.byref(db._o), mode, C.c_void_p(s.cuda_stream))
        self._check(rc, "bsdc_run")

    def filter(self, db: DeviceBatch, fparams: FilterParams, molecular: bool = False,
               stream: Optional[torch.cuda.Stream] = None):
        """fgbio FilterConsensusReads over a batch run with MODE_TAGS (bsdc_filter),
        enqueued on the stream that ran it: db.seq / db.qual are masked in place, db.filt and
        db.masked filled (fetch returns them).  molecular: step-1 records (one strand per end)."""
        if db.filt is None:
            raise ValueError("the batch was uploaded without filt=True")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        p = fparams.c_struct()
        rc = self.lib.bsdc_filter(self.ctx, C.byref(p), 1 if molecular else 0, db.n_fam, C.byref(db._o),
                                  C.c_void_p(_dptr(db.filt)), C.c_void_p(_dptr(db.masked)), C.c_void_p(s.cuda_stream))
        self._check(rc, "bsdc_filter")

    def metrics_begin(self, cycles: int = 512):
        """The run's metrics accumulator (bsdc_metrics_words(cycles) u64 words in HBM),
        allocated and zeroed once; `metrics` and `metrics_filter` add every batch into it."""
        n = int(self.lib.bsdc_metrics_words(int(cycles)))
        if n < 0:
            raise ValueError("metrics: cycles outside 2..1024 (%r)" % (cycles,))
        with torch.cuda.device(self.device):
            self._metrics = (torch.zeros(n, dtype=torch.int64, device=self.device), int(cycles))

    def _metrics_acc(self):
        if self._metrics is None:
            raise ValueError("no metrics accumulator: call Engine.metrics_begin first")
        return self._metrics

    def metrics(self, db: DeviceBatch, molecular: bool = False, stream: Optional[torch.cuda.Stream] = None):
        """A voted batch (run with MODE_TAGS) reduced into the accumulator (bsdc_metrics), enqueued on
        the stream that ran the vote, after it and before `filter` masks the consensus."""
        acc, cycles = self._metrics_acc()
        if not db.tags:
            raise ValueError("metrics: the batch was uploaded without tags=True")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self.lib.bsdc_metrics(self.ctx, C.byref(db._o), db.n_fam, db.n_wide, 1 if molecular else 0, cycles,
                                   C.c_void_p(_dptr(acc)), C.c_void_p(s.cuda_stream))
        self._check(rc, "bsdc_metrics")

    def metrics_filter(self, db: DeviceBatch, stream: Optional[torch.cuda.Stream] = None):
        """The filter's outcome of a batch (db.filt, db.masked) added to the accumulator
        (bsdc_metrics_filter), enqueued after `filter` on its stream."""
        acc, _ = self._metrics_acc()
        if db.filt is None:
            raise ValueError("metrics_filter: the batch was uploaded without filt=True")
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self.lib.bsdc_metrics_filter(self.ctx, C.c_void_p(_dptr(db.status)), C.c_void_p(_dptr(db.filt)),
                                          C.c_void_p(_dptr(db.masked)), db.n_fam, C.c_void_p(_dptr(acc)),
                                          C.c_void_p(s.cuda_stream))
        self._check(rc, "bsdc_metrics_filter")

    def metrics_fetch(self) -> np.ndarray:
        """-> the accumulator as uint64 words (one copy, after a synchronize of the current stream:
        at the end of the run).  The accumulator stays, so a later batch keeps adding."""
        acc, _ = self._metrics_acc()
        torch.cuda.current_stream(self.device).synchronize()
        return acc.cpu().numpy().view(np.uint64).copy()

    def fastq(self, db: DeviceBatch, names, stream: Optional[torch.cuda.Stream] = None) -> FastqText:
        """The FASTQ text of the batch's kept families formatted where the consensus lies
        (bsdc_fastq_format), enqueued on the stream that ran the vote, after it and after `filter`.
        names: the families' read names, one each, as a packed table (.buf, .off: bam.family_names).
        The table goes up, two text buffers of the size known beforehand (bsdc_fastq_text_bound)
        are allocated, and db.fastq holds them with an event recorded behind the launch."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        F = db.n_fam
        off_h = np.ascontiguousarray(names.off, np.int64)
        if off_h.shape[0] != F + 1:
            raise ValueError("one name per family: %d offsets for %d families" % (off_h.shape[0], F))
        off_h = off_h - off_h[0]
        nb = int(off_h[-1])
        buf_h = np.ascontiguousarray(names.buf[int(names.off[0]):int(names.off[0]) + nb], np.uint8)
        cap = int(self.lib.bsdc_fastq_text_bound(F, nb, db.stride))
        with torch.cuda.device(self.device), torch.cuda.stream(s):
            d_off = torch.from_numpy(off_h).to(self.device)
            d_buf = torch.from_numpy(buf_h if nb else np.zeros(1, np.uint8)).to(self.device)
            text = tuple(torch.empty(max(cap, 16), dtype=torch.uint8, device=self.device) for _ in range(2))
            off = torch.empty((2, F + 1), dtype=torch.int64, device=self.device)
            tmp = torch.empty(int(self.lib.bsdc_fastq_tmp_bytes(F)), dtype=torch.uint8, device=self.device)
            rc = self.lib.bsdc_fastq_format(C.byref(db._o), C.c_void_p(_dptr(db.filt)) if db.filt is not None else None,
                                            F, C.c_void_p(_dptr(d_off)), C.c_void_p(_dptr(d_buf)),
                                            C.c_void_p(off_h.ctypes.data), C.c_void_p(_dptr(off[0])),
                                            C.c_void_p(_dptr(off[1])), C.c_void_p(_dptr(text[0])),
                                            C.c_void_p(_dptr(text[1])), cap, cap, C.c_void_p(_dptr(tmp)),
                                            C.c_void_p(s.cuda_stream))
            if rc != 0:
                raise RuntimeError("bsdc_fastq_format failed (%d)" % rc)
            ev = torch.cuda.Event()
            ev.record(s)
        db.fastq = FastqText(text, off, (cap, cap), ev, off_h)
        return db.fastq

    def bam_records(self, db: DeviceBatch, names, aux, molecular: bool = False, tags: bool = True,
                    stream: Optional[torch.cuda.Stream] = None) -> BamText:
        """The output BAM's records of the batch's kept families written where the consensus lies
        (bsdc_bam_format), enqueued on the stream that ran the vote, after it and after `filter`.
        names, aux: the families' read names and aux bytes (RG / MI / RX), one each, as packed tables
        (.buf, .off: bam.family_names, bam.family_aux).  tags: fgbio's consensus tags follow, from
        the single-strand rows (the batch was uploaded with tags=True).  The tables go up, a buffer of
        the size known beforehand (bsdc_bam_bytes_bound) is allocated, and db.bamrec holds it with an
        event recorded behind the launch."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        F = db.n_fam
        if tags and not db.tags:
            raise ValueError("bam_records(tags=True): the batch was uploaded without tags=True")
        host = []
        for t in (names, aux):
            off_h = np.ascontiguousarray(t.off, np.int64)
            if off_h.shape[0] != F + 1:
                raise ValueError("one entry per family: %d offsets for %d families" % (off_h.shape[0], F))
            off_h = off_h - off_h[0]
            nb = int(off_h[-1])
            buf_h = np.ascontiguousarray(t.buf[int(t.off[0]):int(t.off[0]) + nb], np.uint8)
            host.append((off_h, buf_h if nb else np.zeros(1, np.uint8), nb))
        cap = int(self.lib.bsdc_bam_bytes_bound(F, host[0][2], host[1][2], db.stride, 1 if molecular else 0,
                                                1 if tags else 0))
        with torch.cuda.device(self.device), torch.cuda.stream(s):
            dev = [(torch.from_numpy(o).to(self.device), torch.from_numpy(b).to(self.device)) for o, b, _ in host]
            rec = torch.empty(max(cap, 16), dtype=torch.uint8, device=self.device)
            off = torch.empty(F + 1, dtype=torch.int64, device=self.device)
            tmp = torch.empty(int(self.lib.bsdc_bam_tmp_bytes(F)), dtype=torch.uint8, device=self.device)
            p = lambda t: C.c_void_p(_dptr(t))  # noqa: E731
            rc = self.lib.bsdc_bam_format(C.byref(db._o), p(db.filt) if db.filt is not None else None,
                                          1 if molecular else 0, 1 if tags else 0, F,
                                          p(dev[0][0]), p(dev[0][1]), C.c_void_p(host[0][0].ctypes.data),
                                          p(dev[1][0]), p(dev[1][1]), C.c_void_p(host[1][0].ctypes.data),
                                          p(off), p(rec), cap, p(tmp), C.c_void_p(s.cuda_stream))
            if rc != 0:
                raise RuntimeError("bsdc_bam_format failed (%d)" % rc)
            ev = torch.cuda.Event()
            ev.record(s)
        db.bamrec = BamText(rec, off, cap, ev)
        return db.bamrec

    def toolrec(self, db: DeviceBatch, tables, stream: Optional[torch.cuda.Stream] = None) -> ToolrecText:
        """The batch's records after tool 1 and tool 2 written as BAM records where the stage dump
        lies (bsdc_toolrec_format), enqueued on the stream that ran bsdc_run(.. | MODE_DUMP), after
        it.  tables: toolrec.Tables of the batch's records (toolrec.batch_tables).  The tables go up,
        a buffer of the size known beforehand (bsdc_toolrec_bytes_bound) is allocated, and db.toolrec
        holds it with an event recorded behind the launch."""
        if not db.dump:
            raise ValueError("toolrec: the batch was uploaded without dump=True")
        if tables.n != db.n_rec:
            raise ValueError("toolrec: %d table entries for %d records" % (tables.n, db.n_rec))
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        n = db.n_rec
        n_dump = int(db.dump_seq.numel()) // 4 * 4
        if n_dump < db.n_slots:  # (every record's slot lies inside the batch's n_slots)
            raise ValueError("toolrec: the dump buffers hold %d bytes, the batch's slots %d" % (n_dump, db.n_slots))
        cap = tables.bound(n_dump)
        tab_h = np.ascontiguousarray(tables.tab) if n else np.zeros(1, _lib.TOOLREC_REC)
        fam_first = np.ascontiguousarray(db.fb.fam_off if db.fb is not None else [0, n], np.int64)
        with torch.cuda.device(self.device), torch.cuda.stream(s):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(self.device)  # noqa: E731
            d_tab, d_names, d_cig, d_aux = up(tab_h), up(tables.names), up(tables.cigar), up(tables.aux)
            rec = torch.empty(max(cap, 16), dtype=torch.uint8, device=self.device)
            off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
            tmp = torch.empty(int(self.lib.bsdc_toolrec_tmp_bytes(n)), dtype=torch.uint8, device=self.device)
            p = lambda t: C.c_void_p(_dptr(t))  # noqa: E731
            rc = self.lib.bsdc_toolrec_format(C.byref(db._o), p(db.t["rec"]), n, n_dump, p(d_tab),
                                              C.c_void_p(tab_h.ctypes.data), p(d_names), int(tables.names.shape[0]),
                                              p(d_cig), int(tables.cigar.shape[0]), p(d_aux), int(tables.aux.shape[0]),
                                              p(off), p(rec), cap, p(tmp), C.c_void_p(s.cuda_stream))
            if rc != 0:
                raise RuntimeError("bsdc_toolrec_format failed (%d): %s" % (
                    rc, self.lib.bsdc_toolrec_last_error().decode()))
            foff = off[torch.from_numpy(fam_first).to(self.device)]
            ev = torch.cuda.Event()
            ev.record(s)
        db.toolrec = ToolrecText(rec, off, foff, cap, ev)
        return db.toolrec

    def tables(self):
        lr = np.zeros(256, np.int64)
        thr = np.zeros(94, np.float32)
        self._check(self.lib.bsdc_get_tables(self.ctx, lr.ctypes.data, thr.ctypes.data), "bsdc_get_tables")
        return lr, thr

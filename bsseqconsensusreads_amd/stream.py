"""The streaming step: a coordinate-sorted BAM through the consensus in bounded memory, pipelined.

One front end (FrontEnd: decoder -> reader -> planner threads), the GPU stage on the caller's
thread, one back end (BackEnd: builder -> writer threads); a Chunk travels between them, each stage
working on the chunk after the next stage's.  Peak host memory is about six chunks, whatever the
file size.  The output is byte-identical to bam.step5's (tests/test_stream.py): every chunk's
TemplateCoordinate keys sort before the next chunk's, so the chunks' families in order are the
whole file's.  run() is the one-GPU stream (bam.step5_stream, bam.molecular_stream, a rank of
ranks.step5_ranks); fleet.step5_stream_multi puts its dealer and collector between the same ends.
"""
from __future__ import annotations

import contextlib
import dataclasses
import functools
import os
import queue
import threading
import time
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from . import bam, bgzf, pipeline
from . import filter as _filter
from . import records as R

MINKEY = -(1 << 62)  # sort key of the pieces before every family (the header, a first range's start)
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@dataclasses.dataclass
class StreamJob:
    """What run() is to do, as plain values (a rank's job crosses a process boundary).
    molecular: None = step 5, else step 1 with this --min-consensus-base-quality.  gpu_bgzf: the
    BAM's and the FASTQ pair's blocks are deflated on the engine's GPU (bgzf.GpuBgzf; the same
    records, other compressed bytes, files ≈4% larger).  filter (filter.FilterParams): every batch
    is filtered on the device after its vote (step5's `filter`); an Engine stream only.  defer:
    the span past which a template is deferred (step 5; default bam.DEFAULT_DEFER_SPAN, 0 = off;
    see run).
    rank-parallel use (ranks.py): rng = the record range of the input to run and owner = the rank's
    key interval (bam.stream_chunks); fragment = "first" / "next" (the output pieces a rank writes:
    BamWriter, FastqWriter); spill = the file the deferred records go to; late_splices = the
    deferred keys the spill's pass cuts at; first_key = the sort key of the rank's first piece;
    regions (the ranks' passes) = also cut before the first family of every new key contig pair (a
    piece keyed (pair, MINKEY)): a rank does not register cross keys (bsdc_io.cpp), so the deferred
    families of a contig's cross keys go between those pieces.
    gpu_inflate: the input BAM's BGZF blocks are inflated on the engine's GPU (bgzf.GpuInflate; the
    same bytes, so the same output files); an Engine stream only.
    gpu_fastq: the FASTQ pair's text is formatted, checksummed and deflated on the engine's GPU
    (Engine.fastq, bgzf.GpuBgzf.submit_device): the files of a gpu_bgzf run, byte for byte; needs
    `fastq`, an Engine stream only.
    gpu_bam: the output BAM's records are written in HBM from the consensus (Engine.bam_records),
    checksummed and deflated there (bgzf.BamWriter.add_device): the file of a gpu_bgzf run, byte
    for byte; needs `out_bam`, an Engine stream only; implies the GPU deflate for the BAM.
    gpu_image: the chunks are decoded without unpacked bases (bam.StreamChunk.decode(packed=True)),
    their SEQ / QUAL bytes go up once a chunk and every batch's family images are made in HBM from
    them (Engine.image, bsdc_image_gather) instead of on the host: the same images, so the same
    output files; an Engine stream only.  A split_ext chunk unpacks its bases on the host.
    metrics: the path of the run's metrics JSON (metrics.write): every batch, the
    whole-chunk batches of a split_ext plan and the deferred templates' pass included, is reduced into
    one accumulator on the engine's GPU (Engine.metrics; metrics_cycles rows of by_cycle) and the
    file is written once at the end; the output files are those of the run without it.  An Engine
    stream of one process only: not in a rank's stream, not with a runner.
    groupsort_bam: the path of a BAM of the records after tool 1 and tool 2 in TemplateCoordinate
    order (rule groupsort_convert's file): every batch runs with BSDC_MODE_DUMP and
    its records are written in HBM (Engine.toolrec), checksummed and deflated there through a second
    BamWriter (add_device); a split_ext chunk's come from the host twin.  The file is cut at the
    deferred keys as the other outputs are.  Step 5, an Engine stream of one process only; the other
    output files are those of the run without it."""

    in_bam: str
    fasta: Optional[str]
    out_bam: Optional[str]
    fastq: Optional[Tuple[str, str]] = None
    prefix: Optional[str] = None
    threads: int = 0
    level: int = 6
    tags: bool = True
    gpu_bgzf: bool = False
    chunk_bytes: int = bam.DEFAULT_CHUNK_BYTES
    slack: int = bam.DEFAULT_SLACK
    batch_bases: Optional[int] = None
    read_size: int = 8 << 20
    molecular: Optional[int] = None
    filter: Optional[_filter.FilterParams] = None
    defer: Optional[int] = None
    rng: Optional[tuple] = None
    owner: Optional[tuple] = None
    fragment: Optional[str] = None
    spill: Optional[str] = None
    late_splices: Optional[np.ndarray] = None
    first_key: Optional[tuple] = None
    regions: bool = False
    metrics: Optional[str] = None
    metrics_cycles: int = 512
    groupsort_bam: Optional[str] = None
    gpu_fastq: bool = False
    gpu_bam: bool = False
    gpu_image: bool = False
    gpu_inflate: bool = False  # (stays the last field)


@dataclasses.dataclass
class Chunk:
    """What travels between the stages: a chunk's records, then its family plan and batches (None:
    a split_ext plan, run as a whole chunk), the deferred keys its output is cut before, the pooled
    buffer its record arrays are carved from (given back once its output is written), and -- the
    fleet -- the workers' result segments to release then."""

    raw: R.RawRecords
    plan: object = None
    batches: Optional[list] = None
    splices: Optional[np.ndarray] = None
    pool_buf: Optional[np.ndarray] = None
    results: Sequence = ()
    pin_buf: object = None  # (gpu_image) the pinned tensor raw.raw_bases lies in (PinnedRaw)


class Fault:
    """The stages' first-error list and their `stop` event: a failing stage reports here, every
    stage stops working at its next chunk and drains to its upstream's None, so no stage blocks."""

    def __init__(self, on_fail: Optional[Callable[[], None]] = None):
        self.stop, self.errors, self.on_fail = threading.Event(), [], on_fail

    def __call__(self, e: BaseException):
        self.errors.append(e)
        self.stop.set()
        if self.on_fail is not None:
            self.on_fail()


def plan_step5(raw, ref):
    return raw, pipeline.plan_families(raw, "full", ref)


def plan_molecular(raw):
    """Step 1: the chunk's MI runs are the families, the vote alone."""
    raw = pipeline.molecular_records(raw)
    return raw, pipeline.plan_families(raw, "vote", family_order="mi-group")


class PinnedRaw:
    """Pinned host buffers for the chunks' SEQ / QUAL bytes (RawRecords.raw_bases, gpu_image): the
    reader take()s one per chunk, the upload from it runs asynchronously, and it is give()n back
    once the chunk's output is written (its batches were fetched, so the copy is done)."""

    def __init__(self):
        self.free, self.lock = [], threading.Lock()

    def take(self, nbytes: int):
        import torch
        with self.lock:
            fit = [i for i, t in enumerate(self.free) if t.numel() >= nbytes]
            if fit:
                return self.free.pop(min(fit, key=lambda i: self.free[i].numel()))
        return torch.empty(max(int(nbytes * 1.15), 1), dtype=torch.uint8, pin_memory=True)

    def give(self, t):
        if t is not None:
            with self.lock:
                self.free.append(t)


class PinnedBatches:
    """A chunk's batches materialized into pinned memory: chunk k's into pool k % 3 -- chunk k - 3
    is done on the GPU by then (the planner handed chunk k - 1 over only after the GPU stage took
    chunk k - 2).  A loading engine's first chunks (ranks._LazyEngine) materialize into plain host
    arrays, the pools come with it."""

    def __init__(self, engine, gather: bool = False):
        self.engine, self.k, self.gather = engine, 0, gather  # gather: no host images (gpu_image)
        self.pools = [] if getattr(engine, "lazy", False) else self._new()

    def _new(self):
        from .device import PinnedPool
        return [PinnedPool() for _ in range(3)]

    def __call__(self, plan, ranges):
        if self.gather:
            return pipeline.materialize_ranges(plan, ranges, gather=True)
        if not self.pools and self.engine.ready():
            self.pools = self._new()
        images = None
        if self.pools:
            pool = self.pools[self.k % 3]
            self.k += 1
            pool.reset()
            images = pool.images
        return pipeline.materialize_ranges(plan, ranges, images)


class _Stages:
    """Stage threads (self.workers), started on entering the `with` block."""

    def __enter__(self):
        for t in self.workers:
            t.start()
        return self


class FrontEnd(_Stages):
    """decoder -> reader -> planner, each a thread, depth-1 queues between them; the caller's
    thread iterates over the planned Chunks (`with FrontEnd(...) as front: for ch in front`).
    Leaving the block early -- an exception, or fault.stop -- drains and joins the threads.
    source: bam.stream_chunks' arguments (its `stats` dict receives the range statistics); plan:
    records -> (records, FamilyPlan); build: (plan, family ranges) -> the chunk's batches (a
    split_ext plan gets none); spill: the file the chunks' spill entries are written to
    (deferral), counted in spilled_bytes, the deferred keys past the last chunk in splices_tail.
    T: seconds inside the decoder (decode), the reader's wait for it (reader_wait), parsing
    (parse), plan, materialize, and the caller's wait for a chunk (wait); R: bam.StreamChunk.decode's."""

    def __init__(self, fault: Fault, source: dict, plan, build, threads: int, batch_bases: Optional[int],
                 bufs: "bam.BufferPool", spill: Optional[str] = None, pinned: Optional[PinnedRaw] = None):
        self.pinned = pinned  # (gpu_image) decode without unpacked bases, raw_bases into its buffers
        self.fault, self.source, self.plan, self.build = fault, dict(source), plan, build
        self.source.setdefault("stats", {})
        self.threads, self.batch_bases, self.bufs, self.spill = threads, batch_bases, bufs, spill
        self.spilled_bytes, self.splices_tail = 0, np.zeros((0, 2), np.int64)
        self.T = {"decode": 0.0, "reader_wait": 0.0, "parse": 0.0, "plan": 0.0, "materialize": 0.0, "wait": 0.0}
        self.R: dict = {}
        self.raws, self.parsed, self.chunks = (queue.Queue(maxsize=1) for _ in range(3))
        self.drained = False
        self.workers = [threading.Thread(target=f, name="stream" + f.__name__, daemon=True)
                        for f in (self._decoder, self._reader, self._planner)]

    def _decoder(self):  # cuts the next chunk (inflate, split, family-complete selection) while the
        # reader thread parses the one before
        it = sw = None
        stop, rs = self.fault.stop, self.source["stats"]
        try:
            if self.spill is not None:
                sw = open(self.spill, "wb")
            it = bam.stream_chunks(**self.source)
            while not stop.is_set():
                t0 = time.perf_counter()
                nxt = next(it, None)
                self.T["decode"] += time.perf_counter() - t0
                if nxt is None:
                    break
                if sw is not None and nxt.spill:
                    sw.write(nxt.spill)
                    self.spilled_bytes += len(nxt.spill)
                self.raws.put(nxt)
            if sw is not None and not stop.is_set():
                tail = rs.pop("spill_tail", b"")
                sw.write(tail)
                self.spilled_bytes += len(tail)
                self.splices_tail = rs.pop("splices_tail", self.splices_tail)
        except BaseException as e:  # noqa: BLE001 -- handed to the caller
            self.fault(e)
        finally:
            if sw is not None:
                sw.close()
            if it is not None:
                it.close()  # (the stream is freed once every chunk is back)
            self.raws.put(None)

    def _reader(self):  # parses a chunk's records while the planner forms the families of the one before
        try:
            while True:
                t0 = time.perf_counter()
                ch = self.raws.get()
                if ch is None:
                    break
                if self.fault.stop.is_set():
                    ch.discard()
                    continue  # drain to the decoder's None without parsing
                t1 = time.perf_counter()
                pin_t = []
                if self.pinned is not None:
                    def pin(nbytes):
                        pin_t.append(self.pinned.take(nbytes))
                        return pin_t[0].numpy()
                    raw = ch.decode(self.threads, self.R, self.bufs, packed=True, pin=pin)[1]
                else:
                    raw = ch.decode(self.threads, self.R, self.bufs)[1]
                self.T["parse"] += time.perf_counter() - t1
                self.T["reader_wait"] += t1 - t0
                self.parsed.put(Chunk(raw, splices=ch.splices, pool_buf=ch.pool_buf,
                                      pin_buf=pin_t[0] if pin_t else None))
        except BaseException as e:  # noqa: BLE001
            self.fault(e)
            for ch in iter(self.raws.get, None):  # let the decoder finish
                ch.discard()
        finally:
            self.parsed.put(None)

    def _planner(self):  # forms a chunk's families and materializes its batches ahead of the GPU stage
        try:
            while True:
                ch = self.parsed.get()
                if ch is None:
                    break
                if self.fault.stop.is_set():
                    continue  # drain to the reader's None without planning
                t0 = time.perf_counter()
                ch.raw, ch.plan = self.plan(ch.raw)
                t1 = time.perf_counter()
                if not ch.plan.split_ext:
                    ch.batches = self.build(ch.plan, pipeline.plan_ranges(ch.plan, self.batch_bases))
                self.T["plan"] += t1 - t0
                self.T["materialize"] += time.perf_counter() - t1
                self.chunks.put(ch)
        except BaseException as e:  # noqa: BLE001
            self.fault(e)
            while self.parsed.get() is not None:  # let the reader finish
                pass
        finally:
            self.chunks.put(None)

    def __iter__(self):
        while True:
            t0 = time.perf_counter()
            ch = self.chunks.get()
            self.T["wait"] += time.perf_counter() - t0
            if ch is None:
                self.drained = True
                return
            if self.fault.stop.is_set():  # a stage failed: stop working, __exit__ drains
                return
            yield ch

    def __exit__(self, *exc):
        if not self.drained:  # let the planner finish (it stops planning once `stop` is set)
            self.fault.stop.set()
            while self.chunks.get() is not None:
                pass
        for t in self.workers:
            t.join()


class BackEnd(_Stages):
    """builder -> writer: put(cons, chunk, cuts) hands a chunk's consensus over; a builder thread
    makes its output records (bam.duplex_records) while a writer thread encodes the chunk before
    (bgzf.BamWriter / FastqWriter; gz_device: a call that gives the device whose GPU deflates,
    bgzf.GpuBgzf).  cuts: (record index, key) -- everything before the index leaves as whole blocks
    and a piece with that key starts there, noted in `marks` ((BAM offset, FASTQ offsets x 2), sort
    key (key, tie)); the first mark is the header's, keyed first_key.  Once a chunk is written its
    pooled buffers go back to `bufs` and on_written(chunk) is called.  Leaving the `with` block
    ends the threads; a failing writer closes its files quietly (bgzf.close_quietly).
    fq_device (a call that gives the device): the FASTQ pair takes a chunk's text from HBM where
    its Consensus carries it (Consensus.fastq, pipeline.FastqPiece): the cuts become byte ranges of
    that text (FastqWriter.add_device), no records are built without a BAM, and the text is
    released once the chunk is written.  A chunk without device text (a split_ext plan) goes the
    host way through the same writer.  fastq_counters: the pair's GpuBgzf counters at the close.
    bam_device (a call that gives the device): likewise the BAM takes a chunk's records from HBM
    where its Consensus carries them (Consensus.bamrec, pipeline.BamPiece; BamWriter.add_device):
    no tagged records are built for such a chunk (untagged ones only when the FASTQ pair is
    formatted on the host); bam_counters: the BAM's GpuBgzf counters at the close.
    groupsort ((path, a call that gives the device)): a second BamWriter for the tool-stage
    records (Consensus.toolrec, pipeline.ToolrecPiece), whose whole blocks are
    checksummed and deflated on the GPU as bam_device's are; put()'s gcuts give its cuts as family
    indices (it holds every family, kept or not), and a mark's fourth offset is its length there."""

    def __init__(self, fault: Fault, out_bam: Optional[str], fastq, header, prefix: str, threads: int, level: int,
                 bufs: "bam.BufferPool", molecular: bool = False, gz_device=None, fragment: Optional[str] = None,
                 marks: Optional[list] = None, first_key=(MINKEY, 0, 1), tie: int = 1, on_written=None,
                 fq_device=None, bam_device=None, groupsort=None):
        self.fault, self.out_bam, self.fastq, self.header, self.prefix = fault, out_bam, fastq, header, prefix
        self.threads, self.level, self.bufs, self.molecular, self.gz_device = threads, level, bufs, molecular, gz_device
        self.fragment, self.first_key, self.tie, self.on_written = fragment, first_key, tie, on_written
        self.marks = [] if marks is None else marks
        self.fq_device, self.fastq_counters = fq_device, None
        self.bam_device, self.bam_counters = bam_device, None
        # groupsort: (path, a call that gives the device) -- the tool-stage records' BAM, a second
        # BamWriter fed from Consensus.toolrec; put()'s gcuts are its cuts, as family indices
        self.groupsort, self.groupsort_counters = groupsort, {"records": 0, "raw_bytes": 0}
        self.T = {"records": 0.0, "encode": 0.0, "writer_wait": 0.0}
        self.records_out = 0
        self.outs, self.recq = queue.Queue(maxsize=1), queue.Queue(maxsize=1)  # consensus -> builder -> writer
        self.workers = [threading.Thread(target=f, name="stream" + f.__name__, daemon=True)
                        for f in (self._builder, self._writer)]

    def put(self, cons, chunk: Chunk, cuts: Sequence = (), gcuts: Sequence = ()):
        self.outs.put((cons, chunk, list(cuts), list(gcuts)))

    def _builder(self):  # the output records of a chunk, while the writer compresses the one before
        try:
            while True:
                t0 = time.perf_counter()
                item = self.outs.get()
                self.T["writer_wait"] += time.perf_counter() - t0
                if item is None:
                    break
                cons, chunk, cuts, gcuts = item
                t0 = time.perf_counter()
                trec = (cons.toolrec, gcuts) if self.groupsort is not None else None
                text = cons.fastq if self.fq_device is not None else None
                brec = cons.bamrec if self.bam_device is not None else None
                # (the FASTQ pair's device text reads no records, nor do the BAM's device records)
                if (text is not None or self.fastq is None) and (brec is not None or self.out_bam is None):
                    recs, tags_buf = None, None
                else:
                    recs, tags_buf = bam.duplex_records(cons, chunk.raw, self.prefix, self.threads,
                                                        molecular=self.molecular, pool=self.bufs)
                self.T["records"] += time.perf_counter() - t0
                chunk.raw = chunk.plan = chunk.batches = None
                del item, cons
                self.recq.put((recs, tags_buf, chunk, cuts, text, brec, trec))
        except BaseException as e:  # noqa: BLE001
            self.fault(e)
            while self.outs.get() is not None:  # drain so that put() never blocks
                pass
        finally:
            self.recq.put(None)

    def _writer(self):
        w = fq = g = None
        th = self.threads
        try:
            gz = (lambda: bgzf.GpuBgzf(self.gz_device())) if self.gz_device is not None else (lambda: None)
            if self.out_bam is not None:  # (a GpuBgzf each: one job in flight)
                w = bgzf.BamWriter(self.out_bam, bam.output_header(self.header), self.level,
                                   bgzf.GpuBgzf(self.bam_device()) if self.bam_device is not None else gz(),
                                   self.fragment)
            if self.fastq is not None:
                fq = bgzf.FastqWriter(self.fastq[0], self.fastq[1], self.level,
                                      bgzf.GpuBgzf(self.fq_device()) if self.fq_device is not None else gz(),
                                      self.fragment is not None)
            if self.groupsort is not None:
                from . import toolrec as _toolrec
                g = bgzf.BamWriter(self.groupsort[0], _toolrec.header(self.header), self.level,
                                   bgzf.GpuBgzf(self.groupsort[1]()), self.fragment)
            self.marks.append(((0, 0, 0, 0), self.first_key))  # (a first piece holds the header, if any)
            while True:
                item = self.recq.get()
                if item is None:
                    break
                recs, tags_buf, chunk, cuts, text, brec, trec = item
                t1 = time.perf_counter()
                a = ga = 0
                n_out = recs.n if recs is not None else 2 * sum(x.kept for x in (text if text is not None else brec))
                part = None
                n_fam = sum(x.fams for x in trec[0]) if trec is not None else 0
                gcuts = (trec[1] if trec is not None else [0] * len(cuts)) + [n_fam]
                for (idx, key), gidx in zip(cuts + [(n_out, None)], gcuts):
                    if recs is not None:
                        part = recs if (a == 0 and idx == n_out) else _slice_records(recs, a, idx)
                    if idx > a:
                        if w is not None and brec is not None:
                            w.add_device([_rec_ranges(brec, a // 2, idx // 2)], th)
                        elif w is not None:
                            w.add(part, th)
                        if fq is not None and text is not None:
                            fq.add_device(_text_ranges(text, a // 2, idx // 2), th)
                        elif fq is not None:
                            fq.add(part, th)
                    if g is not None and gidx > ga:
                        _add_toolrec(g, trec[0], ga, gidx, th)
                    if key is not None:  # everything so far leaves as whole blocks; a piece starts here
                        bo = w.flush(th) if w is not None else 0
                        fo = fq.flush(th) if fq is not None else (0, 0)
                        go = g.flush(th) if g is not None else 0
                        self.marks.append(((bo, fo[0], fo[1], go), (key[0], key[1], self.tie)))
                    a, ga = idx, gidx
                self.records_out += n_out
                self.T["encode"] += time.perf_counter() - t1
                if trec is not None:
                    self.groupsort_counters["records"] += sum(x.n_rec for x in trec[0])
                    self.groupsort_counters["raw_bytes"] += sum(int(x.foff[-1]) for x in trec[0])
                del item, recs, part, text, brec, trec  # (the device bytes are released here, the job that reads them submitted)
                # (the chunk's records are written; nothing refers to their arrays)
                self.bufs.give(chunk.pool_buf)
                self.bufs.give(tags_buf)
                if self.on_written is not None:
                    self.on_written(chunk)
            if w is not None:
                w.close(th)
                if self.bam_device is not None:
                    c = w.gpu.counters()
                    self.bam_counters = {"blocks": c["blocks"], "raw_bytes": c["text_bytes"],
                                         "compressed_bytes": c["compressed_bytes"],
                                         "fallback_blocks": c["fallback_blocks"]}
            if fq is not None:
                fq.close(th)
                if self.fq_device is not None:
                    self.fastq_counters = fq.gpu.counters()
            if g is not None:
                g.close(th)
        except BaseException as e:  # noqa: BLE001
            self.fault(e)
            bgzf.close_quietly(w, fq, g)
            while self.recq.get() is not None:  # drain so the builder never blocks
                pass

    def __exit__(self, *exc):
        if exc[0] is not None:
            self.fault.stop.set()
        self.outs.put(None)
        for t in self.workers:
            t.join()


def step5_stream(in_bam: str, fasta: str, out_bam: Optional[str], engine=None, prefix: Optional[str] = None,
                 threads: int = 0, level: int = 6, fastq: Optional[Tuple[str, str]] = None, tags: bool = True,
                 chunk_bytes: int = bam.DEFAULT_CHUNK_BYTES, slack: int = bam.DEFAULT_SLACK,
                 batch_bases: Optional[int] = None, stats: Optional[dict] = None, gpu_bgzf: bool = False,
                 defer: Optional[int] = None, read_size: int = 8 << 20, filter=None, gpu_inflate: bool = False,
                 gpu_fastq: bool = False, gpu_bam: bool = False, gpu_image: bool = False,
                 metrics: Optional[str] = None, metrics_cycles: int = 512, groupsort_bam: Optional[str] = None) -> dict:
    """step5 in bounded memory, pipelined (run); defer: the span past which a template is
    deferred (default DEFAULT_DEFER_SPAN; 0 = off); read_size: compressed bytes per refill;
    filter: as step5's; gpu_inflate: the input's BGZF blocks inflate on the GPU (bgzf.GpuInflate);
    gpu_fastq: the FASTQ pair is formatted, checksummed and deflated on the GPU (StreamJob);
    gpu_bam: the BAM's records are written, checksummed and deflated on the GPU (StreamJob);
    gpu_image: the family images are made on the GPU from the records' bytes (StreamJob);
    metrics: the run's consensus metrics, reduced on the GPU, written to this JSON file (StreamJob);
    groupsort_bam: the records after tool 1 and tool 2, encoded on the GPU, written to this BAM (StreamJob)."""
    job = StreamJob(in_bam, fasta, out_bam, fastq, prefix, threads, level, tags, gpu_bgzf, chunk_bytes, slack,
                    batch_bases, read_size, filter=filter, defer=defer, gpu_inflate=gpu_inflate, gpu_fastq=gpu_fastq,
                    gpu_bam=gpu_bam, gpu_image=gpu_image, metrics=metrics, metrics_cycles=metrics_cycles,
                    groupsort_bam=groupsort_bam)
    return _public(run(job, engine, stats=stats))


def molecular_stream(in_bam: str, out_bam: Optional[str], engine=None, prefix: Optional[str] = None, threads: int = 0,
                     level: int = 6, fastq: Optional[Tuple[str, str]] = None, tags: bool = True,
                     chunk_bytes: int = bam.DEFAULT_CHUNK_BYTES, batch_bases: Optional[int] = None,
                     stats: Optional[dict] = None, gpu_bgzf: bool = False, min_consensus_base_quality: int = 0,
                     filter=None, gpu_inflate: bool = False, gpu_fastq: bool = False, gpu_bam: bool = False,
                     gpu_image: bool = False, metrics: Optional[str] = None, metrics_cycles: int = 512) -> dict:
    """Rule call_consensus_reads_molecular (main.snake.py:46-55) in bounded memory: the same
    pipeline as step5_stream over a GroupReadsByUmi-ordered input cut between MI runs
    (stream_chunks(runs=True)); each chunk's runs are its consensus families (pipeline.molecular_records,
    the vote alone, --min-consensus-base-quality applied).  The output is byte-identical to
    molecular()'s whole-file path: no run straddles two chunks.  The reference's rule needs -Xmx100g
    (main.snake.py:54, README.md:83); this holds about six chunks."""
    job = StreamJob(in_bam, None, out_bam, fastq, prefix, threads, level, tags, gpu_bgzf, chunk_bytes,
                    batch_bases=batch_bases, molecular=int(min_consensus_base_quality), filter=filter,
                    gpu_inflate=gpu_inflate, gpu_fastq=gpu_fastq, gpu_bam=gpu_bam, gpu_image=gpu_image, metrics=metrics,
                    metrics_cycles=metrics_cycles)
    return _public(run(job, engine, stats=stats))


def _public(info: dict) -> dict:
    """The stream's info as the CLI prints it (JSON): the spliced keys become their count"""
    sp = info.pop("splices", None)
    info["spliced_families"] = 0 if sp is None else int(len(sp))
    return info


def _family_cuts(cons, raw, plan, splices, strict: bool, start: int = 0, fams: Optional[list] = None):
    """Output record indices where a chunk's BAM / FASTQ output is cut before each splice key, in
    order: (record index, key) per key used.  A family's key is its first record's coarse key
    (RawRecords.tc_key).  strict (the main stream): before the first family whose key exceeds the
    splice (no family lies within kDeferMargin of one); else (the spill's pass): before the first
    family whose key reaches the splice minus kDeferMargin (a deferred template's two records may
    estimate its key a few positions apart).  splices[start:] are tried; a key no family of the
    chunk reaches is left (-> cuts, the index of the first key left).  fams: a list that receives
    the family index of every cut (the tool-stage records' BAM is cut there: it holds every family)."""
    F = int(cons.status.shape[0])
    if F == 0 or splices.shape[0] <= start:
        return [], start
    first = plan.order[plan.fam_off[:-1]]
    k0, k1 = raw.tc_key[first, 0], raw.tc_key[first, 1]
    em = np.zeros(F + 1, np.int64)
    em[1:] = np.cumsum(_filter.kept(cons))
    out, lo, j = [], 0, start
    while j < splices.shape[0]:
        s0, s1 = int(splices[j, 0]), int(splices[j, 1]) - (0 if strict else bam.DEFER_MARGIN)
        hit = (k0 > s0) | ((k0 == s0) & ((k1 > s1) if strict else (k1 >= s1)))
        hit[:lo] = False
        if not hit.any():
            if not strict:  # (the pass's later chunks take it)
                break
            f = F
        else:
            f = int(np.argmax(hit))
        lo = max(lo, f)
        out.append((2 * int(em[lo]), (int(splices[j, 0]), int(splices[j, 1]))))
        if fams is not None:
            fams.append(int(lo))
        j += 1
    return out, j


def _region_cuts(cons, raw, plan, prev: int):
    """Output record indices where a chunk's output is cut before the first family of each new key
    contig pair (a family's key: its first record's coarse key), keyed (pair, MINKEY); prev = the
    pair of the family before the chunk (at first: that of the range's first piece's key)
    -> cuts, the pair of the chunk's last family."""
    first = plan.order[plan.fam_off[:-1]]
    k0 = raw.tc_key[first, 0]
    em = np.zeros(k0.shape[0] + 1, np.int64)
    em[1:] = np.cumsum(_filter.kept(cons))
    before = np.empty_like(k0)
    before[0] = prev
    before[1:] = k0[:-1]
    return [(2 * int(em[f]), (int(k0[f]), MINKEY)) for f in np.nonzero(k0 != before)[0]], int(k0[-1])


def _text_ranges(text, a: int, b: int) -> list:
    """Kept families a..b-1 of a chunk whose batches' device text is `text` (pipeline.FastqPiece
    each, in order) -> FastqWriter.add_device's pieces: per file, the byte ranges in order."""
    out, k0 = [[], []], 0
    for x in text:
        lo, hi = max(a - k0, 0), min(b - k0, x.kept)
        if hi > lo:
            for d, r in enumerate(x.ranges(lo, hi)):
                out[d] += r
        k0 += x.kept
    return out


def _add_toolrec(g, pieces, a: int, b: int, threads: int):
    """Families a..b-1 of a chunk whose batches' tool-stage records are `pieces` (pipeline.ToolrecPiece
    each, in order) join the BAM writer g: device records as byte ranges (add_device), the host
    twin's as raw records."""
    dev, k0 = [], 0
    for x in pieces:
        lo, hi = max(a - k0, 0), min(b - k0, x.fams)
        k0 += x.fams
        if hi <= lo:
            continue
        if x.event is not None:
            dev += x.ranges(lo, hi)
            continue
        if dev:
            g.add_device([dev], threads)
            dev = []
        g.add_raw(x.host(lo, hi), threads)
    if dev:
        g.add_device([dev], threads)


def _rec_ranges(brec, a: int, b: int) -> list:
    """Kept families a..b-1 of a chunk whose batches' device records are `brec` (pipeline.BamPiece
    each, in order) -> the BAM's byte ranges in order (BamWriter.add_device's pieces[0]); output
    record k is record k & 1 of kept family k // 2."""
    out, k0 = [], 0
    for x in brec:
        lo, hi = max(a - k0, 0), min(b - k0, x.kept)
        if hi > lo:
            out += x.ranges(lo, hi)
        k0 += x.kept
    return out


def _slice_records(recs: "bam.OutRecordsBam", a: int, b: int) -> "bam.OutRecordsBam":
    """Records a..b-1 as views (the encoders index the ragged fields by absolute offsets)."""
    ST = bam.StringTable
    return bam.OutRecordsBam(flag=recs.flag[a:b], tid=recs.tid[a:b], pos=recs.pos[a:b], mapq=recs.mapq[a:b],
                             next_tid=recs.next_tid[a:b], next_pos=recs.next_pos[a:b], tlen=recs.tlen[a:b],
                             names=ST(recs.names.buf, recs.names.off[a:b + 1]), cig_off=recs.cig_off[a:b + 1],
                             cigar=recs.cigar, seq_off=recs.seq_off[a:b + 1], seq=recs.seq, qual=recs.qual,
                             aux=ST(recs.aux.buf, recs.aux.off[a:b + 1]),
                             aux2=ST(recs.aux2.buf, recs.aux2.off[a:b + 1]) if recs.aux2 is not None else None)


def pieces_of(marks, paths, phase: int, rank: int) -> list:
    """One output's pieces between its marks (BackEnd): (sort key, phase, rank, index, paths,
    starts, ends), ends of the last piece = the files' sizes."""
    out = []
    size = [os.path.getsize(x) if x else 0 for x in paths]
    for i, (offs, key) in enumerate(marks):
        end = list(marks[i + 1][0]) if i + 1 < len(marks) else size
        out.append((tuple(key), phase, rank, i, list(paths), list(offs), end))
    return out


def assemble(dst: str, pieces, k: int):
    """Output file k (0 the BAM, 1 / 2 the FASTQ pair, 3 the tool-stage records' BAM) from the pieces in sort-key order, then one
    BGZF EOF block; written aside and renamed over dst."""
    tmp = dst + ".asm"
    with open(tmp, "wb") as out:
        for p in sorted(pieces, key=lambda x: (x[0], x[1], x[2], x[3])):
            path, a, b = p[4][k], p[5][k], p[6][k]
            if path is None or b <= a:
                continue
            with open(path, "rb") as f:
                f.seek(a)
                left = b - a
                while left > 0:
                    buf = f.read(min(left, 1 << 24))
                    if not buf:
                        raise RuntimeError("%s: short piece" % path)
                    out.write(buf)
                    left -= len(buf)
        out.write(EOF_BLOCK)
    os.replace(tmp, dst)


def write_spill_bam(dst: str, header: "bam.BamHeader", spills: Sequence[str], level: int = 1, threads: int = 0) -> int:
    """The spill files' records (bsdc_bam_stream_spill entries) in file order as a BAM -> records."""
    data = b"".join(open(x, "rb").read() for x in spills if x and os.path.exists(x))
    recs, n = bam.spill_sorted_records(data)
    del data
    w = bgzf.BamWriter(dst, header, level)
    try:
        w.add_raw(recs, threads)
    finally:
        w.close(threads)
    return n


def _run_chunk(eng, runner, ch: Chunk, mode: int, tags: bool, job: StreamJob, G: dict):
    """The GPU stage of one chunk (split_ext: pipeline.run_step5 on its records) -> its Consensus."""
    if runner is not None:
        if ch.batches is None:
            return runner.run_chunk(ch.raw, tags, job.batch_bases)
        parts = []
        for fb in ch.batches:
            sub = R.take(ch.raw, fb.src) if getattr(runner, "needs_raw", False) else None
            parts.append(pipeline.consensus_from_output(fb, runner.run_batch(fb, mode, tags, sub)))
        return pipeline.concat_consensus(parts)
    if ch.batches is None:  # (gpu_image: the whole-chunk path reads unpacked bases)
        mkw = {} if job.metrics is None else {"metrics": True}
        if job.groupsort_bam is not None:
            mkw["toolrec"] = "device"
        return pipeline.run_step5(eng, R.unpack_bases(ch.raw), tags=tags, batch_bases=job.batch_bases,
                                  filter=job.filter, **mkw)[0]
    fkw = {} if job.filter is None else {"filter": job.filter, "molecular": job.molecular is not None}
    if job.metrics is not None:  # each batch is reduced into the engine's accumulator after its vote
        fkw.update(metrics=True, molecular=job.molecular is not None)
    raw = ch.raw
    names = lambda fb: bam.family_names(fb.fam_mi, raw.mi_names, job.prefix)  # noqa: E731
    # an output formatted on the host reads the fetched bases: the BAM without gpu_bam, the pair without gpu_fastq
    host_out = (job.out_bam is not None and not job.gpu_bam) or (job.fastq is not None and not job.gpu_fastq)
    if job.gpu_fastq:  # the batches' FASTQ text is made where their consensus lies
        fkw.update(fastq_names=names, seqqual=host_out)
    if job.gpu_bam:  # so are the BAM's records; the tags' rows then stay in HBM
        fkw.update(bam_tables=lambda fb: (names(fb), bam.family_aux(fb.fam_off, fb.src, fb.fam_mi, raw, job.threads)),
                   bam_tags=job.tags, seqqual=host_out, molecular=job.molecular is not None)
        tags = False
    if job.gpu_image:  # the batches carry no images: they are made in HBM from the chunk's bytes
        fkw.update(raw_bases=raw.raw_bases)
    if job.groupsort_bam is not None:  # the records after the tools are written where their dump lies
        from . import toolrec as _toolrec
        fkw.update(toolrec=lambda fb: _toolrec.batch_tables(raw, fb))
    return pipeline.concat_consensus(pipeline.run_batches(eng, ch.batches, mode, tags, G, **fkw))


def run(job: StreamJob, engine=None, runner=None, stats: Optional[dict] = None, range_stats: Optional[dict] = None,
        marks: Optional[list] = None) -> dict:
    """The one-GPU stream of `job` (module docstring): the GPU stage between a FrontEnd and a
    BackEnd.  engine: the Engine to run on (default: one on device 0, closed here; a rank's may
    still be loading, ranks._LazyEngine); runner: a fleet-style runner (run_batch / run_chunk; the
    CPU stand-in of the tests) instead -- step 5 with host deflate only, unfiltered; stats
    receives the stages' seconds, range_stats the input range's statistics once read; marks: a list
    that receives the output's cut points (BackEnd) -- the caller (ranks.py) then runs the second
    pass and the assembly.
    Deferred templates (step 5; job.defer): a template whose other end lies far away or on another
    contig (bsdc_bam_stream_set_defer) would hold every family after its key in memory until the
    stream reaches that end.  Its records go to a spill file instead (with every family that may
    interleave with it), and the output is cut, at every deferred key, into pieces (marks).  At
    the end a second pass (_finish_deferred) runs the spill's records (in file order, their own
    BAM; memory as their count) with the same keys (late_splices: each cut before the first family
    that reaches the key), and the pieces of both are assembled in key order: the same records as
    the whole file's.  Without deferred templates the output is written in place."""
    molecular = job.molecular is not None
    own = engine is None and runner is None
    if runner is None:
        if own:
            from .device import Engine
        eng = Engine(0) if own else engine
    else:
        eng = None
        if job.gpu_bgzf or molecular or job.filter is not None or job.gpu_inflate or job.gpu_fastq or job.gpu_bam:
            raise ValueError("a runner stream: step 5 with host inflate and deflate only, unfiltered "
                             "(no gpu_bgzf, gpu_inflate, gpu_fastq or gpu_bam)")
        if job.gpu_image:
            raise ValueError("a runner stream makes the family images on the host (no gpu_image)")
    if job.metrics is not None and runner is not None:
        raise ValueError("a runner stream reduces no metrics (no metrics: one process, one GPU)")
    if job.metrics is not None and (job.rng is not None or job.owner is not None):
        raise ValueError("metrics is not supported in a rank's stream yet (one process, one GPU)")
    if job.gpu_image and (job.rng is not None or job.owner is not None):
        raise ValueError("gpu_image is not supported in a rank's stream yet (one process, one GPU)")
    if job.groupsort_bam is not None:
        if runner is not None:
            raise ValueError("a runner stream writes no groupsort_bam (one process, one GPU)")
        if job.rng is not None or job.owner is not None:
            raise ValueError("groupsort_bam is not supported in a rank's stream yet (one process, one GPU)")
        if molecular:
            raise ValueError("groupsort_bam applies to step 5 only: step 1 runs no tools")
    if job.gpu_fastq and job.fastq is None:
        raise ValueError("gpu_fastq needs the FASTQ pair (fastq=(path1, path2))")
    if job.gpu_bam and job.out_bam is None:
        raise ValueError("gpu_bam needs the output BAM (out_bam)")
    out_bam, fastq = job.out_bam, job.fastq
    info = {"records_in": 0, "families": 0, "families_emitted": 0, "records_out": 0, "chunks": 0,
            "spilled_bytes": 0, "deferred_families": 0, "splices": []}
    if job.filter is not None:
        info["filter"] = _filter.empty_summary()
    # deferral (step 5): the spill file and the output's pieces
    dspan = 0 if molecular else (bam.DEFAULT_DEFER_SPAN if job.defer is None else int(job.defer))
    late = None if job.late_splices is None else np.asarray(job.late_splices, np.int64).reshape(-1, 2)
    lj = 0  # (the spill's pass: the first deferred key not yet cut at)
    solo = marks is None and late is None  # this call runs the spill's pass and the assembly itself
    # (the spill pass's first piece, before its first key, is empty: after the header in any case)
    k_first = tuple(job.first_key) if job.first_key is not None else (MINKEY, 0, 2 if late is not None else 1)
    pair = int(k_first[0])  # (regions: the key contig pair of the last family written; a range whose
    # first family lies in a later contig pair: cut before it)
    out0 = out_bam if out_bam is not None else fastq[0]
    spill_path = None
    if dspan:
        spill_path = job.spill if job.spill is not None else os.path.join(
            os.path.dirname(os.path.abspath(out0)), ".%s.%d.%x.spill" % (os.path.basename(out0), os.getpid(), id(info)))
    T, G = {"gpu": 0.0}, {}  # G: the GPU stage's host steps (pipeline.run_batches timing)
    bufs = bam.BufferPool()  # a chunk's record arrays, given back once its output is written
    rs = range_stats if range_stats is not None else {}
    # the header and the reference come first: the plan of a chunk needs the reference
    header = bam.read_bam_header(job.in_bam)
    ref = None if molecular else bam.read_fasta(job.fasta, header)  # (step 1 converts nothing)
    prefix = bam.read_name_prefix(header) if job.prefix is None else job.prefix
    flags = eng.flags(min_consensus_base_quality=job.molecular) if molecular else contextlib.nullcontext()
    try:
        flags.__enter__()
    except BaseException:
        if own:
            eng.close()
        raise
    fault = Fault()
    inflater = None
    try:
        if job.metrics is not None and late is None:  # (the deferred templates' pass adds into the same one)
            eng.metrics_begin(job.metrics_cycles)
        if ref is not None:
            (runner if runner is not None else eng).load_reference(ref)
        if job.gpu_inflate:  # (called on the decoder thread, on its own HIP stream)
            inflater = bgzf.GpuInflate(eng.device)
        source = dict(path=job.in_bam, threads=job.threads, chunk_bytes=job.chunk_bytes, slack=job.slack,
                      read_size=job.read_size, runs=molecular, rng=job.rng, stats=rs, owner=job.owner, defer=dspan,
                      keys=late is not None, inflater=inflater)
        pinned = PinnedRaw() if job.gpu_image else None
        front = FrontEnd(fault, source, plan_molecular if molecular else functools.partial(plan_step5, ref=ref),
                         pipeline.materialize_ranges if runner is not None else PinnedBatches(eng, job.gpu_image),
                         job.threads, job.batch_bases, bufs, spill_path, pinned=pinned)
        back = BackEnd(fault, out_bam, fastq, header, prefix, job.threads, job.level, bufs, molecular,
                       (lambda: eng.device) if job.gpu_bgzf else None,
                       "first" if (solo and dspan) else job.fragment, marks, k_first,
                       tie=0 if late is not None else 1,  # (a spill piece sorts before the stream's piece of its key)
                       fq_device=(lambda: eng.device) if job.gpu_fastq else None,
                       bam_device=(lambda: eng.device) if job.gpu_bam else None,
                       groupsort=(job.groupsort_bam, lambda: eng.device) if job.groupsort_bam is not None else None,
                       on_written=(lambda ch: pinned.give(ch.pin_buf)) if pinned is not None else None)
        pjob = dataclasses.replace(job, prefix=prefix)  # (the read names' prefix, resolved)
        mode = pipeline.MODE_VOTE if molecular else pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE
        tg = job.tags and out_bam is not None  # the FASTQ pair carries no tags
        with front, back:
            for ch in front:
                t0 = time.perf_counter()
                cons = _run_chunk(eng, runner, ch, mode, tg, pjob, G)
                ch.batches = None
                T["gpu"] += time.perf_counter() - t0
                info["records_in"] += ch.raw.n
                info["families"] += int(cons.status.shape[0])
                info["families_emitted"] += int(((cons.status & 1) != 0).sum())
                info["chunks"] += 1
                if job.filter is not None:
                    info["filter"] = _filter.add_summary(info["filter"], _filter.summary(cons))
                cuts, gcuts = [], []
                if late is not None:  # the spill's pass: cut before the families of each deferred key
                    cuts, lj = _family_cuts(cons, ch.raw, ch.plan, late, False, lj, gcuts)
                elif ch.splices is not None and ch.splices.shape[0]:
                    cuts, _ = _family_cuts(cons, ch.raw, ch.plan, ch.splices, True, fams=gcuts)
                    info["splices"].append(ch.splices)
                if job.regions and cons.status.shape[0]:
                    rc, pair = _region_cuts(cons, ch.raw, ch.plan, pair)
                    cuts = sorted(cuts + rc)
                back.put(cons, ch, cuts, gcuts)
                del ch, cons
        if inflater is not None:
            info["gpu_inflate"] = inflater.counters()
            if inflater.error is not None:  # (the reader saw a failed call as a corrupt block)
                fault.errors.insert(0, inflater.error)
        if not fault.errors:
            if job.gpu_fastq:
                info["gpu_fastq"] = back.fastq_counters
            if job.gpu_bam:
                info["gpu_bam"] = back.bam_counters
            if job.groupsort_bam is not None:
                info["groupsort_bam"] = dict(back.groupsort_counters)
            info["records_out"] = back.records_out
            info["spilled_bytes"] = front.spilled_bytes
            info["deferred_families"] = int(rs.get("deferred", 0))
            info["peak_buffered"] = int(rs.get("peak_buffered", 0))
            info["splices"] = np.concatenate(info["splices"] + [front.splices_tail, np.zeros((0, 2), np.int64)]) \
                if dspan else np.zeros((0, 2), np.int64)
            if solo and dspan:  # the deferred templates' pass and the assembly (or just the EOF blocks)
                _finish_deferred(dataclasses.replace(job, prefix=prefix), eng, runner, back.marks, spill_path, info)
            if job.metrics is not None and late is None:
                from . import metrics as _metrics
                _metrics.write(job.metrics, eng.metrics_fetch(), job.metrics_cycles,
                               _metrics.run_params(eng.params, molecular, job.filter))
                info["metrics"] = job.metrics
            if job.groupsort_bam is not None and os.path.exists(job.groupsort_bam):
                info["groupsort_bam"]["compressed_bytes"] = os.path.getsize(job.groupsort_bam)
    finally:
        flags.__exit__(None, None, None)
        if own:
            eng.close()
        if solo and spill_path is not None and os.path.exists(spill_path):
            os.unlink(spill_path)
    if fault.errors:
        raise fault.errors[0]
    if stats is not None:
        T.update(decode=front.T["decode"], plan=front.T["plan"], materialize=front.T["materialize"],
                 gpu_wait=front.T["wait"], **back.T)
        stats.update({k: round(v, 4) for k, v in T.items()})
        stats.update({"gpu_" + k: round(v, 4) for k, v in G.items()})
        stats.update({"reader_" + k: round(v, 4) for k, v in front.R.items()})
    return info


def _finish_deferred(job: StreamJob, eng, runner, marks, spill_path: str, info: dict):
    """One process's deferred templates: with none, the EOF blocks the fragment-mode writers left
    out; else the spill's records as their own BAM through the stream (no deferral; cut at every
    deferred key), then the pieces of both outputs assembled in key order."""
    out_bam, fastq = job.out_bam, job.fastq
    paths = [out_bam, fastq[0] if fastq else None, fastq[1] if fastq else None, job.groupsort_bam]
    if info["splices"].shape[0] == 0 and info["spilled_bytes"] == 0:
        for x in paths:
            if x is not None:
                with open(x, "ab") as f:
                    f.write(EOF_BLOCK)
        return
    base, sb = spill_path + ".p2", spill_path + ".p2.bam"
    p2 = [base + ".out.bam" if out_bam is not None else None,
          base + ".1.fq.gz" if fastq else None, base + ".2.fq.gz" if fastq else None,
          base + ".gs.bam" if job.groupsort_bam is not None else None]
    try:
        info["deferred_records"] = write_spill_bam(sb, bam.read_bam_header(job.in_bam), [spill_path], 1, job.threads)
        mk2: list = []
        inf2 = run(dataclasses.replace(job, in_bam=sb, out_bam=p2[0], fastq=(p2[1], p2[2]) if fastq else None,
                                       fragment="next", defer=0, late_splices=info["splices"], read_size=8 << 20,
                                       groupsort_bam=p2[3]),
                   eng, runner, marks=mk2)
        for k in ("records_in", "families", "families_emitted", "records_out"):
            info[k] += inf2[k]
        if "gpu_fastq" in inf2:
            info["gpu_fastq"] = {k: v + inf2["gpu_fastq"][k] for k, v in info["gpu_fastq"].items()}
        if "gpu_bam" in inf2:
            info["gpu_bam"] = {k: v + inf2["gpu_bam"][k] for k, v in info["gpu_bam"].items()}
        if "groupsort_bam" in inf2:
            for k in ("records", "raw_bytes"):
                info["groupsort_bam"][k] += inf2["groupsort_bam"][k]
        if "gpu_inflate" in inf2:  # (the spill's BAM, inflated the same way)
            info["gpu_inflate_deferred"] = inf2["gpu_inflate"]
        if job.filter is not None:
            info["filter"] = _filter.add_summary(info["filter"], inf2["filter"])
        pieces = pieces_of(marks, paths, 0, 0) + pieces_of(mk2, p2, 1, 0)
        for k in range(4):
            if paths[k] is not None:
                assemble(paths[k], pieces, k)
    finally:
        for x in [sb] + p2:
            if x is not None and os.path.exists(x):
                os.unlink(x)

"""The file-level step-5 drop-in: BAM in -> duplex consensus BAM out.

The reference's step 5 is four Snakemake rules over files (main.snake.py:121-164): tool 1 and
tool 2 read and write BAM through pysam, fgbio SortBam writes the TemplateCoordinate-sorted BAM,
and CallDuplexConsensusReads writes the unmapped consensus pairs.  Here one call reads the input
BAM (libbsdc_io: BGZF inflated and records parsed in parallel, include/bsdc_io.h), runs the fused
device path (pipeline.run_step5: tools 1+2, TemplateCoordinate families, vote, duplex), builds
fgbio's output records and writes them (libbsdc_io: BGZF deflated in
parallel).

Output records (fgbio DuplexConsensusCaller as restated; PARITY UNPINNED -- fgbio is not
vendored): an unmapped pair per emitted family, R1 flag 77 and R2 flag 141, name
``<prefix>:<MI base>``, tags RG:Z:A, MI:Z:<MI base>, RX:Z:<consensus UMI> (when the inputs carry
RX), then fgbio's consensus tags when the consensus was called with tags=True (the default of
the file-level calls, as fgbio's --output-per-base-tags defaults to true): per read cD cM cE,
aD aM aE, bD bM bE; per base ad ae ac aq, bd be bc bq (molecular: cD cM cE, cd ce), encoded by
libbsdc_io (bsdc_consensus_tags) from the single-strand reads the kernels write.  The consumer of
this file (SamToFastq, main.snake.py:167-177) reads name, flag, SEQ and QUAL only.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import filter as _filter
from . import records as R

IO_LIB_PATH = os.environ.get("BSDC_IO_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                 "libbsdc_io.so")
BSDC_IO_ABI_VERSION = 16
_P = C.c_void_p
# bsdc_inflate_fn (include/bsdc_io.h): user, comp, n_comp, blk, nblk, out, n_out -> 0 or an error
INFLATE_FN = C.CFUNCTYPE(C.c_int32, _P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64)


class _Sizes(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_rec", "n_bases", "n_cigar", "n_mc", "aux_bytes", "n_names", "name_bytes",
                                         "n_mi", "mi_bytes", "header_bytes")] + \
               [("n_ref", C.c_int32), ("ref_name_bytes", C.c_int64)]


class _Arrays(C.Structure):
    _fields_ = [(k, _P) for k in (
        "flag", "tid", "pos", "mapq", "l_seq", "seq_off", "seq", "qual", "cig_off", "n_cig", "cigar", "next_tid",
        "next_pos", "tlen", "name_id", "name_off", "name_buf", "mi_id", "mi_strand", "mi_off", "mi_buf", "mc_off",
        "mc_n", "mc_cigar", "la", "rd", "aux_off", "aux", "header", "ref_len", "ref_name_off", "ref_name_buf",
        "raw_bases", "seq_src")]


class _Records(C.Structure):
    _fields_ = [("n_rec", C.c_int64)] + [(k, _P) for k in (
        "flag", "tid", "pos", "mapq", "next_tid", "next_pos", "tlen", "name_off", "name_buf", "cig_off", "cigar",
        "seq_off", "seq", "qual", "aux_off", "aux", "aux2_off", "aux2")]


_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(IO_LIB_PATH):
        raise RuntimeError("%s is missing: run __graft_entry__.build()" % IO_LIB_PATH)
    lib = C.CDLL(IO_LIB_PATH)  # (OMP_WAIT_POLICY: see the package __init__)
    lib.bsdc_io_abi_version.restype = C.c_int32
    lib.bsdc_io_last_error.restype = C.c_char_p
    lib.bsdc_bam_read.argtypes = [C.c_char_p, C.c_int32, C.POINTER(_P)]
    lib.bsdc_bam_read.restype = C.c_int32
    lib.bsdc_bam_sizes_of.argtypes = [_P, C.POINTER(_Sizes)]
    lib.bsdc_bam_copy.argtypes = [_P, C.POINTER(_Arrays)]
    lib.bsdc_bam_copy.restype = C.c_int32
    lib.bsdc_bam_free.argtypes = [_P]
    lib.bsdc_bam_stream_open.argtypes = [C.c_char_p, C.c_int32, C.c_int64, C.POINTER(_P)]
    lib.bsdc_bam_stream_open.restype = C.c_int32
    lib.bsdc_bam_stream_next.argtypes = [_P, C.c_int64, C.c_int64, C.POINTER(_P)]
    lib.bsdc_bam_stream_next.restype = C.c_int32
    lib.bsdc_bam_stream_next_raw.argtypes = [_P, C.c_int64, C.c_int64, C.POINTER(_P)]
    lib.bsdc_bam_stream_next_raw.restype = C.c_int32
    lib.bsdc_bam_stream_next_runs.argtypes = [_P, C.c_int64, C.POINTER(_P)]
    lib.bsdc_bam_stream_next_runs.restype = C.c_int32
    lib.bsdc_bam_parse.argtypes = [_P, C.c_int32]
    lib.bsdc_bam_parse.restype = C.c_int32
    lib.bsdc_bam_stream_close.argtypes = [_P]
    lib.bsdc_bam_stream_recycle.argtypes = [_P, _P]
    lib.bsdc_bam_stream_recycle.restype = None
    lib.bsdc_bam_stream_header.argtypes = [_P, C.POINTER(_P)]
    lib.bsdc_bam_stream_header.restype = C.c_int32
    # the streaming writers (what both have, then what one has) and their BGZF sinks
    rec = C.POINTER(_Records)
    decl = {"bam_writer_open": [C.c_char_p, C.c_char_p, C.c_int64, C.c_int32, _P, _P, _P, C.c_int32, C.POINTER(_P)],
            "fastq_writer_open": [C.c_char_p, C.c_char_p, C.c_int32, C.POINTER(_P)],
            "bam_writer_fragment": [_P, C.c_int32], "fastq_writer_fragment": [_P],
            "bam_writer_raw": [_P, _P, C.c_int64, C.c_int32],
            "bgzf_sink_take": [_P, C.c_int64, _P, _P, C.c_int32],
            "bgzf_sink_put": [_P, C.c_int64, _P, _P, _P, _P, C.c_int32],
            "bgzf_sink_append": [_P, _P, C.c_int64]}
    for kind in ("bam", "fastq"):
        decl.update({kind + "_writer_add": [_P, rec, C.c_int32], kind + "_writer_encode": [_P, rec, C.c_int32],
                     kind + "_writer_flush": [_P, C.c_int32], kind + "_writer_close": [_P, C.c_int32]})
    for name, args in decl.items():
        fn = getattr(lib, "bsdc_" + name)
        fn.argtypes, fn.restype = args, C.c_int32
    lib.bsdc_bam_writer_sink.argtypes, lib.bsdc_bam_writer_sink.restype = [_P], _P
    lib.bsdc_fastq_writer_sink.argtypes, lib.bsdc_fastq_writer_sink.restype = [_P, C.c_int32], _P
    lib.bsdc_bgzf_sink_whole.argtypes, lib.bsdc_bgzf_sink_whole.restype = [_P], C.c_int64
    lib.bsdc_bgzf_sink_tell.argtypes, lib.bsdc_bgzf_sink_tell.restype = [_P], C.c_int64
    lib.bsdc_bgzf_sink_take_tail.argtypes, lib.bsdc_bgzf_sink_take_tail.restype = [_P, _P, C.c_int64], C.c_int64
    lib.bsdc_bam_write.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int32, _P, _P, _P, C.POINTER(_Records),
                                   C.c_int32, C.c_int32]
    lib.bsdc_bam_write.restype = C.c_int32
    lib.bsdc_rx_consensus.argtypes = [C.c_int64, _P, _P, _P, _P, _P, _P, _P, C.c_int32]
    lib.bsdc_rx_consensus.restype = C.c_int64
    lib.bsdc_fastq_write.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(_Records), C.c_int32, C.c_int32]
    lib.bsdc_fastq_write.restype = C.c_int32
    lib.bsdc_family_image.argtypes = [C.c_int64, _P, _P, _P, _P, _P, C.c_int64, _P, _P, C.c_int32]
    lib.bsdc_family_image.restype = C.c_int32
    lib.bsdc_consensus_tags.argtypes = [C.c_int64, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P,
                                        _P, _P, C.c_int32]
    lib.bsdc_consensus_tags.restype = C.c_int64
    lib.bsdc_table_concat.argtypes = [C.c_int64, C.c_int32, C.POINTER(_P), C.POINTER(_P), _P, _P, _P, C.c_int32]
    lib.bsdc_table_concat.restype = C.c_int64
    lib.bsdc_table_rank.argtypes = [C.c_int64, _P, _P, _P, C.c_int32]
    lib.bsdc_table_rank.restype = None
    lib.bsdc_table_take.argtypes = [C.c_int64, _P, _P, _P, _P, _P, C.c_int32]
    lib.bsdc_table_take.restype = C.c_int64
    lib.bsdc_unpack_nibbles.argtypes = [C.c_int64, _P, _P, C.c_int32]
    lib.bsdc_unpack_nibbles.restype = None
    lib.bsdc_rows_gather.argtypes = [C.c_int64, _P, _P, C.c_int64, _P, _P, _P, C.c_int32]
    lib.bsdc_rows_gather.restype = None
    lib.bsdc_bam_find_cut.argtypes = [C.c_char_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                      _P]
    lib.bsdc_bam_find_cut.restype = C.c_int32
    lib.bsdc_bam_stream_open_range.argtypes = [C.c_char_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                               C.c_int64, C.POINTER(_P)]
    lib.bsdc_bam_stream_open_range.restype = C.c_int32
    lib.bsdc_bam_stream_set_owner.argtypes = [_P, C.c_int32, _P, C.c_int32, C.c_int64, C.c_int32]
    lib.bsdc_bam_stream_set_owner.restype = C.c_int32
    lib.bsdc_bam_stream_spill.argtypes = [_P, _P]
    lib.bsdc_bam_stream_spill.restype = C.c_int64
    lib.bsdc_bam_stream_set_defer.argtypes = [_P, C.c_int64]
    lib.bsdc_bam_stream_set_defer.restype = C.c_int32
    lib.bsdc_bam_stream_set_inflater.argtypes = [_P, INFLATE_FN, _P]
    lib.bsdc_bam_stream_set_inflater.restype = C.c_int32
    lib.bsdc_bam_stream_splices.argtypes = [_P, _P]
    lib.bsdc_bam_stream_splices.restype = C.c_int64
    lib.bsdc_bam_rec_keys.argtypes = [_P, _P]
    lib.bsdc_bam_rec_keys.restype = C.c_int32
    lib.bsdc_spill_sort.argtypes = [_P, C.c_int64, _P, _P]
    lib.bsdc_spill_sort.restype = C.c_int64
    lib.bsdc_bam_stream_range_stats.argtypes = [_P, _P]
    lib.bsdc_bam_stream_range_stats.restype = None
    if lib.bsdc_io_abi_version() != BSDC_IO_ABI_VERSION:
        raise RuntimeError("libbsdc_io ABI %d != %d" % (lib.bsdc_io_abi_version(), BSDC_IO_ABI_VERSION))
    _lib = lib
    return lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_P)


class StringTable:
    """Strings packed in one buffer (``buf[off[i]:off[i+1]]``); indexing gives bytes (or str)."""

    def __init__(self, buf: np.ndarray, off: np.ndarray, as_str: bool = False):
        self.buf = np.ascontiguousarray(buf, np.uint8)
        self.off = np.ascontiguousarray(off, np.int64)
        self.as_str = as_str

    def __len__(self):
        return int(self.off.shape[0]) - 1

    def __getitem__(self, i):
        b = self.buf[int(self.off[i]):int(self.off[i + 1])].tobytes()
        return b.decode() if self.as_str else b

    @staticmethod
    def from_list(items) -> "StringTable":
        bs = [x if isinstance(x, bytes) else str(x).encode() for x in items]
        off = np.zeros(len(bs) + 1, np.int64)
        if bs:
            off[1:] = np.cumsum([len(x) for x in bs])
        return StringTable(np.frombuffer(b"".join(bs), np.uint8) if bs else np.zeros(0, np.uint8), off,
                           as_str=bool(items) and isinstance(items[0], str))

    def lex_key(self, ids: np.ndarray) -> np.ndarray:
        """A key per id ordering the ids as their strings sort in byte order (vectorised)."""
        ids = np.asarray(ids, np.int64)
        if ids.shape[0] == 0:
            return np.zeros(0, np.int64)
        u, inv = np.unique(ids, return_inverse=True)
        lens = self.off[u + 1] - self.off[u]
        w = max(int(lens.max()), 1)
        j = np.arange(w)[None, :]
        idx = self.off[u][:, None] + j
        m = np.where(j < lens[:, None], self.buf[np.minimum(idx, max(self.buf.shape[0] - 1, 0))], 0).astype(np.uint8)
        fixed = np.ascontiguousarray(m).view("S%d" % w).reshape(-1)
        _, rk = np.unique(fixed, return_inverse=True)
        return rk.astype(np.int64)[inv]


@dataclass
class BamHeader:
    text: str
    ref_names: List[str]
    ref_lens: np.ndarray

    def read_groups(self) -> List[dict]:
        out = []
        for line in self.text.splitlines():
            if line.startswith("@RG"):
                out.append(dict(f.split(":", 1) for f in line.split("\t")[1:] if ":" in f))
        return out


class BufferPool:
    """Host byte buffers handed from one stream chunk's decoded records to a later chunk's
    (bam.step5_stream): a fresh array of a few hundred MB costs its page faults and the kernel's
    zeroing on every chunk.  take() the smallest free buffer that fits (or a new one), give() it
    back once nothing refers to the arrays carved from it."""

    def __init__(self, keep: int = 6):
        import threading
        self.free: list = []
        self.keep = keep
        self.lock = threading.Lock()

    def take(self, nbytes: int) -> np.ndarray:
        with self.lock:
            fit = [i for i, b in enumerate(self.free) if b.size >= nbytes]
            if fit:
                return self.free.pop(min(fit, key=lambda i: self.free[i].size))
        return np.empty(max(int(nbytes * 1.15), 1), np.uint8)

    def give(self, buf: Optional[np.ndarray]):
        if buf is None:
            return
        with self.lock:
            self.free.append(buf)
            if len(self.free) > self.keep:  # drop the smallest (by position: arrays do not compare)
                del self.free[min(range(len(self.free)), key=lambda i: self.free[i].size)]


def _decode(lib, h, what: str, pool: Optional[BufferPool] = None, packed: bool = False, pin=None):
    """A bsdc_bam handle (whole file or stream chunk) -> (BamHeader, RawRecords, pooled buffer);
    frees nothing.  With `pool`, the record arrays are carved from one pooled buffer (bsdc_bam_copy
    writes every element), returned for the caller to give back (else None).  packed: no unpacked
    bases (RawRecords.seq / qual None): the records' SEQ and QUAL fields as they lie in the file go
    to RawRecords.raw_bases, at seq_src; pin(nbytes) -> uint8 array: where raw_bases goes (pinned
    memory, which uploads asynchronously) instead of the pooled buffer."""
    s = _Sizes()
    lib.bsdc_bam_sizes_of(h, C.byref(s))
    n = s.n_rec
    specs = []

    def z(k, dt):
        specs.append((max(int(k), 1), np.dtype(dt)))
        return len(specs) - 1
    A = dict(flag=z(n, np.uint16), tid=z(n, np.int32), pos=z(n, np.int32), mapq=z(n, np.uint8),
             l_seq=z(n, np.int32), seq_off=z(n, np.int64), seq=z(0 if packed else s.n_bases, np.uint8),
             qual=z(0 if packed else s.n_bases, np.uint8),
             cig_off=z(n, np.int64), n_cig=z(n, np.int32), cigar=z(s.n_cigar, np.uint32),
             next_tid=z(n, np.int32), next_pos=z(n, np.int32), tlen=z(n, np.int32), name_id=z(n, np.int32),
             name_off=z(s.n_names + 1, np.int64), name_buf=z(s.name_bytes, np.uint8), mi_id=z(n, np.int32),
             mi_strand=z(n, np.int8), mi_off=z(s.n_mi + 1, np.int64), mi_buf=z(s.mi_bytes, np.uint8),
             mc_off=z(n, np.int64), mc_n=z(n, np.int32), mc_cigar=z(s.n_mc, np.uint32), la=z(n, np.int32),
             rd=z(n, np.int32), aux_off=z(n + 1, np.int64), aux=z(s.aux_bytes, np.uint8),
             header=z(s.header_bytes, np.uint8), ref_len=z(s.n_ref, np.int64),
             ref_name_off=z(s.n_ref + 1, np.int64), ref_name_buf=z(s.ref_name_bytes, np.uint8))
    n_raw = int(s.n_bases + (s.n_bases + n) // 2 + 8)  # (bsdc_bam_arrays.raw_bases' bound, + slack)
    if packed:
        A["seq_src"] = z(n + 1, np.int64)
        if pin is None:
            A["raw_bases"] = z(n_raw, np.uint8)
    buf = None
    if pool is None:
        arrs = [np.zeros(k, dt) for k, dt in specs]
    else:
        sizes = [(k * dt.itemsize + 63) & ~63 for k, dt in specs]
        buf = pool.take(sum(sizes))
        arrs, o = [], 0
        for (k, dt), nb in zip(specs, sizes):
            arrs.append(buf[o:o + k * dt.itemsize].view(dt))
            o += nb
    A = {key: arrs[i] for key, i in A.items()}
    if packed and pin is not None:
        A["raw_bases"] = pin(n_raw)
    a = _Arrays(**{k: _ptr(v) for k, v in A.items()})
    if lib.bsdc_bam_copy(h, C.byref(a)) != 0:
        raise OSError("%s: %s" % (what, lib.bsdc_io_last_error().decode()))
    names_tab = StringTable(A["ref_name_buf"][:s.ref_name_bytes], A["ref_name_off"][:s.n_ref + 1], as_str=True)
    header = BamHeader(A["header"][:s.header_bytes].tobytes().decode(errors="replace"),
                       [names_tab[i] for i in range(s.n_ref)], A["ref_len"][:s.n_ref].copy())
    raw = R.RawRecords(
        flag=A["flag"][:n], tid=A["tid"][:n], pos=A["pos"][:n], mapq=A["mapq"][:n], l_seq=A["l_seq"][:n],
        seq_off=A["seq_off"][:n], seq=None if packed else A["seq"][:s.n_bases],
        qual=None if packed else A["qual"][:s.n_bases], cig_off=A["cig_off"][:n],
        n_cig=A["n_cig"][:n], cigar=A["cigar"][:s.n_cigar], next_tid=A["next_tid"][:n], next_pos=A["next_pos"][:n],
        tlen=A["tlen"][:n], name_id=A["name_id"][:n],
        names=StringTable(A["name_buf"][:s.name_bytes], A["name_off"][:s.n_names + 1]),
        mi_id=A["mi_id"][:n], mi_strand=A["mi_strand"][:n],
        mi_names=StringTable(A["mi_buf"][:s.mi_bytes], A["mi_off"][:s.n_mi + 1], as_str=True),
        mc_off=A["mc_off"][:n], mc_n=A["mc_n"][:n], mc_cigar=A["mc_cigar"][:s.n_mc],
        aux=StringTable(A["aux"][:s.aux_bytes], A["aux_off"][:n + 1]), la_tag=A["la"][:n], rd_tag=A["rd"][:n])
    if packed:
        raw.seq_src = A["seq_src"][:n + 1]
        raw.raw_bases = A["raw_bases"][:int(raw.seq_src[n])]
    return header, raw, buf


def read_bam(path: str, threads: int = 0):
    """BAM file -> (BamHeader, records.RawRecords) with MI / MC / LA / RD decoded and the other
    aux bytes kept (``raw.aux`` is a StringTable of per-record aux blocks)."""
    lib = _load()
    h = _P()
    rc = lib.bsdc_bam_read(path.encode(), int(threads), C.byref(h))
    if rc != 0:
        raise OSError("%s: %s" % (path, lib.bsdc_io_last_error().decode()))
    try:
        return _decode(lib, h, path)[:2]
    finally:
        lib.bsdc_bam_free(h)


DEFAULT_CHUNK_BYTES = 64 << 20  # uncompressed record bytes per stream chunk (about 0.23M records)
DEFAULT_SLACK = 10_000           # positions: > any template's span (fragment + clips)
# a template whose mate lies further than this (or on another contig, unmapped or absent) is
# deferred: it leaves the stream for the spill, whose families are spliced in at their keys
# (bsdc_bam_stream_set_defer); half the slack, so that no rank window misses a near template's end
DEFAULT_DEFER_SPAN = DEFAULT_SLACK // 2
DEFER_MARGIN = 12  # kDeferMargin (csrc/bsdc_io.cpp): 3 x kKeyDelta


def read_bam_header(path: str) -> BamHeader:
    """The header of a BAM (its first BGZF blocks only)."""
    lib = _load()
    st = _P()
    if lib.bsdc_bam_stream_open(path.encode(), 1, 1 << 20, C.byref(st)) != 0:
        raise OSError("%s: %s" % (path, lib.bsdc_io_last_error().decode()))
    try:
        h = _P()
        lib.bsdc_bam_stream_header(st, C.byref(h))
        try:
            return _decode(lib, h, path)[0]
        finally:
            lib.bsdc_bam_free(h)
    finally:
        lib.bsdc_bam_stream_close(st)


class StreamChunk:
    """A chunk cut from a BAM stream but not yet decoded (bsdc_bam_stream_next_raw).  decode()
    parses it and copies it out (any thread: the stream meanwhile cuts the next chunk); discard()
    drops it.  Either returns its buffer to the stream; exactly one of them must be called."""

    def __init__(self, lib, st, h, path: str):
        self._lib, self._st, self._h, self._path = lib, st, h, path
        self.keys = False      # decode() also fills RawRecords.tc_key (bsdc_bam_rec_keys)
        self.splices = None    # int64 [k, 2]: deferred keys to cut this chunk's output before
        self.spill = b""       # spill entries (bsdc_bam_stream_spill) since the chunk before
        self.pool_buf = None   # decode(pool=...): the pooled buffer of the records, to give back

    def decode(self, threads: int = 0, timing: Optional[dict] = None, pool: Optional[BufferPool] = None,
               packed: bool = False, pin=None):
        """-> (BamHeader, RawRecords); `timing`: seconds added under "parse" (records, tags,
        interning) and "copy" (the arrays copied out); `pool`, `packed`, `pin`: see _decode."""
        import time
        lib, h = self._lib, self._h
        self._h = None
        try:
            t0 = time.perf_counter()
            if lib.bsdc_bam_parse(h, int(threads)) != 0:
                raise OSError("%s: %s" % (self._path, lib.bsdc_io_last_error().decode()))
            t1 = time.perf_counter()
            *out, self.pool_buf = _decode(lib, h, self._path, pool, packed, pin)
            if self.keys:  # the records' coarse TemplateCoordinate keys (splicing deferred families)
                kk = np.zeros(2 * max(out[1].n, 1), np.int64)
                if lib.bsdc_bam_rec_keys(h, _ptr(kk)) != 0:
                    raise OSError("%s: %s" % (self._path, lib.bsdc_io_last_error().decode()))
                out[1].tc_key = kk[:2 * out[1].n].reshape(-1, 2)
            if timing is not None:
                timing["parse"] = timing.get("parse", 0.0) + t1 - t0
                timing["copy"] = timing.get("copy", 0.0) + time.perf_counter() - t1
            return tuple(out)
        finally:
            lib.bsdc_bam_stream_recycle(self._st, h)

    def discard(self):
        if self._h is not None:
            h, self._h = self._h, None
            self._lib.bsdc_bam_stream_recycle(self._st, h)


KEY_GUARD = 16  # positions of key gap on each side of a rank boundary (> 2 x kKeyDelta of the tools' jitter)


def find_cut(path: str, start: int, threads: int = 0, min_span: Optional[int] = None, slack: int = DEFAULT_SLACK,
             guard: int = KEY_GUARD, max_bytes: int = 256 << 20):
    """A rank boundary of a coordinate-sorted BAM after file offset `start` (bsdc_bam_find_cut), or
    None: a dict with `key` (the boundary X, 2 ints), `coord` (contig << 32 | x), `start` (block,
    offset) of the first record at or past x - slack, `end` the same at or past x + slack, and
    `slack`."""
    lib = _load()
    out = np.zeros(8, np.int64)
    ms = 2 * slack if min_span is None else min_span
    if lib.bsdc_bam_find_cut(path.encode(), int(threads), int(start), int(ms), int(slack), int(guard), int(max_bytes),
                             _ptr(out)) != 0:
        raise OSError("%s: %s" % (path, lib.bsdc_io_last_error().decode()))
    if not out[7]:
        return None
    return {"start": (int(out[0]), int(out[1])), "end": (int(out[2]), int(out[3])), "key": (int(out[4]), int(out[5])),
            "coord": int(out[6]), "slack": int(slack)}


OWN_STOP_FOREIGN = 1  # include/bsdc_io.h BSDC_OWN_*


def _stream_spill(lib, st) -> bytes:
    """The stream's spill entries since the last call (bsdc_bam_stream_spill: per record an int64
    coordinate, an int64 file sequence number, the block_size-prefixed record)."""
    n = int(lib.bsdc_bam_stream_spill(st, None))
    if n == 0:
        return b""
    buf = np.empty(n, np.uint8)
    lib.bsdc_bam_stream_spill(st, _ptr(buf))
    return buf.tobytes()


def _stream_splices(lib, st) -> np.ndarray:
    """The deferred keys the last chunk reported (bsdc_bam_stream_splices) -> int64 [k, 2]."""
    n = int(lib.bsdc_bam_stream_splices(st, None))
    out = np.zeros((max(n, 1), 2), np.int64)
    if n:
        lib.bsdc_bam_stream_splices(st, _ptr(out))
    return out[:n]


def spill_sorted_records(data: bytes):
    """Spill entries (_stream_spill, possibly several streams' concatenated) -> (their records in
    file order -- sorted by (coordinate, sequence), the stable order of the input for equal pairs
    (bsdc_spill_sort) --, their count)."""
    if not data:
        return b"", 0
    lib = _load()
    a = np.frombuffer(data, np.uint8)
    cnt = np.zeros(1, np.int64)
    n = int(lib.bsdc_spill_sort(_ptr(a), a.shape[0], None, _ptr(cnt)))
    if n < 0:
        raise ValueError("spill: %s" % lib.bsdc_io_last_error().decode())
    out = np.empty(max(n, 1), np.uint8)
    lib.bsdc_spill_sort(_ptr(a), a.shape[0], _ptr(out), None)
    return out[:n].tobytes(), int(cnt[0])


def stream_chunks(path: str, threads: int = 0, chunk_bytes: int = DEFAULT_CHUNK_BYTES, slack: int = DEFAULT_SLACK,
                  read_size: int = 8 << 20, runs: bool = False, rng=None, stats: Optional[dict] = None, owner=None,
                  defer: int = 0, keys: bool = False, inflater=None):
    """The chunks of a coordinate-sorted BAM in bounded memory, undecoded (StreamChunk): cut where no
    template or MI family straddles two chunks (include/bsdc_io.h, bsdc_bam_stream_next_raw).  The
    stream itself is freed once it is exhausted and every chunk has been decoded or discarded.
    runs: a GroupReadsByUmi-ordered BAM (step 1's input) cut between runs of one MI value instead
    (bsdc_bam_stream_next_runs; any record order, no `slack`).  rng: (start block, offset in it,
    end block, offset in it) -- the records of that range only (start block -1: from the first
    record, end block -1: to the end; bsdc_bam_stream_open_range); `stats` then receives the range
    statistics (bsdc_bam_stream_range_stats: n, c0, dropped, foreign) once the stream is exhausted.
    owner: (rank, boundaries[, flags]) -- keep the records whose key lies in the rank's interval
    between the boundaries (find_cut dicts; bsdc_bam_stream_set_owner); flags (OWN_*):
    OWN_STOP_FOREIGN -- a foreign record raises OSError("... foreign record ...").
    defer: the span past which a template is deferred (bsdc_bam_stream_set_defer; 0 = off): each
    chunk then carries its `spill` entries and its `splices` (the deferred keys its output is cut
    before), and its records decode with their keys (RawRecords.tc_key); once exhausted, `stats`
    receives the rest as "spill_tail" and "splices_tail".  keys: the records decode with their keys
    in any case.  inflater: the blocks' inflate goes to it (bsdc_bam_stream_set_inflater): a
    GpuInflate, or any object whose `callback` is an INFLATE_FN (kept alive here for the stream's
    lifetime); the chunks are the same bytes."""
    lib = _load()
    st = _P()
    hook = None if inflater is None else inflater.callback  # (referenced until the stream is closed)
    if rng is None:
        rc = lib.bsdc_bam_stream_open(path.encode(), int(threads), int(read_size), C.byref(st))
    else:
        rc = lib.bsdc_bam_stream_open_range(path.encode(), int(threads), int(read_size), *[int(x) for x in rng],
                                            C.byref(st))
    if rc != 0:
        raise OSError("%s: %s" % (path, lib.bsdc_io_last_error().decode()))
    try:
        if hook is not None and lib.bsdc_bam_stream_set_inflater(st, hook, None) != 0:
            raise OSError("%s: %s" % (path, lib.bsdc_io_last_error().decode()))
        if owner is not None:
            rank, cuts = owner[:2]
            flags = int(owner[2]) if len(owner) > 2 else 0  # OWN_* (True: OWN_STOP_FOREIGN)
            bd = np.array([[c["key"][0], c["key"][1], c["coord"]] for c in cuts], np.int64).reshape(-1)
            wsl = min(c["slack"] for c in cuts) if cuts else 0  # (the windows' own margin)
            if lib.bsdc_bam_stream_set_owner(st, int(rank), _ptr(bd) if len(bd) else None, len(cuts), int(wsl),
                                             flags) != 0:
                raise OSError("%s: %s" % (path, lib.bsdc_io_last_error().decode()))
        if defer and lib.bsdc_bam_stream_set_defer(st, int(defer)) != 0:
            raise OSError("%s: %s" % (path, lib.bsdc_io_last_error().decode()))
        while True:
            h = _P()
            if runs:
                rc = lib.bsdc_bam_stream_next_runs(st, int(chunk_bytes), C.byref(h))
            else:
                rc = lib.bsdc_bam_stream_next_raw(st, int(chunk_bytes), int(slack), C.byref(h))
            if rc != 0:
                raise OSError("%s: %s" % (path, lib.bsdc_io_last_error().decode()))
            if not h:
                if stats is not None:
                    v = np.zeros(7, np.int64)
                    lib.bsdc_bam_stream_range_stats(st, _ptr(v))
                    stats.update(n=int(v[0]), c0=int(v[1]), dropped=int(v[2]), foreign=int(v[3]), spilled=int(v[4]),
                                 deferred=int(v[5]), peak_buffered=int(v[6]), spill_tail=_stream_spill(lib, st),
                                 splices_tail=_stream_splices(lib, st))
                return
            ch = StreamChunk(lib, st, h, path)
            ch.keys = bool(defer) or keys
            if defer:
                ch.spill = _stream_spill(lib, st)
                ch.splices = _stream_splices(lib, st)
            yield ch
    finally:
        lib.bsdc_bam_stream_close(st)


def stream_bam(path: str, threads: int = 0, chunk_bytes: int = DEFAULT_CHUNK_BYTES, slack: int = DEFAULT_SLACK,
               read_size: int = 8 << 20, inflater=None):
    """Chunks of a coordinate-sorted BAM in bounded memory: yields (BamHeader, RawRecords) per chunk,
    cut where no template or MI family straddles two chunks (include/bsdc_io.h,
    bsdc_bam_stream_next); names and MI ids are chunk-local.  inflater: as stream_chunks'."""
    for c in stream_chunks(path, threads, chunk_bytes, slack, read_size, inflater=inflater):
        yield c.decode(threads)


def _aux_table(raw: R.RawRecords) -> StringTable:
    if isinstance(raw.aux, StringTable):
        return raw.aux
    if raw.aux is None:
        return StringTable(np.zeros(0, np.uint8), np.zeros(raw.n + 1, np.int64))
    return StringTable.from_list(list(raw.aux))


@dataclass
class OutRecordsBam:
    """Records to write, structure-of-arrays (the bsdc_bam_records layout)."""

    flag: np.ndarray
    tid: np.ndarray
    pos: np.ndarray
    mapq: np.ndarray
    next_tid: np.ndarray
    next_pos: np.ndarray
    tlen: np.ndarray
    names: StringTable
    cig_off: np.ndarray     # [n + 1]
    cigar: np.ndarray
    seq_off: np.ndarray     # [n + 1]
    seq: np.ndarray         # nt16 codes
    qual: np.ndarray
    aux: StringTable
    aux2: Optional[StringTable] = None  # more aux bytes written after aux (the consensus tags)

    @property
    def n(self) -> int:
        return int(self.flag.shape[0])


def _ascii_int(x: np.ndarray):
    """Non-negative ints -> their decimal ASCII, packed: (buf, off)."""
    x = np.asarray(x, np.int64)
    d = np.ones_like(x)
    for k in range(1, 19):
        d += x >= 10 ** k
    off = np.zeros(x.shape[0] + 1, np.int64)
    off[1:] = np.cumsum(d)
    pos = np.arange(int(off[-1]), dtype=np.int64)
    rec = np.repeat(np.arange(x.shape[0]), d)
    p = pos - off[rec]                       # digit index from the left
    buf = (48 + (x[rec] // (10 ** (d[rec] - 1 - p))) % 10).astype(np.uint8)
    return buf, off


def _concat_fields(parts, n):
    """Per-record byte fields (each (buf, off) or a constant bytes) -> one packed StringTable
    (libbsdc_io bsdc_table_concat: parallel copies, no per-byte index arrays)."""
    lib = _load()
    k = len(parts)
    offs = (_P * k)()
    bufs = (_P * k)()
    clen = np.zeros(k, np.int64)
    keep = []
    for j, p in enumerate(parts):
        if isinstance(p, bytes):
            b = np.frombuffer(p if p else b"\0", np.uint8).copy()
            keep.append(b)
            offs[j], bufs[j], clen[j] = None, _ptr(b), len(p)
        else:
            pb = np.ascontiguousarray(p[0], np.uint8)
            po = np.ascontiguousarray(p[1], np.int64)
            if pb.size == 0:
                pb = np.zeros(1, np.uint8)
            keep += [pb, po]
            offs[j], bufs[j] = _ptr(po), _ptr(pb)
    off = np.zeros(n + 1, np.int64)
    total = lib.bsdc_table_concat(int(n), k, offs, bufs, _ptr(clen), _ptr(off), None, 0)
    buf = np.empty(max(int(total), 1), np.uint8)
    lib.bsdc_table_concat(int(n), k, offs, bufs, _ptr(clen), _ptr(off), _ptr(buf), 0)
    return StringTable(buf[:int(total)], off)


def table_ranks(t: StringTable) -> np.ndarray:
    """Byte-order rank of every entry of a packed table (equal entries share a rank; libbsdc_io)."""
    lib = _load()
    n = len(t)
    rank = np.zeros(max(n, 1), np.int64)
    if n:
        buf = np.ascontiguousarray(t.buf, np.uint8) if t.buf.size else np.zeros(1, np.uint8)
        lib.bsdc_table_rank(n, _ptr(np.ascontiguousarray(t.off, np.int64)), _ptr(buf), _ptr(rank), 0)
    return rank[:n]


def unpack_nibbles(packed: np.ndarray, threads: int = 0) -> np.ndarray:
    """Packed nt16 bytes (high nibble first) -> one code per byte, same leading shape, last axis x2
    (libbsdc_io, parallel)."""
    a = np.ascontiguousarray(packed, np.uint8)
    out = np.empty(a.shape[:-1] + (2 * a.shape[-1],), np.uint8)
    if a.size:
        _load().bsdc_unpack_nibbles(int(a.size), _ptr(a), _ptr(out), int(threads))
    return out


def _take_table(t: StringTable, idx: np.ndarray) -> StringTable:
    """Entries idx[0], idx[1], ... of a packed table (libbsdc_io bsdc_table_take)."""
    lib = _load()
    idx = np.ascontiguousarray(idx, np.int64)
    n = int(idx.shape[0])
    src_off = np.ascontiguousarray(t.off, np.int64)
    src = np.ascontiguousarray(t.buf, np.uint8) if t.buf.size else np.zeros(1, np.uint8)
    off = np.zeros(n + 1, np.int64)
    total = lib.bsdc_table_take(n, _ptr(idx), _ptr(src_off), _ptr(src), _ptr(off), None, 0)
    buf = np.empty(max(int(total), 1), np.uint8)
    lib.bsdc_table_take(n, _ptr(idx), _ptr(src_off), _ptr(src), _ptr(off), _ptr(buf), 0)
    return StringTable(buf[:int(total)], off)


def take_records(recs: "OutRecordsBam", idx: np.ndarray) -> "OutRecordsBam":
    """Records idx[0], idx[1], ... of an OutRecordsBam (a contiguous range for the streaming writer)."""
    idx = np.asarray(idx, np.int64)

    def ragged(off, vals):
        ln = (off[1:] - off[:-1])[idx]
        o = np.zeros(idx.shape[0] + 1, np.int64)
        o[1:] = np.cumsum(ln)
        src = np.repeat(off[:-1][idx] - o[:-1], ln) + np.arange(int(o[-1]), dtype=np.int64)
        return o, vals[src]
    co, cig = ragged(recs.cig_off, recs.cigar)
    so, seq = ragged(recs.seq_off, recs.seq)
    _, qual = ragged(recs.seq_off, recs.qual)
    return OutRecordsBam(flag=recs.flag[idx], tid=recs.tid[idx], pos=recs.pos[idx], mapq=recs.mapq[idx],
                         next_tid=recs.next_tid[idx], next_pos=recs.next_pos[idx], tlen=recs.tlen[idx],
                         names=_take_table(recs.names, idx), cig_off=co, cigar=cig, seq_off=so, seq=seq, qual=qual,
                         aux=_take_table(recs.aux, idx),
                         aux2=_take_table(recs.aux2, idx) if recs.aux2 is not None else None)


def _synthetic_fields(raw: R.RawRecords):
    """Vectorised MI / MC aux and QNAMEs of a synthetic stream (decimal lazy names, one-op MC)."""
    n = raw.n
    mi_pre = getattr(raw.mi_names, "prefix", None)
    nm_pre = getattr(raw.names, "prefix", None)
    if mi_pre is None or nm_pre is None or (raw.mc_n > 1).any() or (raw.mi_id < 0).any() or (raw.mi_strand < 0).any():
        return None
    mi = _ascii_int(raw.mi_id)
    sfx = (np.frombuffer(b"AB", np.uint8)[raw.mi_strand.astype(np.int64)], np.arange(n + 1, dtype=np.int64))
    has_mc = raw.mc_off >= 0
    mcv = raw.mc_cigar[np.where(has_mc, raw.mc_off, 0)] if raw.mc_cigar.shape[0] else np.zeros(n, np.uint32)
    if not has_mc.all():
        return None
    mcl = _ascii_int(mcv >> 4)
    mco = (np.frombuffer(R.CIGAR_OPS.encode(), np.uint8)[(mcv & 0xF).astype(np.int64)], np.arange(n + 1, dtype=np.int64))
    aux = _concat_fields([b"MIZ" + mi_pre.encode(), mi, b"/", sfx, b"\0MCZ", mcl, mco, b"\0"], n)
    names = _concat_fields([nm_pre.encode(), _ascii_int(raw.name_id)], n)
    return aux, names


def records_to_bam(raw: R.RawRecords) -> OutRecordsBam:
    """A RawRecords stream as records to write: its own aux bytes, or for synthetic streams
    (no aux) the MI (with the /A|/B strand) and MC tags rebuilt from the decoded fields."""
    n = raw.n
    syn = _synthetic_fields(raw) if raw.aux is None and n else None
    if raw.aux is not None:
        aux = _aux_table(raw)
    elif syn is not None:
        aux = syn[0]
    else:
        parts = []
        for k in range(n):
            t = []
            if raw.mi_id[k] >= 0:
                sfx = {0: "/A", 1: "/B"}.get(int(raw.mi_strand[k]), "")
                t.append(("MI", "Z", "%s%s" % (raw.mi_names[int(raw.mi_id[k])], sfx)))
            if raw.mc_off[k] >= 0:
                mc = raw.mc_cigar[raw.mc_off[k]:raw.mc_off[k] + raw.mc_n[k]]
                t.append(("MC", "Z", R.cigar_string([int(x) for x in mc])))
            parts.append(R.encode_aux(t))
        aux = StringTable.from_list(parts)
    cig_off = np.zeros(n + 1, np.int64)
    cig_off[:n] = raw.cig_off
    cig_off[n] = int(raw.cig_off[-1] + raw.n_cig[-1]) if n else 0
    seq_off = np.zeros(n + 1, np.int64)
    seq_off[:n] = raw.seq_off
    seq_off[n] = int(raw.seq_off[-1] + raw.l_seq[-1]) if n else 0
    if syn is not None:
        tab = syn[1]
    else:
        names = raw.names
        tab = StringTable.from_list([names[int(i)] for i in raw.name_id.astype(np.int64)])
    return OutRecordsBam(raw.flag, raw.tid, raw.pos, raw.mapq, raw.next_tid, raw.next_pos, raw.tlen, tab, cig_off,
                         raw.cigar, seq_off, raw.seq, raw.qual, aux)


def _c_array(keep: list, x, dt):
    """x as a contiguous dt array (kept alive in `keep`; one element if empty) -> its pointer."""
    a = np.ascontiguousarray(x, dtype=dt)
    if a.size == 0:
        a = np.zeros(1, dt)
    keep.append(a)
    return _ptr(a)


def _header_args(header: BamHeader, keep: list) -> tuple:
    """bsdc_bam_write's / bsdc_bam_writer_open's header arguments: text, its length, n_ref, the
    reference names' offsets and bytes, the reference lengths."""
    rn = StringTable.from_list([x.encode() for x in header.ref_names])
    text = header.text.encode()
    return (text, len(text), len(header.ref_names), _c_array(keep, rn.off, np.int64), _c_array(keep, rn.buf, np.uint8),
            _c_array(keep, np.asarray(header.ref_lens, np.int64), np.int64))


def _records_struct(recs: OutRecordsBam, keep: list) -> _Records:
    def c(x, dt):
        return _c_array(keep, x, dt)
    return _Records(recs.n, c(recs.flag, np.uint16), c(recs.tid, np.int32), c(recs.pos, np.int32),
                    c(recs.mapq, np.uint8), c(recs.next_tid, np.int32), c(recs.next_pos, np.int32),
                    c(recs.tlen, np.int32), c(recs.names.off, np.int64), c(recs.names.buf, np.uint8),
                    c(recs.cig_off, np.int64), c(recs.cigar, np.uint32), c(recs.seq_off, np.int64),
                    c(recs.seq, np.uint8), c(recs.qual, np.uint8), c(recs.aux.off, np.int64),
                    c(recs.aux.buf, np.uint8),
                    c(recs.aux2.off, np.int64) if recs.aux2 is not None else None,
                    c(recs.aux2.buf, np.uint8) if recs.aux2 is not None else None)


def family_image(src_off, length, dst_off, seq, qual, n_slots: int, packed: np.ndarray, qual_out: np.ndarray,
                 threads: int = 0):
    """batch.build_family_batch's image: record r's bases / quals at src_off[r] -> nibble / byte
    dst_off[r] + 1 of `packed` / `qual_out` (zeroed by the caller; libbsdc_io)."""
    lib = _load()
    so = np.ascontiguousarray(src_off, np.int64)
    ln = np.ascontiguousarray(length, np.int64)
    do = np.ascontiguousarray(dst_off, np.int64)
    sq = np.ascontiguousarray(seq, np.uint8)
    ql = np.ascontiguousarray(qual, np.uint8)
    if packed.shape[0] * 2 < n_slots or qual_out.shape[0] < n_slots or not (packed.flags.c_contiguous and
                                                                           qual_out.flags.c_contiguous):
        raise ValueError("family image outputs too small")
    if so.shape[0] and (int((so + ln).max()) > sq.shape[0] or int((so + ln).max()) > ql.shape[0]):
        raise ValueError("family image: record past the end of seq / qual")
    rc = lib.bsdc_family_image(so.shape[0], _ptr(so), _ptr(ln), _ptr(do), _ptr(sq), _ptr(ql), int(n_slots),
                               _ptr(packed), _ptr(qual_out), int(threads))
    if rc != 0:
        raise ValueError(lib.bsdc_io_last_error().decode())


def fastq_offsets(status: np.ndarray, length: np.ndarray, filt: Optional[np.ndarray], name_off: np.ndarray):
    """-> (off0, off1), int64 [F + 1] each: where family f's bytes start in the FASTQ text of file
    1 / file 2 that libbsdc's bsdc_fastq_format (or format_fastq here) writes for a batch --
    8 + name + 2 * length bytes per kept family (filter.kept's rule), none for the others;
    off[F] = the text's size.  name_off: the families' packed name table offsets [F + 1]."""
    F = int(status.shape[0])
    keep = (np.asarray(status) & 1) != 0
    if filt is not None:
        keep &= np.asarray(filt) == 0
    nl = np.diff(np.asarray(name_off, np.int64))
    out = []
    for d in range(2):
        off = np.zeros(F + 1, np.int64)
        np.cumsum(np.where(keep, 8 + nl + 2 * np.asarray(length, np.int64).reshape(F, 2)[:, d], 0), out=off[1:])
        out.append(off)
    return out[0], out[1]


def family_names(fam_mi: np.ndarray, mi_names, prefix: str) -> StringTable:
    """The read name "prefix:MI" of every family (duplex_records' names), a packed table."""
    ids = np.maximum(np.asarray(fam_mi, np.int64), 0)
    F = int(ids.shape[0])
    if isinstance(mi_names, StringTable):
        mt = _take_table(mi_names, ids)
    else:
        uniq, inv = np.unique(ids, return_inverse=True)
        mt = _take_table(StringTable.from_list([(lambda m: m if isinstance(m, bytes) else m.encode())(
            mi_names[int(i)]) for i in uniq]), inv) if F else StringTable.from_list([])
    return _concat_fields([prefix.encode() + b":", (mt.buf, mt.off)], F)


def write_fastq(path1: str, path2: str, recs: OutRecordsBam, level: int = 6, threads: int = 0):
    """Paired gzip FASTQ of `recs` as picard SamToFastq F=path1 F2=path2 writes it (the rule after
    step 5, main.snake.py:167-177): '@name/1' / '@name/2', SEQ, '+', QUAL+33 (libbsdc_io)."""
    lib = _load()
    keep = []
    r = _records_struct(recs, keep)
    rc = lib.bsdc_fastq_write(path1.encode(), path2.encode(), C.byref(r), int(level), int(threads))
    if rc != 0:
        raise ValueError("%s, %s: %s" % (path1, path2, lib.bsdc_io_last_error().decode()))


def write_bam(path: str, header: BamHeader, recs: OutRecordsBam, level: int = 6, threads: int = 0):
    lib = _load()
    keep = []
    r = _records_struct(recs, keep)
    rc = lib.bsdc_bam_write(path.encode(), *_header_args(header, keep), C.byref(r), int(level), int(threads))
    if rc != 0:
        raise OSError("%s: %s" % (path, lib.bsdc_io_last_error().decode()))


def read_fasta(path: str, header: BamHeader) -> R.Reference:
    """FASTA -> the packed reference in the BAM header's tid order (contigs the FASTA lacks are
    absent: tool 1 then converts against N, tools/1.convert_AG_to_CT.py:103-117)."""
    data = np.fromfile(path, dtype=np.uint8)
    starts = np.nonzero(data == ord(">"))[0]
    starts = starts[(starts == 0) | (data[np.maximum(starts - 1, 0)] == ord("\n"))]
    contigs = {}
    for i, s0 in enumerate(starts):
        e = int(starts[i + 1]) if i + 1 < len(starts) else data.shape[0]
        nl = s0 + int(np.argmax(data[s0:e] == ord("\n"))) if (data[s0:e] == ord("\n")).any() else e
        name = data[s0 + 1:nl].tobytes().decode().split()[0]
        body = data[nl:e]
        body = body[(body != ord("\n")) & (body != ord("\r"))]
        contigs[name] = body.tobytes()
    return R.Reference.from_contigs(header.ref_names, {k: v for k, v in contigs.items()}, keep_letters=False,
                                    header_lengths=list(header.ref_lens))


def read_name_prefix(header: BamHeader) -> str:
    """fgbio's default consensus read-name prefix (restated, parity unpinned): the input read
    groups' libraries (or IDs), distinct, sorted, joined by '|'."""
    ids = sorted({rg.get("LB", rg.get("ID", "")) for rg in header.read_groups()})
    return "|".join(ids)


def output_header(header: BamHeader) -> BamHeader:
    """fgbio's consensus header (restated): unsorted/query-grouped, the input's @SQ lines, one
    read group A carrying the input's sample and library when they are unique."""
    rgs = header.read_groups()
    rg = ["@RG", "ID:A"]
    for key in ("SM", "LB"):
        vals = sorted({g[key] for g in rgs if key in g})
        if len(vals) == 1:
            rg.append("%s:%s" % (key, vals[0]))
    lines = ["@HD\tVN:1.6\tSO:unsorted\tGO:query"]
    lines += [ln for ln in header.text.splitlines() if ln.startswith("@SQ")]
    lines += ["\t".join(rg), "@PG\tID:bsseqconsensusreads_amd\tPN:bsseqconsensusreads_amd\tCL:step5"]
    return BamHeader("\n".join(lines) + "\n", list(header.ref_names), np.asarray(header.ref_lens, np.int64))


def consensus_tags(cons, em: np.ndarray, molecular: bool = False, threads: int = 0,
                   pool: Optional["BufferPool"] = None) -> StringTable:
    """fgbio's consensus tags (aux bytes) of the output records R1, R2 of families `em`, from the
    single-strand reads in cons.ss (libbsdc_io bsdc_consensus_tags).  Duplex: a record's 'a'
    strand is its AB read (AB-R1 for R1, AB-R2 for R2), or the only strand present; 'b' its BA read
    when both are present.  Molecular: set 0 for R1, set 1 for R2.  With `pool`, the bytes land in
    a pooled buffer and the result is (table, that buffer, for the caller to give back): the tags
    are ≈1.8 KB a record, and fresh pages for them cost as much as writing them."""
    lib = _load()
    ss = cons.ss
    F = em.shape[0]
    n = 2 * F
    em2 = np.repeat(em.astype(np.int64), 2)
    end = np.tile(np.asarray([0, 1], np.int64), F)
    if molecular:
        row_a = 4 * em2 + end
        row_b = np.full(n, -1, np.int64)
    else:
        sa, sb = end, 3 - end                      # R1: sets 0 / 3, R2: sets 1 / 2
        la = ss["len"][em2, sa] > 0
        lb = ss["len"][em2, sb] > 0
        row_a = 4 * em2 + np.where(la, sa, sb)
        row_b = np.where(la & lb, 4 * em2 + sb, -1)
    out_len = np.ascontiguousarray(cons.length[em].reshape(-1), np.int32)
    stride = int(ss["base"].shape[2])
    c = lambda a, dt: np.ascontiguousarray(a, dt).reshape(-1)
    base, qual = c(ss["base"], np.uint8), c(ss["qual"], np.uint8)
    wide, wdepth, werr = ss.get("wide"), ss.get("wdepth"), ss.get("werr")
    if np.asarray(ss["depth"]).dtype != np.uint8:  # u16 statistics (oracle/): bytes + wide rows
        d16, e16 = np.asarray(ss["depth"]), np.asarray(ss["err"])
        big = (d16.reshape(d16.shape[0], -1).max(axis=1, initial=0) > 255) | \
              (e16.reshape(e16.shape[0], -1).max(axis=1, initial=0) > 255)
        wide = np.where(big, np.cumsum(big) - 1, -1).astype(np.int32)
        wdepth, werr = d16[big].astype(np.uint16), e16[big].astype(np.uint16)
        depth, err = c(np.minimum(d16, 255), np.uint8), c(np.minimum(e16, 255), np.uint8)
    else:
        depth, err = c(ss["depth"], np.uint8), c(ss["err"], np.uint8)
    has_wide = wide is not None and wdepth is not None and wdepth.shape[0] > 0
    if has_wide:
        wide = np.ascontiguousarray(wide, np.int32)
        wdepth, werr = c(wdepth[:, :, :stride], np.uint16), c(werr[:, :, :stride], np.uint16)
    row_a, row_b = np.ascontiguousarray(row_a), np.ascontiguousarray(row_b)
    off = np.zeros(n + 1, np.int64)
    args = (n, _ptr(row_a), _ptr(row_b), _ptr(out_len), 1 if molecular else 0, stride, _ptr(base), _ptr(qual),
            _ptr(depth), _ptr(err), _ptr(wide) if has_wide else None, _ptr(wdepth) if has_wide else None,
            _ptr(werr) if has_wide else None, _ptr(off))
    total = lib.bsdc_consensus_tags(*args, None, int(threads))
    buf = pool.take(max(int(total), 1)) if pool is not None else np.empty(max(int(total), 1), np.uint8)
    lib.bsdc_consensus_tags(*args, _ptr(buf), int(threads))
    tab = StringTable(buf[:int(total)], off)
    return tab if pool is None else (tab, buf)


def _mi_table(mi_names, mi_ids: np.ndarray):
    """The MI names of the ids as (buf, off) of a packed table."""
    mi_ids = np.asarray(mi_ids, np.int64)
    if isinstance(mi_names, StringTable):  # decoded BAM: a packed table already
        mt = _take_table(mi_names, mi_ids)
    else:
        uniq, inv = np.unique(mi_ids, return_inverse=True)
        mt = _take_table(StringTable.from_list([(lambda m: m if isinstance(m, bytes) else m.encode())(
            mi_names[int(i)]) for i in uniq]), inv)
    return mt.buf, mt.off


def family_aux(fam_rec_off, fam_src, fam_mi, raw: R.RawRecords, threads: int = 0,
               fams: Optional[np.ndarray] = None) -> StringTable:
    """The aux bytes both output records of a family carry -- RG:Z:A, MI:Z:<the family's MI>, and
    RX:Z:<the consensus UMI of its records' RX tags> where they have one (libbsdc_io
    bsdc_rx_consensus) -- as a packed table, one entry per family of `fams` (indices; default: every
    family, emitted or not, as Engine.bam_records wants them before the launch).  Families:
    fam_src[fam_rec_off[f]:fam_rec_off[f + 1]] are family f's input records, fam_mi[f] its MI id
    (pipeline.Consensus' fields, or a FamilyBatch's fam_off / src / fam_mi)."""
    lib = _load()
    aux = _aux_table(raw)
    fro = np.ascontiguousarray(fam_rec_off, np.int64)
    fsrc = np.ascontiguousarray(fam_src, np.int64)
    strand = np.ascontiguousarray(raw.mi_strand, np.int8)
    nf_all = int(fro.shape[0]) - 1
    em = np.arange(nf_all, dtype=np.int64) if fams is None else np.asarray(fams, np.int64)
    F = int(em.shape[0])
    # consensus UMI per family from its records' RX (libbsdc_io)
    width = lib.bsdc_rx_consensus(nf_all, _ptr(fro), _ptr(fsrc), _ptr(strand), _ptr(aux.off),
                                  _ptr(aux.buf if aux.buf.size else np.zeros(1, np.uint8)), None, None, int(threads))
    rx = np.zeros(max(nf_all * max(width, 1), 1), np.uint8)
    rx_len = np.zeros(max(nf_all, 1), np.int32)
    if width > 0:
        lib.bsdc_rx_consensus(nf_all, _ptr(fro), _ptr(fsrc), _ptr(strand), _ptr(aux.off), _ptr(aux.buf), _ptr(rx),
                              _ptr(rx_len), int(threads))
    mi = _mi_table(raw.mi_names, np.maximum(np.asarray(fam_mi, np.int64)[em], 0) if fams is None else
                   np.asarray(fam_mi, np.int64)[em])
    if width > 0:
        rl = rx_len[em].astype(np.int64)
        has = rl > 0
        rxb = rx.reshape(-1, width)[em] if F else np.zeros((0, max(width, 1)), np.uint8)
        rxv = (rxb[np.arange(width)[None, :] < rl[:, None]], np.concatenate([[0], np.cumsum(rl)]).astype(np.int64))
        tag = (np.repeat(np.frombuffer(b"RXZ", np.uint8)[None, :], F, 0)[has].reshape(-1),
               np.concatenate([[0], np.cumsum(np.where(has, 3, 0))]).astype(np.int64))
        nul = (np.zeros(int(has.sum()), np.uint8), np.concatenate([[0], np.cumsum(has)]).astype(np.int64))
        return _concat_fields([b"RGZA\0MIZ", mi, b"\0", tag, rxv, nul], F)
    return _concat_fields([b"RGZA\0MIZ", mi, b"\0"], F)


def duplex_records(cons, raw: R.RawRecords, prefix: str, threads: int = 0, molecular: bool = False,
                   pool: Optional["BufferPool"] = None) -> OutRecordsBam:
    """fgbio duplex output records for the emitted families of `cons`
    (pipeline.Consensus, family order): R1 then R2 per family; fgbio's consensus tags appended
    when cons.ss holds the single-strand reads (``molecular``: CallMolecularConsensusReads' set).
    `pool`: the tags' buffer comes from it (consensus_tags) and the result is (records, that buffer
    or None, for the caller to give back).  A filtered consensus (cons.filt) gives
    the kept families only, SEQ / QUAL masked; their tags are those of the unfiltered reads, as
    fgbio FilterConsensusReads leaves them."""
    lib = _load()
    em = np.nonzero(_filter.kept(cons))[0]
    F = em.shape[0]
    n = 2 * F
    mi = _mi_table(raw.mi_names, cons.fam_mi[em])
    fam_aux = family_aux(cons.fam_rec_off, cons.fam_src, cons.fam_mi, raw, threads, em)
    fam_names = _concat_fields([prefix.encode() + b":", mi], F)
    two = np.repeat(np.arange(F, dtype=np.int64), 2)
    names_t, auxs_t = _take_table(fam_names, two), _take_table(fam_aux, two)
    tg = tags_buf = None
    if getattr(cons, "ss", None) is not None:
        tg = consensus_tags(cons, em, molecular, threads, pool)
        if pool is not None:
            tg, tags_buf = tg
    L = np.ascontiguousarray(cons.length[em].reshape(-1), np.int32)  # R1, R2, R1, R2 ...
    seq_off = np.zeros(n + 1, np.int64)
    seq_off[1:] = np.cumsum(L)
    stride = cons.seq.shape[2]
    rows = np.ascontiguousarray(np.repeat(em.astype(np.int64), 2) * 2 + np.tile(np.asarray([0, 1], np.int64), F))
    total = int(seq_off[-1])
    seq = np.empty(max(total, 1), np.uint8)[:total]
    qual = np.empty(max(total, 1), np.uint8)[:total]
    for src, dst in ((cons.seq, seq), (cons.qual, qual)):  # the (family, end) rows, in record order
        src = np.ascontiguousarray(src, np.uint8)
        if n:
            lib.bsdc_rows_gather(n, _ptr(rows), _ptr(L), int(stride), _ptr(src), _ptr(seq_off), _ptr(dst), int(threads))
    recs = OutRecordsBam(
        flag=np.tile(np.asarray([77, 141], np.uint16), F), tid=np.full(n, -1, np.int32), pos=np.full(n, -1, np.int32),
        mapq=np.zeros(n, np.uint8), next_tid=np.full(n, -1, np.int32), next_pos=np.full(n, -1, np.int32),
        tlen=np.zeros(n, np.int32), names=names_t, cig_off=np.zeros(n + 1, np.int64),
        cigar=np.zeros(0, np.uint32), seq_off=seq_off, seq=seq, qual=qual, aux=auxs_t, aux2=tg)
    return recs if pool is None else (recs, tags_buf)


def consensus_sharded(eng, raw: R.RawRecords, tags: bool, batch_bases: Optional[int] = None, dist=None,
                      filter=None, metrics: bool = False, toolrec: Optional[str] = None):
    """pipeline.run_step5 over the ranks of `dist` (None = this process alone): every rank forms
    the same family plan, runs the batches shard.deal gives it on its own GPU, and rank 0 gets the
    consensus of all batches in plan order (shard.gather_in_order; other ranks get None).  A plan
    whose tool-2 extension partners straddle families runs on rank 0 alone (pipeline.run_step5's
    two-launch fallback)."""
    from . import pipeline, shard
    if dist is None or dist.get_world_size() == 1:
        mkw = {"metrics": True} if metrics else {}
        if toolrec is not None:
            mkw["toolrec"] = toolrec
        return pipeline.run_step5(eng, raw, tags=tags, batch_bases=batch_bases, filter=filter, **mkw)[0]
    if filter is not None:
        raise ValueError("the consensus filter is not supported with several ranks yet")
    if toolrec is not None:
        raise ValueError("the group-sorted BAM of the tool-stage records is not supported with several ranks yet")
    if metrics:
        raise ValueError("metrics is not supported with several ranks yet")
    rank, world = dist.get_rank(), dist.get_world_size()
    plan = pipeline.plan_families(raw, "full", eng.ref)
    if plan.split_ext:
        return pipeline.run_step5(eng, raw, tags=tags, batch_bases=batch_bases)[0] if rank == 0 else None
    ranges = pipeline.plan_ranges(plan, batch_bases)
    mine_idx = shard.deal(ranges, world, rank)
    parts = pipeline.run_ranges(eng, plan, [ranges[i] for i in mine_idx],
                                pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE, tags)
    got = shard.gather_in_order(dist, dict(zip(mine_idx, parts)), len(ranges))
    return pipeline.concat_consensus(got) if rank == 0 else None


def step5(in_bam: str, fasta: str, out_bam: Optional[str], engine=None, prefix: Optional[str] = None, threads: int = 0,
          level: int = 6, fastq: Optional[Tuple[str, str]] = None, tags: bool = True, batch_bases: Optional[int] = None,
          dist=None, filter=None, metrics: Optional[str] = None, metrics_cycles: int = 512,
          groupsort_bam: Optional[str] = None) -> dict:
    """Rules convert_Bstrain .. callduplex (main.snake.py:121-164) as one call on files; with
    `fastq`, also the following consensusduplex_to_fq rule (main.snake.py:167-177) straight from
    the consensus records (out_bam may then be None: no BAM round trip).  The stream runs as
    bounded device batches (batch_bases, pipeline.DEFAULT_BATCH_BASES); with `dist` the batches
    are shared by the ranks (one GPU each) and rank 0 writes the files.  filter (filter.FilterParams):
    fgbio FilterConsensusReads on the device between the vote and the records -- the outputs hold
    the kept templates, masked, and the info dict a `filter` entry (filter.summary).  metrics: the
    path of the run's metrics JSON, reduced on the device from every batch (one rank).
    groupsort_bam: the path of a BAM of the records after tool 1 and tool 2 in TemplateCoordinate
    order (rule groupsort_convert's file, main.snake.py:144-153), encoded by the host
    twin (bsdc_toolrec_host) from every batch's stage dump; one rank."""
    from .device import Engine
    header, raw = read_bam(in_bam, threads)
    ref = read_fasta(fasta, header)
    own = engine is None
    eng = Engine(0) if own else engine
    try:
        eng.load_reference(ref)
        if metrics is not None:
            eng.metrics_begin(metrics_cycles)
        mkw = {"metrics": True} if metrics is not None else {}
        if groupsort_bam is not None:
            mkw["toolrec"] = "host"
        cons = consensus_sharded(eng, raw, tags and out_bam is not None, batch_bases, dist, filter, **mkw)
        if metrics is not None:
            _write_metrics(eng, metrics, metrics_cycles, False, filter)
    finally:
        if own:
            eng.close()
    if cons is None:  # not rank 0
        return {"records_in": raw.n}
    info = _write_consensus(cons, raw, raw.n, header, prefix, out_bam, fastq, level, threads, False, filter)
    if groupsort_bam is not None:
        info["groupsort_bam"] = _write_groupsort(groupsort_bam, header, cons.toolrec, level, threads)
    return info


def _write_groupsort(path: str, header: BamHeader, pieces, level: int, threads: int) -> dict:
    """The batches' tool-stage records (pipeline.ToolrecPiece of host bytes, in order) as the
    group-sorted BAM through the ordinary host writer -> the info entry."""
    from . import bgzf, toolrec
    w = bgzf.BamWriter(path, toolrec.header(header), level)
    n = raw_bytes = 0
    try:
        for x in pieces:
            w.add_raw(x.host(0, x.fams), threads)
            n += x.n_rec
            raw_bytes += int(x.foff[-1])
    finally:
        w.close(threads)
    return {"records": n, "raw_bytes": raw_bytes, "compressed_bytes": os.path.getsize(path)}


def _write_metrics(eng, path: str, cycles: int, molecular: bool, flt):
    from . import metrics as _metrics
    _metrics.write(path, eng.metrics_fetch(), cycles, _metrics.run_params(eng.params, molecular, flt))


def _write_consensus(cons, raw, n_in: int, header, prefix, out_bam, fastq, level, threads, molecular, flt) -> dict:
    """The whole-file steps' tail: the consensus' records -> the BAM and / or the FASTQ pair ->
    the info dict (with the `filter` entry of a filtered consensus)."""
    recs = duplex_records(cons, raw, read_name_prefix(header) if prefix is None else prefix, threads,
                          molecular=molecular)
    if out_bam is not None:
        write_bam(out_bam, output_header(header), recs, level, threads)
    if fastq is not None:
        write_fastq(fastq[0], fastq[1], recs, level, threads)
    info = {"records_in": n_in, "families": int(cons.status.shape[0]),
            "families_emitted": int(((cons.status & 1) != 0).sum()), "records_out": recs.n}
    if flt is not None:
        info["filter"] = _filter.summary(cons)
    return info


def molecular(in_bam: str, out_bam: Optional[str], engine=None, prefix: Optional[str] = None, threads: int = 0,
              level: int = 6, fastq: Optional[Tuple[str, str]] = None, tags: bool = True,
              min_consensus_base_quality: int = 0, filter=None, metrics: Optional[str] = None,
              metrics_cycles: int = 512) -> dict:
    """Rule call_consensus_reads_molecular (main.snake.py:46-55, fgbio CallMolecularConsensusReads)
    on files; with `fastq`, also consensus_to_fq_unfiltered (main.snake.py:58-67) -- or, with
    `filter` (as step5's, the molecular rules), the filtered pair of consensus_to_fq (:70-80).
    metrics: as step5's."""
    from . import pipeline
    from .device import Engine
    header, raw = read_bam(in_bam, threads)
    own = engine is None
    eng = Engine(0) if own else engine
    try:
        if metrics is not None:
            eng.metrics_begin(metrics_cycles)
        cons, rm = pipeline.run_molecular(eng, raw, tags=tags and out_bam is not None,
                                          min_consensus_base_quality=min_consensus_base_quality, filter=filter,
                                          **({"metrics": True} if metrics is not None else {}))
        if metrics is not None:
            with eng.flags(min_consensus_base_quality=min_consensus_base_quality):  # (the flags the run used)
                _write_metrics(eng, metrics, metrics_cycles, True, filter)
    finally:
        if own:
            eng.close()
    return _write_consensus(cons, rm, raw.n, header, prefix, out_bam, fastq, level, threads, True, filter)


def __getattr__(name):
    """The streaming steps live in stream.py, the GPU BGZF codecs and the streaming writers in
    bgzf.py, cli zipper's driver in zipper.py, cli group's in group.py (all import this module); they stay importable from here."""
    home = {"step5_stream": "stream", "molecular_stream": "stream", "GpuBgzf": "bgzf", "GpuInflate": "bgzf",
            "_BgzfWriter": "bgzf", "BamWriter": "bgzf", "FastqWriter": "bgzf", "close_quietly": "bgzf",
            "zipper": "zipper", "group": "group"}.get(name)
    if home is None:
        raise AttributeError("module %r has no attribute %r" % (__name__, name))
    import importlib
    return getattr(importlib.import_module("." + home, __package__), name)

"""The records after tool 1 and tool 2 as a group-sorted BAM (cli step5 --groupsort-bam; DESIGN.md
3.10): the file rule groupsort_convert leaves for fgbio CallDuplexConsensusReads
(main.snake.py:144-153,163), made of the stage dump of a BSDC_MODE_DUMP run and the input records'
own fields.

* ``tables``  -- a batch's per-record table (bsdc_toolrec_rec) with the names, the clip-stripped
  cigar ops and the aux bytes it points into; the RD / LA tags of the records tool 1 converts are
  cut out here, by a walk over the aux tags (a B array or Z string that holds "RD" is payload).
* ``host``    -- bsdc_toolrec_host over a fetched dump: the twin's bytes (the whole-file path, and
  what the tests compare the kernel with).
* ``header``  -- the input's header with SO:unsorted GO:query SS:unsorted:template-coordinate.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from . import records as R
from .batch import LINK_CONVERT

HD_TAGS = (("SO", "unsorted"), ("GO", "query"), ("SS", "unsorted:template-coordinate"))
_AUX_FIXED = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}


@dataclass
class Tables:
    """One batch's inputs of bsdc_toolrec_format besides the dump: tab [n_rec] (_lib.TOOLREC_REC),
    names / aux uint8 (aux padded to a non-empty buffer), cigar uint32."""

    tab: np.ndarray
    names: np.ndarray
    cigar: np.ndarray
    aux: np.ndarray

    @property
    def n(self) -> int:
        return int(self.tab.shape[0])

    def bound(self, n_dump: int) -> int:
        return int(_lib.load().bsdc_toolrec_bytes_bound(self.n, int(self.names.shape[0]), int(self.cigar.shape[0]),
                                                        int(self.aux.shape[0]), int(n_dump)))


def header(h):
    """The input's BamHeader with @HD carrying SO:unsorted GO:query SS:unsorted:template-coordinate
    (an @HD line is added when there is none); the reference list unchanged, no @PG added."""
    import dataclasses
    lines = h.text.split("\n")
    want = dict(HD_TAGS)
    for i, line in enumerate(lines):
        if line.startswith("@HD"):
            f = [x for x in line.split("\t")[1:] if x[:2] not in want]
            lines[i] = "\t".join(["@HD"] + f + ["%s:%s" % kv for kv in HD_TAGS])
            break
    else:
        lines.insert(0, "\t".join(["@HD", "VN:1.6"] + ["%s:%s" % kv for kv in HD_TAGS]))
    return dataclasses.replace(h, text="\n".join(lines))


def strip_rd_la(aux: bytes) -> bytes:
    """An aux block without its RD and LA tags (pysam's set_tag removes before it appends,
    tools/1.convert_AG_to_CT.py:180-183); the other tags in order.  The tags are walked by their
    types, so a B array or a Z / H string whose payload holds "RD" or "LA" is kept whole."""
    out, i, n = [], 0, len(aux)
    while i + 3 <= n:
        t = aux[i + 2]
        if t in _AUX_FIXED:
            j = i + 3 + _AUX_FIXED[t]
        elif t in (ord("Z"), ord("H")):
            j = aux.index(b"\0", i + 3) + 1
        elif t == ord("B"):
            j = i + 8 + _AUX_FIXED[aux[i + 3]] * int.from_bytes(aux[i + 4:i + 8], "little")
        else:
            raise ValueError("aux tag %r has the unknown type %r" % (aux[i:i + 2], chr(t)))
        if j > n:
            raise ValueError("aux tag %r runs past the record" % (aux[i:i + 2],))
        if aux[i:i + 2] not in (b"RD", b"LA"):
            out.append(aux[i:j])
        i = j
    if i != n:
        raise ValueError("trailing aux bytes")
    return b"".join(out)


def _ragged(off: np.ndarray, ln: np.ndarray) -> np.ndarray:
    """indices off[k] .. off[k] + ln[k] - 1 for every k, concatenated"""
    ln = np.asarray(ln, np.int64)
    tot = int(ln.sum())
    if tot == 0:
        return np.zeros(0, np.int64)
    start = np.cumsum(ln) - ln
    return np.repeat(np.asarray(off, np.int64) - start, ln) + np.arange(tot, dtype=np.int64)


def _holds_rd_la(buf: np.ndarray, off: np.ndarray) -> np.ndarray:
    """per entry of the packed table: its bytes hold "RD" or "LA" somewhere (vectorised)"""
    n = int(off.shape[0]) - 1
    out = np.zeros(n, bool)
    if buf.shape[0] < 2 or n == 0:
        return out
    a, b = buf[:-1], buf[1:]
    at = np.nonzero(((a == ord("R")) & (b == ord("D"))) | ((a == ord("L")) & (b == ord("A"))))[0]
    k = np.searchsorted(off, at, "right") - 1
    ok = (k >= 0) & (k < n)
    k, at = k[ok], at[ok]
    out[k[at + 2 <= off[k + 1]]] = True  # (both bytes inside the entry)
    return out


def tables(raw: R.RawRecords, src: np.ndarray, conv: np.ndarray) -> Tables:
    """The table of the records raw[src] in that order; conv: the records tool 1 converts (their
    dump tags may carry bit1), whose RD / LA tags are cut out of the aux bytes."""
    src = np.asarray(src, np.int64)
    conv = np.asarray(conv, bool)
    n = int(src.shape[0])
    tab = np.zeros(n, _lib.TOOLREC_REC)
    for k, v in (("ref_id", raw.tid), ("next_ref_id", raw.next_tid), ("next_pos", raw.next_pos), ("tlen", raw.tlen),
                 ("flag", raw.flag), ("mapq", raw.mapq)):
        tab[k] = np.asarray(v)[src]
    # names
    nid = np.asarray(raw.name_id, np.int64)[src]
    if hasattr(raw.names, "off"):
        noff, nbuf = raw.names.off, raw.names.buf
        nl = (noff[nid + 1] - noff[nid]).astype(np.int64)
        names = nbuf[_ragged(noff[nid], nl)]
    else:
        bs = [raw.names[int(i)] for i in nid]
        bs = [x if isinstance(x, bytes) else str(x).encode() for x in bs]
        nl = np.asarray([len(x) for x in bs], np.int64)
        names = np.frombuffer(b"".join(bs), np.uint8)
    if n and (nl.min() < 1 or nl.max() > 254):
        raise ValueError("a read name outside 1..254 bytes")
    tab["name_len"] = nl
    tab["name_off"] = np.cumsum(nl) - nl
    # cigar ops without the leading and the trailing S
    co = np.asarray(raw.cig_off, np.int64)[src]
    nc = np.asarray(raw.n_cig, np.int64)[src]
    cg = np.asarray(raw.cigar, np.uint32)
    has = nc > 0
    lead = np.zeros(n, bool)
    lead[has] = (cg[co[has]] & 15) == R.OP_S
    co, nc = co + lead, nc - lead
    has = nc > 0
    trail = np.zeros(n, bool)
    trail[has] = (cg[co[has] + nc[has] - 1] & 15) == R.OP_S
    nc = nc - trail
    tab["n_cig"] = nc
    tab["cig_off"] = np.cumsum(nc) - nc
    cigar = cg[_ragged(co, nc)]
    # aux bytes; RD / LA cut out where tool 1 sets them
    if raw.aux is None:
        aux = np.zeros(0, np.uint8)
        al = np.zeros(n, np.int64)
    elif hasattr(raw.aux, "off"):
        aoff, abuf = raw.aux.off, raw.aux.buf
        al = (aoff[src + 1] - aoff[src]).astype(np.int64)
        # the converted records whose aux holds the bytes "RD" or "LA" anywhere are walked (a tag of
        # any type and value; a payload that merely reads so is kept by the walk)
        cut = conv & _holds_rd_la(abuf, aoff)[src] if conv.any() else conv
        if cut.any():
            parts = []
            for k in range(n):
                b = abuf[int(aoff[src[k]]):int(aoff[src[k] + 1])].tobytes()
                parts.append(strip_rd_la(b) if cut[k] else b)
            al = np.asarray([len(x) for x in parts], np.int64)
            aux = np.frombuffer(b"".join(parts), np.uint8)
        else:
            aux = abuf[_ragged(aoff[src], al)]
    else:
        parts = [bytes(raw.aux[int(i)]) for i in src]
        parts = [strip_rd_la(b) if c else b for b, c in zip(parts, conv)]
        al = np.asarray([len(x) for x in parts], np.int64)
        aux = np.frombuffer(b"".join(parts), np.uint8)
    tab["aux_len"] = al
    tab["aux_off"] = np.cumsum(al) - al
    pad = (-int(aux.shape[0])) % 4 or (4 if aux.shape[0] == 0 else 0)
    aux = np.concatenate([aux, np.zeros(pad, np.uint8)])  # (a copy: numpy's own, aligned allocation)
    return Tables(tab, np.ascontiguousarray(names if names.shape[0] else np.zeros(1, np.uint8)),
                  np.ascontiguousarray(cigar if cigar.shape[0] else np.zeros(1, np.uint32)), aux)


def batch_tables(raw: R.RawRecords, fb) -> Tables:
    """tables() of a FamilyBatch: its records in batch order, converted = the link word's bit."""
    return tables(raw, fb.src, (np.asarray(fb.rec_link) & LINK_CONVERT) != 0)


def _consensus_c(dump_pos, dump_len, dump_tags, dump_seq, dump_qual):
    o = _lib.ConsensusC()
    o.dump_pos, o.dump_len, o.dump_tags = dump_pos.ctypes.data, dump_len.ctypes.data, dump_tags.ctypes.data
    o.dump_seq, o.dump_qual = dump_seq.ctypes.data, dump_qual.ctypes.data
    return o


def host(t: Tables, rec_off: np.ndarray, dump_pos, dump_len, dump_tags, dump_seq, dump_qual,
         cap: Optional[int] = None, fill: Optional[int] = None):
    """bsdc_toolrec_host -> (off int64 [n + 1], the buffer uint8 [cap]): the records are
    buf[:off[n]].  rec_off [n]: each record's offset in dump_seq / dump_qual (FamilyBatch.rec_off);
    dump_*: DeviceBatch.fetch's arrays; cap: the buffer's size (default: the bound); fill: the
    byte the buffer holds beforehand."""
    lib = _lib.load()
    n = t.n
    rec = np.zeros((max(n, 1), 4), np.uint32)
    rec[:n, 0] = np.asarray(rec_off, np.uint32)[:n]
    dp = np.ascontiguousarray(dump_pos, np.int32)
    dl = np.ascontiguousarray(dump_len).astype(np.uint16)
    dt = np.ascontiguousarray(dump_tags, np.uint8)
    n_dump = int(min(dump_seq.shape[0], dump_qual.shape[0])) // 4 * 4
    ds = np.ascontiguousarray(dump_seq[:n_dump], np.uint8)
    dq = np.ascontiguousarray(dump_qual[:n_dump], np.uint8)
    if n_dump == 0:
        ds = dq = np.zeros(4, np.uint8)
    if n == 0:
        dp, dl, dt = np.zeros(1, np.int32), np.zeros(1, np.uint16), np.zeros(1, np.uint8)
    o = _consensus_c(dp, dl, dt, ds, dq)
    cap = t.bound(n_dump) if cap is None else int(cap)
    buf = np.empty(max(cap, 1), np.uint8) if fill is None else np.full(max(cap, 1), fill, np.uint8)
    off = np.zeros(n + 1, np.int64)
    rc = lib.bsdc_toolrec_host(C.byref(o), rec.ctypes.data, n, n_dump, t.tab.ctypes.data, t.names.ctypes.data,
                               int(t.names.shape[0]), t.cigar.ctypes.data, int(t.cigar.shape[0]), t.aux.ctypes.data,
                               int(t.aux.shape[0]), off.ctypes.data, buf.ctypes.data, cap)
    if rc != 0:
        raise ValueError("bsdc_toolrec_host failed (%d): %s" % (rc, lib.bsdc_toolrec_last_error().decode()))
    return off, buf


def host_bytes(raw: R.RawRecords, fb, out: dict) -> np.ndarray:
    """A fetched batch's (DeviceBatch.fetch with dump) tool-stage records as BAM record bytes."""
    off, buf = host(batch_tables(raw, fb), fb.rec_off, out["dump_pos"], out["dump_len"], out["dump_tags"],
                    out["dump_seq"], out["dump_qual"])
    return buf[:int(off[-1])]


_HD_RE = re.compile(r"^@HD\t.*$", re.M)


def hd_line(text: str) -> Optional[str]:
    m = _HD_RE.search(text)
    return m.group(0) if m else None

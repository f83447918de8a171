"""cli group: paired-UMI molecule ids for the templates of a tagged, aligned
BAM -- the file `fgbio GroupReadsByUmi -s Paired` leaves, the input of cli molecular.  fgbio
GroupReadsByUmi restated, parity unpinned.

* ``templates`` -- rules 1-3 on the host: the records joined by read name and end, the filters with
  their counters, the 5' positions, the position keys and the packed canonical UMIs, in name order.
* ``assign_host`` / ``assign_device`` -- rules 4-6 (bsdc_group_assign_host / bsdc_group_assign).
* ``format_host`` / ``format_device`` -- rule 7's records (bsdc_group_format_host / bsdc_group_format).
* ``header``  -- rule 7's header.
* ``group``   -- the driver: one GPU, the input read whole (streaming is a follow-up); the records
  are checksummed, deflated and packed on the device behind the BAM writer's sink.  host=True runs
  the host twins and the host deflate instead: for the tests, never chosen by cli.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from . import bam
from .toolrec import _ragged
from .zipper import Records, read_records

DROPS = ("secondary_supplementary_records", "not_paired", "unmapped_or_mate_unmapped", "no_reference", "non_pf",
         "low_mapq", "umi_other_letters")
POS_BIAS = 1 << 30  # added to a 5' position (clipping can take it below 0) before it is packed


@dataclass
class Templates:
    """The kept templates in name order: r1 / r2 (their records in the input), k0 / k1 / umi /
    strand (bsdc_group_assign's inputs), counts (templates_in and the drop counters)."""
    r1: np.ndarray
    r2: np.ndarray
    k0: np.ndarray
    k1: np.ndarray
    umi: np.ndarray
    strand: np.ndarray
    counts: dict

    @property
    def n(self) -> int:
        return int(self.r1.shape[0])

    @property
    def kmax(self) -> np.ndarray:
        red = lambda x: np.bitwise_or.reduce(x) if x.shape[0] else np.uint64(0)  # noqa: E731
        return np.asarray([red(self.k0), red(self.k1), red(self.umi)], np.uint64)


def _name(a: Records, k: int) -> str:
    return a.name(int(k)).decode(errors="replace")


def five_prime(a: Records, recs: np.ndarray) -> np.ndarray:
    """Rule 2: the unclipped start of a forward record, the unclipped end of a reverse one (0-based)."""
    s = a.src[recs]
    off = s["off"].astype(np.int64)
    n_cig = (a.buf[off + 16].astype(np.int64) | a.buf[off + 17].astype(np.int64) << 8)
    c0 = off + 36 + s["name_len"].astype(np.int64) + 1
    words = a.buf[_ragged(c0, 4 * n_cig)].reshape(-1, 4).astype(np.int64)
    ops = words[:, 0] | words[:, 1] << 8 | words[:, 2] << 16 | words[:, 3] << 24
    seg = np.repeat(np.arange(recs.shape[0]), n_cig)
    op, ln = ops & 15, ops >> 4
    clip = (op == 4) | (op == 5)
    m = recs.shape[0]
    ref_len = np.bincount(seg, np.where(np.isin(op, (0, 2, 3, 7, 8)), ln, 0), m).astype(np.int64)
    body_ops = np.bincount(seg, (~clip).astype(np.int64), m).astype(np.int64)
    body = np.cumsum(~clip) - np.repeat(np.cumsum(body_ops) - body_ops, n_cig)  # non-clip ops up to here, in the record
    lead = np.bincount(seg, np.where(clip & (body == 0), ln, 0), m).astype(np.int64)
    trail = np.bincount(seg, np.where(clip & (body > 0), ln, 0), m).astype(np.int64)
    pos = s["pos"].astype(np.int64)
    rev = (s["flag"] & 0x10) != 0
    return np.where(rev, pos + np.maximum(ref_len, 1) - 1 + trail, pos - lead)


_FIXED = {65: 1, 99: 1, 67: 1, 115: 2, 83: 2, 105: 4, 73: 4, 102: 4}  # A c C s S i I f


def _raw_umi(a: Records, k: int, tag: bytes):
    """The raw tag's Z value of record k (aux walked by type, every step inside the block), None
    when it has none; a malformed block is an error that names the read."""
    o, ln, ax = int(a.src["off"][k]), int(a.src["len"][k]), int(a.src["aux"][k])
    b = a.buf[o + ax:o + ln].tobytes()
    i, n = 0, len(b)
    while i < n:
        j, what = -1, "runs past the record"
        if i + 3 > n:
            what = "is cut short"
        elif b[i + 2] in _FIXED:
            j = i + 3 + _FIXED[b[i + 2]]
        elif b[i + 2] in (90, 72):
            j = b.find(0, i + 3) + 1 or -1
        elif b[i + 2] == 66 and i + 8 <= n and b[i + 3] in _FIXED and b[i + 3] != 65:
            j = i + 8 + _FIXED[b[i + 3]] * int.from_bytes(b[i + 4:i + 8], "little")
        elif b[i + 2] != 66 or i + 8 <= n:
            what = "has an unknown type"
        if j < 0 or j > n:
            raise ValueError("read %r: aux tag %r %s" % (_name(a, k), b[i:i + 2].decode(errors="replace"), what))
        if b[i:i + 2] == tag:
            return b[i + 3:j - 1] if b[i + 2] == 90 else None
        i = j
    return None


_DIGIT = bytes.maketrans(b"ACGT", b"0123")


def _pack(half: bytes) -> int:
    """Two bits a base, the first base highest (the half holds ACGT only)"""
    return int(half.translate(_DIGIT), 4)


def templates(a: Records, min_map_q: int = 1, include_non_pf: bool = False, raw_tag: str = "RX") -> Templates:
    """Rules 1-3."""
    counts = {"records_in": a.n}
    flag = a.src["flag"].astype(np.int64)
    prim = np.nonzero((flag & 0x900) == 0)[0]
    counts["secondary_supplementary_records"] = a.n - int(prim.shape[0])
    ln = a.src["name_len"][prim].astype(np.int64)
    o = np.zeros(prim.shape[0] + 1, np.int64)
    o[1:] = np.cumsum(ln)
    rank = bam.table_ranks(bam.StringTable(a.buf[_ragged(a.src["off"][prim] + 36, ln)], o))[:prim.shape[0]] \
        if prim.shape[0] else np.zeros(0, np.int64)
    end = (flag[prim] >> 6) & 3
    key = rank * 4 + end
    by = np.argsort(key, kind="stable")
    ks = key[by]
    dup = np.nonzero((ks[1:] == ks[:-1]) & np.isin(ks[1:] & 3, (1, 2)))[0]
    if dup.shape[0]:
        k = int(prim[by[dup[0] + 1]])
        raise ValueError("read %r (flag %d) occurs twice" % (_name(a, k), int(flag[k])))
    tr, first = np.unique(rank[by], return_index=True)
    nt = int(tr.shape[0])
    counts["templates_in"] = nt
    size = np.diff(np.append(first, by.shape[0]))
    e0 = ks[first] & 3
    paired = (size == 2) & (e0 == 1) & ((ks[np.minimum(first + 1, max(by.shape[0] - 1, 0))] & 3) == 2) if nt else np.zeros(0, bool)
    r1 = prim[by[first]]
    r2 = prim[by[np.minimum(first + 1, max(by.shape[0] - 1, 0))]] if nt else r1
    f1, f2 = flag[r1], flag[r2]
    s1, s2 = a.src[r1], a.src[r2]
    mq1, mq2 = a.buf[s1["off"].astype(np.int64) + 13], a.buf[s2["off"].astype(np.int64) + 13]
    alive = np.ones(nt, bool)
    for name, bad in (("not_paired", ~paired),
                      ("unmapped_or_mate_unmapped", ((f1 & f2 & 1) == 0) | (((f1 | f2) & 0xC) != 0)),
                      ("no_reference", (s1["ref_id"] < 0) | (s2["ref_id"] < 0)),
                      ("non_pf", (((f1 | f2) & 0x200) != 0) & (not include_non_pf)),
                      ("low_mapq", (mq1 < min_map_q) | (mq2 < min_map_q))):
        hit = alive & bad
        counts[name] = int(hit.sum())
        alive &= ~hit
    keep = np.nonzero(alive)[0]
    r1, r2 = r1[keep], r2[keep]
    # the raw tag of R1
    tag = raw_tag.encode()
    umi0, umi1, l0, l1 = (np.zeros(keep.shape[0], np.uint64) for _ in range(4))
    ok = np.ones(keep.shape[0], bool)
    for t, k in enumerate(r1):
        u = _raw_umi(a, int(k), tag)
        if u is None:
            raise ValueError("read %r has no %s:Z tag" % (_name(a, k), raw_tag))
        h = u.split(b"-")
        if len(h) != 2 or not h[0] or not h[1]:
            raise ValueError("read %r: %s %r is not two halves joined by one '-'" % (_name(a, k), raw_tag, u.decode(errors="replace")))
        if (h[0] + h[1]).translate(None, b"ACGT"):
            ok[t] = False
            continue
        if max(len(h[0]), len(h[1])) > 16:
            raise ValueError("read %r: %s %r has more than 16 bases in a half" % (_name(a, k), raw_tag, u.decode()))
        umi0[t], umi1[t], l0[t], l1[t] = _pack(h[0]), _pack(h[1]), len(h[0]), len(h[1])
    counts["umi_other_letters"] = int((~ok).sum())
    r1, r2, umi0, umi1, l0, l1 = (x[ok] for x in (r1, r2, umi0, umi1, l0, l1))
    # ends, keys, canonical UMIs
    p1, p2 = five_prime(a, r1), five_prime(a, r2)
    if r1.shape[0] and (min(p1.min(), p2.min()) < -POS_BIAS or max(p1.max(), p2.max()) >= POS_BIAS):
        raise ValueError("a 5' position is outside +-2^30")
    t1, t2 = a.src["ref_id"][r1].astype(np.int64), a.src["ref_id"][r2].astype(np.int64)
    v1, v2 = (flag[r1] >> 4) & 1, (flag[r2] >> 4) & 1
    e1 = (t1 << 32 | (p1 + POS_BIAS) << 1 | v1).astype(np.uint64)
    e2 = (t2 << 32 | (p2 + POS_BIAS) << 1 | v2).astype(np.uint64)
    c1, c2 = t1 << 32 | (p1 + POS_BIAS), t2 << 32 | (p2 + POS_BIAS)
    top = (c1 < c2) | ((c1 == c2) & (v1 == 0))
    k0, k1 = np.where(top, e1, e2), np.where(top, e2, e1)
    umi = np.where(top, umi0 << np.uint64(32) | umi1, umi1 << np.uint64(32) | umi0)
    la, lb = np.where(top, l0, l1), np.where(top, l1, l0)
    by = np.lexsort((k1, k0))  # (a check only: the half lengths of a position group agree)
    same = (k0[by][1:] == k0[by][:-1]) & (k1[by][1:] == k1[by][:-1])
    bad = np.nonzero(same & ((la[by][1:] != la[by][:-1]) | (lb[by][1:] != lb[by][:-1])))[0]
    if bad.shape[0]:
        x, y = int(by[bad[0]]), int(by[bad[0] + 1])
        raise ValueError("reads %r and %r lie in one position group but their UMI halves differ in length (%d+%d, %d+%d)" % (
            _name(a, r1[x]), _name(a, r1[y]), int(la[x]), int(lb[x]), int(la[y]), int(lb[y])))
    return Templates(r1, r2, np.ascontiguousarray(k0, np.uint64), np.ascontiguousarray(k1, np.uint64),
                     np.ascontiguousarray(umi, np.uint64), np.ascontiguousarray(~top, np.uint8), counts)


def header(h: bam.BamHeader) -> bam.BamHeader:
    """Rule 7: the input's header with @HD SO:unsorted GO:query SS:unsorted:template-coordinate."""
    lines = [x for x in h.text.split("\n") if x]
    vn = "1.6"
    for x in lines:
        if x.startswith("@HD"):
            vn = next((f[3:] for f in x.split("\t")[1:] if f.startswith("VN:")), vn)
    lines = ["@HD\tVN:%s\tSO:unsorted\tGO:query\tSS:unsorted:template-coordinate" % vn] + [x for x in lines if not x.startswith("@HD")]
    return bam.BamHeader("\n".join(lines) + "\n", list(h.ref_names), np.asarray(h.ref_lens, np.int64))


def rec_table(a: Records, t: Templates) -> np.ndarray:
    """bsdc_group_rec [2n]: template k's R1 and R2 at 2k, 2k + 1"""
    tab = np.zeros(2 * t.n, _lib.GROUP_REC)
    for e, r in ((0, t.r1), (1, t.r2)):
        s = a.src[r]
        tab["off"][e::2], tab["len"][e::2], tab["aux"][e::2] = s["off"], s["len"], s["aux"]
    return tab


def _pad(x: np.ndarray, dt) -> np.ndarray:
    x = np.ascontiguousarray(x, dt)
    return x if x.shape[0] else np.zeros(1, dt)


def _err(what: str, rc: int) -> ValueError:
    return ValueError("%s failed (%d): %s" % (what, rc, _lib.load().bsdc_group_last_error().decode()))


def assign_host(k0, k1, umi, strand, edits: int = 1, kmax=None):
    """bsdc_group_assign_host -> (mol uint32 [n], ab uint8 [n], order uint32 [n], stats int64 [4])"""
    lib = _lib.load()
    n = int(np.asarray(k0).shape[0])
    k0, k1, umi, strand = _pad(k0, np.uint64), _pad(k1, np.uint64), _pad(umi, np.uint64), _pad(strand, np.uint8)
    if kmax is None:
        kmax = np.asarray([np.bitwise_or.reduce(x[:max(n, 1)]) for x in (k0, k1, umi)], np.uint64)
    kmax = np.ascontiguousarray(kmax, np.uint64)
    mol, ab, order, stats = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32), np.zeros(4, np.int64)
    rc = lib.bsdc_group_assign_host(k0.ctypes.data, k1.ctypes.data, umi.ctypes.data, strand.ctypes.data, n, int(edits),
                                    kmax.ctypes.data, mol.ctypes.data, ab.ctypes.data, order.ctypes.data, stats.ctypes.data)
    if rc != 0:
        raise _err("bsdc_group_assign_host", rc)
    return mol[:n], ab[:n], order[:n], stats


def assign_device(device, k0, k1, umi, strand, edits: int = 1, kmax=None, arena: int = 0):
    """bsdc_group_assign on one GPU -> (mol, ab, order: device tensors viewed as uint8 bytes, stats)"""
    import torch
    lib = _lib.load()
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    n = int(np.asarray(k0).shape[0])
    k0, k1, umi, strand = _pad(k0, np.uint64), _pad(k1, np.uint64), _pad(umi, np.uint64), _pad(strand, np.uint8)
    if kmax is None:
        kmax = np.asarray([np.bitwise_or.reduce(x[:max(n, 1)]) for x in (k0, k1, umi)], np.uint64)
    kmax = np.ascontiguousarray(kmax, np.uint64)
    up = lambda x: torch.from_numpy(x.view(np.uint8)).to(dev)  # noqa: E731
    stats = np.zeros(4, np.int64)
    with torch.cuda.device(dev):
        d = [up(x) for x in (k0, k1, umi, strand)]
        mol = torch.zeros(4 * max(n, 1), dtype=torch.uint8, device=dev)
        ab = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        order = torch.zeros(4 * max(n, 1), dtype=torch.uint8, device=dev)
        tmp = torch.empty(int(lib.bsdc_group_tmp_bytes(n)), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev)
        rc = lib.bsdc_group_assign(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, int(edits),
                                   kmax.ctypes.data, int(arena), mol.data_ptr(), ab.data_ptr(), order.data_ptr(),
                                   stats.ctypes.data, tmp.data_ptr(), C.c_void_p(st.cuda_stream))
        st.synchronize()
        if rc != 0:
            raise _err("bsdc_group_assign", rc)
    return mol, ab, order, stats


def bound(tab: np.ndarray) -> int:
    return int(_lib.load().bsdc_group_bytes_bound(_pad(tab, _lib.GROUP_REC).ctypes.data, int(tab.shape[0])))


def format_host(order, mol, ab, tab: np.ndarray, rec: np.ndarray, tag: str = "MI", cap: Optional[int] = None):
    """bsdc_group_format_host -> (off int64 [2n + 1], the buffer): the records are buf[:off[2n]]."""
    lib = _lib.load()
    n = int(np.asarray(order).shape[0])
    cap = bound(tab) if cap is None else int(cap)
    buf, off = np.zeros(max(cap, 1), np.uint8), np.zeros(2 * n + 1, np.int64)
    rc = lib.bsdc_group_format_host(_pad(order, np.uint32).ctypes.data, _pad(mol, np.uint32).ctypes.data,
                                    _pad(ab, np.uint8).ctypes.data, n, _pad(tab, _lib.GROUP_REC).ctypes.data, rec.ctypes.data,
                                    int(rec.shape[0]), tag.encode(), off.ctypes.data, buf.ctypes.data, cap)
    if rc != 0:
        raise _err("bsdc_group_format_host", rc)
    return off, buf


def format_device(order, mol, ab, tab: np.ndarray, rec: np.ndarray, tag: str = "MI"):
    """bsdc_group_format behind assign_device's tensors -> (the records' uint8 device tensor, their
    byte count, an event behind the kernels)."""
    import torch
    lib = _lib.load()
    dev = order.device
    n = int(ab.shape[0]) if tab.shape[0] else 0
    tab_h = _pad(tab, _lib.GROUP_REC)
    with torch.cuda.device(dev):
        d_tab = torch.from_numpy(tab_h.view(np.uint8)).to(dev)
        d_rec = torch.from_numpy(rec).to(dev)
        cap = bound(tab)
        dst = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        off = torch.zeros(2 * n + 1, dtype=torch.int64, device=dev)
        tmp = torch.empty(int(lib.bsdc_group_format_tmp_bytes(n)), dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev)
        rc = lib.bsdc_group_format(order.data_ptr(), mol.data_ptr(), ab.data_ptr(), n, d_tab.data_ptr(), tab_h.ctypes.data,
                                   d_rec.data_ptr(), rec.ctypes.data, int(rec.shape[0]), tag.encode(), off.data_ptr(),
                                   dst.data_ptr(), cap, tmp.data_ptr(), C.c_void_p(st.cuda_stream))
        if rc != 0:
            st.synchronize()
            raise _err("bsdc_group_format", rc)
        total = int(off[2 * n].item())  # (synchronises the stream)
        ev = torch.cuda.Event()
        ev.record(st)
    return dst, total, ev


def histogram(mol: np.ndarray, ab: np.ndarray) -> dict:
    """templates per <id>/<strand> as size -> count (fgbio's -f)"""
    if not mol.shape[0]:
        return {}
    fam = np.bincount(mol.astype(np.int64) * 2 + ab)
    size, cnt = np.unique(fam[fam > 0], return_counts=True)
    return {str(int(s)): int(c) for s, c in zip(size, cnt)}


def group(inp: str, out: str, edits: int = 1, min_map_q: int = 1, include_non_pf_reads: bool = False, raw_tag: str = "RX",
          assign_tag: str = "MI", strategy: str = "paired", threads: int = 0, level: int = 6, device=0,
          info: Optional[str] = None, host: bool = False, arena: int = 0) -> dict:
    """IN.bam -> OUT.bam (module docstring; rules in DESIGN.md 3.12).  -> the info dict (also
    written to `info` as JSON)."""
    from . import bgzf
    if strategy.lower() != "paired":
        raise ValueError("strategy %r is not built: only 'paired' is" % strategy)
    if not 0 <= int(edits) <= 3:
        raise ValueError("--edits takes 0..3")
    if len(raw_tag.encode()) != 2 or len(assign_tag.encode()) != 2:
        raise ValueError("a tag name has two letters")
    a = read_records(inp, threads)
    t = templates(a, min_map_q, include_non_pf_reads, raw_tag)
    tab = rec_table(a, t)
    hdr = header(a.header)
    if host:
        mol, ab, order, stats = assign_host(t.k0, t.k1, t.umi, t.strand, edits, t.kmax)
        off, buf = format_host(order, mol, ab, tab, a.buf, assign_tag)
        total = int(off[-1])
        w = bgzf.BamWriter(out, hdr, level)
        try:
            w.add_raw(buf[:total].tobytes(), threads)
        finally:
            w.close(threads)
    else:
        d_mol, d_ab, d_order, stats = assign_device(device, t.k0, t.k1, t.umi, t.strand, edits, t.kmax, arena)
        dst, total, ev = format_device(d_order, d_mol, d_ab, tab, a.buf, assign_tag)
        w = bgzf.BamWriter(out, hdr, level, bgzf.GpuBgzf(dst.device))
        try:
            if total:
                w.add_device([[(dst, 0, total, ev)]], threads)
        finally:
            w.close(threads)
        mol, ab = d_mol.cpu().numpy().view(np.uint32)[:t.n], d_ab.cpu().numpy()[:t.n]
    res = dict(t.counts)
    res.update({"templates_out": t.n, "position_groups": int(stats[0]), "molecules": int(stats[2]),
                "max_nodes_in_group": int(stats[3]), "family_size_histogram": histogram(mol, ab), "raw_bytes": total,
                "compressed_bytes": os.path.getsize(out)})
    if info is not None:
        with open(info, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")
    return res

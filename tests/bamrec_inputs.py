"""Fabricated consensus outputs for the device BAM record path (csrc/bsdc_bam.hip): the arrays a
tags vote leaves -- status, len, packed seq, qual, ss_len, the four single-strand rows, ss_wide with
its wide rows, the filter's filt -- and a name and an aux table per family, built with no vote so
that every branch of the formatter is met at a small size, plus the yardstick: the same families
through bam.consensus_tags and the host BAM writer as a headerless fragment, gunzipped."""
import gzip
import os
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from bsseqconsensusreads_amd import bam, bgzf


@dataclass
class BamRecInput:
    stride: int
    status: np.ndarray   # u8 [F]
    length: np.ndarray   # i32 [F, 2]
    seq: np.ndarray      # u8 [F, 2, stride / 2] packed nt16, high nibble first
    qual: np.ndarray     # u8 [F, 2, stride]
    filt: np.ndarray     # u8 [F] reason bits (0 = kept)
    names: "bam.StringTable"
    aux: "bam.StringTable"
    ss_len: np.ndarray   # i32 [F, 4]
    ss_base: np.ndarray  # u8 [F, 4, stride]
    ss_qual: np.ndarray
    ss_depth: np.ndarray
    ss_err: np.ndarray
    ss_wide: np.ndarray  # i32 [F]: the family's wide row, -1 none
    ss_wdepth: np.ndarray  # u16 [W, 4, stride]
    ss_werr: np.ndarray
    notes: dict          # edge -> the family that holds it

    @property
    def n_fam(self) -> int:
        return int(self.status.shape[0])

    def kept(self, with_filt: bool) -> np.ndarray:
        k = (self.status & 1) != 0
        return k & (self.filt == 0) if with_filt else k

    def depth16(self) -> np.ndarray:
        """[F, 4, stride] the depths the tags read: the wide rows where a family has them"""
        d = self.ss_depth.astype(np.int64)
        w = self.ss_wide >= 0
        d[w] = self.ss_wdepth[self.ss_wide[w]]
        return d


SPECIAL_LEN = lambda stride: [0, 1, 2, 3, 4, 5, min(7, stride - 3) | 1, stride - 2]  # noqa: E731


def make(stride: int, n_fam: int = 300, seed: int = 0, written: str = "mixed", vector_tables: bool = False) -> BamRecInput:
    """vector_tables: the name and the aux table out of one draw each (other bytes than the per-family
    draws give): for a batch too large for them.
    written: "mixed" (unemitted and filtered families at the front, at the back and in runs),
    "none", "all", "first_off" / "last_off" (only that family unemitted).  n_fam >= 40 places every
    edge of the module docstring (notes says where); every name length 1..253 occurs from 300 on."""
    rng = np.random.default_rng(seed)
    F = n_fam
    status = np.full(F, 1, np.uint8) | (rng.integers(0, 4, F).astype(np.uint8) << 1)
    filt = np.zeros(F, np.uint8)
    if written == "mixed":
        off = rng.random(F) < 0.15
        off[:3] = True
        off[-2:] = True
        off[40:57] = True  # a run
        status[off] &= 0xFE
        fl = rng.random(F) < 0.1
        fl[3:5] = True
        fl[-4:-2] = True
        filt[fl] = rng.integers(1, 16, int(fl.sum())).astype(np.uint8)
    elif written == "none":
        status &= 0xFE
    elif written == "first_off":
        status[0] &= 0xFE
    elif written == "last_off":
        status[-1] &= 0xFE
    special = SPECIAL_LEN(stride)
    length = rng.integers(0, stride - 1, (F, 2)).astype(np.int32)
    for f in range(F):
        if f % 3 == 0:
            length[f, 0] = special[(f // 3) % len(special)]
        if f % 3 == 1:
            length[f, 1] = special[(f // 3 + 3) % len(special)]
    length = np.minimum(length, stride - 2)
    seq = rng.integers(0, 256, (F, 2, stride // 2)).astype(np.uint8)  # (every code, also past the lengths)
    qual = rng.integers(0, 256, (F, 2, stride)).astype(np.uint8)
    ss_len = np.zeros((F, 4), np.int32)
    # garbage everywhere, also past the lengths; errors mostly at most the depth
    ss_base = rng.integers(0, 256, (F, 4, stride)).astype(np.uint8)
    ss_base[:, :, ::3] &= 15
    ss_qual = rng.integers(0, 256, (F, 4, stride)).astype(np.uint8)
    ss_depth = rng.integers(0, 256, (F, 4, stride)).astype(np.uint8)
    ss_err = (ss_depth * rng.random((F, 4, stride)) * 0.3).astype(np.uint8)
    ss_err[::7] = rng.integers(0, 256, ss_err[::7].shape).astype(np.uint8)
    # strands: 0 both, 1 AB only, 2 BA only, 3 R1 from AB alone and R2 from both
    strands = rng.integers(0, 4, F)
    n = np.maximum(length, 1)
    ss_len[:, 0], ss_len[:, 1] = np.where(strands != 2, n[:, 0], 0), np.where(strands != 2, n[:, 1], 0)
    ss_len[:, 2], ss_len[:, 3] = np.where(strands % 2 == 0, n[:, 0], 0), np.where(strands != 1, n[:, 1], 0)
    notes = {}
    kept = np.nonzero(((status & 1) != 0) & (filt == 0))[0]
    free = [int(f) for f in kept if f % 3 == 2]  # (their lengths are not the special ones)
    wide = np.full(F, -1, np.int32)
    wd, we = [], []
    Lf = max(stride - 3, 1) | 1 if stride > 16 else stride - 3

    def claim(name, both=True, wide_rows=False):
        if not free:
            return None
        f = free.pop(0)
        notes[name] = f
        length[f] = Lf
        ss_len[f] = [Lf, Lf, Lf, Lf] if both else ss_len[f]
        if wide_rows:
            wide[f] = len(wd)
            wd.append(rng.integers(0, 300, (4, stride)).astype(np.uint16))
            we.append(rng.integers(0, 300, (4, stride)).astype(np.uint16))
        return f

    f = claim("no_depth")  # 0 / 0: the NaN bits, in c, a and b
    if f is not None:
        ss_depth[f] = 0
        ss_err[f] = 0
    f = claim("d255")  # a: D = M = 255 (C, C); b: depth 1, so c: D = M = 256 (S, S)
    if f is not None:
        ss_depth[f, :2] = 255
        ss_depth[f, 2:] = 1
    f = claim("d255_min")  # c: D = 255 (C) with M below
    if f is not None:
        ss_depth[f] = rng.integers(0, 100, (4, stride)).astype(np.uint8)
        ss_depth[f, :2, 1] = 200
        ss_depth[f, 2:, 1] = 55
    f = claim("d256_m255", wide_rows=True)  # a: D = 256 (S), M = 255 (C)
    if f is not None:
        wd[-1][:] = 255
        wd[-1][:, 0] = 256
    f = claim("d256_m256", wide_rows=True)  # D = M = 256 (S, S)
    if f is not None:
        wd[-1][:] = 256
    f = claim("one_strand_255", both=False)  # one strand alone at the C / S edge
    if f is not None:
        ss_len[f] = [Lf, Lf, 0, 0]
        ss_depth[f] = 255
    f = claim("one_strand_256", both=False, wide_rows=True)
    if f is not None:
        ss_len[f] = [0, 0, Lf, Lf]
        wd[-1][:] = 256
        wd[-1][:, 1] = 255
    f = claim("wide_max", wide_rows=True)  # 32767 on both strands: duplex depth 65534
    if f is not None:
        wd[-1][:] = rng.integers(30000, 32768, (4, stride)).astype(np.uint16)
        wd[-1][:, 2] = 32767
        we[-1][:] = rng.integers(0, 32768, (4, stride)).astype(np.uint16)
    f = claim("disagree")  # strands that disagree, with equal and with unequal quals
    if f is not None:
        ss_base[f, 0:2] = 1 + (np.arange(stride) % 2)
        ss_base[f, 2:4] = 4
        ss_qual[f, 2:4] = ss_qual[f, 1::-1][:, :]  # R1 reads sets (0, 3), R2 sets (1, 2)
        ss_qual[f, 2:4, ::2] = ss_qual[f, 2:4, ::2] ^ 0x10
    for k in range(3):  # a few more wide families with garbage rows
        claim("wide%d" % k, both=k != 1, wide_rows=True)
    seq[:min(F, 8), :, :8] = np.asarray([0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xCD, 0xEF], np.uint8)
    q = np.arange(256, dtype=np.uint8)
    if stride >= 258 and free:  # one kept family holds every quality byte, in QUAL and in aq / bq
        f = free.pop(0)
        notes["all_quals"] = f
        length[f, :] = (stride - 3) | 1
        ss_len[f] = length[f, 0]
        qual[f, :, :256] = q
        ss_qual[f, :, :256] = q[::-1]
    else:  # short rows: the 256 values spread over the leading bases of the kept families
        k = 0
        for f in kept:
            for d in range(2):
                n = int(length[f, d])
                take = min(n, 256 - k) if k < 256 else 0
                qual[f, d, :take] = q[k:k + take]
                ss_qual[f, d, :take] = q[k:k + take]
                ss_qual[f, 3 - d, :take] = q[k:k + take][::-1]
                k += take
            if k >= 256:
                break
    nl = rng.integers(1, 12, F)
    nl[:6] = [1, 2, 3, 4, 5, 253][:min(F, 6)]
    nl[-1] = 253
    if F >= 270:
        nl[8:8 + 253] = np.arange(1, 254)
    alphabet = np.frombuffer(b"ACGTNacgt0123456789:/-_", np.uint8)
    auxs = []
    if vector_tables:
        off = np.zeros(F + 1, np.int64)
        np.cumsum(nl, out=off[1:])
        names = bam.StringTable(alphabet[rng.integers(0, alphabet.shape[0], int(off[-1]))], off)
        m = rng.integers(1, 9, F)
        acgt = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 16 * F)].tobytes()
        for f in range(F):
            mi = b"RGZA\0MIZ%d\0" % (f * 7)
            auxs.append(mi + b"RXZ" + acgt[16 * f:16 * f + 8] + b"-" + acgt[16 * f + 8:16 * f + 8 + m[f]] + b"\0"
                        if f % 4 >= 2 else mi if f % 4 else b"")
    else:
        names = bam.StringTable.from_list([bytes(alphabet[rng.integers(0, alphabet.shape[0], int(n))]) for n in nl])
        for f in range(F):
            mi = b"RGZA\0MIZ%d\0" % (f * 7)
            rx = b"RXZ" + bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 8)]) + b"-" + \
                bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(rng.integers(1, 9)))]) + b"\0"
            auxs.append([b"", mi, mi + rx, mi + rx][f % 4])
    aux = bam.StringTable.from_list(auxs)
    W = len(wd)
    return BamRecInput(stride, status, length, seq, qual, filt, names, aux, ss_len, ss_base, ss_qual, ss_depth, ss_err,
                       wide, np.stack(wd) if W else np.zeros((0, 4, stride), np.uint16),
                       np.stack(we) if W else np.zeros((0, 4, stride), np.uint16), notes)


def records(x: BamRecInput, fams: np.ndarray, molecular: bool, tags: bool) -> "bam.OutRecordsBam":
    """Families `fams` (indices) as the R1 / R2 records bam.duplex_records would make of them: the
    consensus rows gathered, name and aux of the family for both mates, bam.consensus_tags' bytes."""
    fams = np.asarray(fams, np.int64)
    n = 2 * fams.shape[0]
    L = x.length[fams].reshape(-1).astype(np.int64)
    seq_off = np.zeros(n + 1, np.int64)
    seq_off[1:] = np.cumsum(L)
    codes = np.stack([x.seq >> 4, x.seq & 15], axis=-1).reshape(x.n_fam, 2, x.stride)
    row = 2 * np.repeat(fams, 2) + np.tile(np.arange(2), fams.shape[0])
    idx = np.repeat(row * x.stride - seq_off[:-1], L) + np.arange(int(seq_off[-1]), dtype=np.int64)
    seq, qual = codes.reshape(-1)[idx], x.qual.reshape(-1)[idx]
    two = np.repeat(fams, 2)
    names, aux = bam._take_table(x.names, two), bam._take_table(x.aux, two)
    tg = None
    if tags:
        cons = SimpleNamespace(length=x.length, ss={"len": x.ss_len, "base": x.ss_base, "qual": x.ss_qual,
                                                    "depth": x.ss_depth, "err": x.ss_err, "wide": x.ss_wide,
                                                    "wdepth": x.ss_wdepth, "werr": x.ss_werr})
        tg = bam.consensus_tags(cons, fams, molecular, 2)
    return bam.OutRecordsBam(
        flag=np.tile(np.asarray([77, 141], np.uint16), n // 2), tid=np.full(n, -1, np.int32),
        pos=np.full(n, -1, np.int32), mapq=np.zeros(n, np.uint8), next_tid=np.full(n, -1, np.int32),
        next_pos=np.full(n, -1, np.int32), tlen=np.zeros(n, np.int32), names=names, cig_off=np.zeros(n + 1, np.int64),
        cigar=np.zeros(0, np.uint32), seq_off=seq_off, seq=seq, qual=qual, aux=aux, aux2=tg)


HEADER = bam.BamHeader("@HD\tVN:1.6\tSO:unsorted\n", [], np.zeros(0, np.int64))


def host_bytes(recs: "bam.OutRecordsBam", tmp: str, tag: str = "h") -> bytes:
    """the records through the host BAM writer as a headerless fragment, gunzipped"""
    p = os.path.join(tmp, "%s.bam" % tag)
    w = bgzf.BamWriter(p, HEADER, 1, fragment="next")
    try:
        w.add(recs, 2)
    finally:
        w.close(2)
    return gzip.open(p).read() if os.path.getsize(p) else b""


def record_sizes(recs: "bam.OutRecordsBam") -> np.ndarray:
    """bytes of each record as encode_records lays it out"""
    L = np.diff(recs.seq_off)
    n = 36 + np.diff(recs.names.off) + 1 + (L + 1) // 2 + L + np.diff(recs.aux.off)
    return n + (np.diff(recs.aux2.off) if recs.aux2 is not None else 0)


def expected(x: BamRecInput, molecular: bool, tags: bool, with_filt: bool, tmp: str, tag: str = "e"):
    """-> (the kept families' record bytes, off int64 [F + 1]: where each family's start)"""
    keep = x.kept(with_filt)
    fams = np.nonzero(keep)[0]
    recs = records(x, fams, molecular, tags)
    data = host_bytes(recs, tmp, tag)
    per = np.zeros(x.n_fam, np.int64)
    per[fams] = record_sizes(recs).reshape(-1, 2).sum(axis=1)
    off = np.zeros(x.n_fam + 1, np.int64)
    np.cumsum(per, out=off[1:])
    assert int(off[-1]) == len(data)
    return data, off


def tables(x: BamRecInput):
    """-> (name buf, name off, aux buf, aux off) as contiguous arrays"""
    c = np.ascontiguousarray
    return c(x.names.buf, np.uint8), c(x.names.off, np.int64), c(x.aux.buf, np.uint8), c(x.aux.off, np.int64)

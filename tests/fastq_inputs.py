"""Fabricated consensus outputs for the device FASTQ path (csrc/bsdc_fastq.hip; bam.fastq_offsets):
the arrays a vote leaves -- status, len, packed seq, qual, the filter's filt -- and a family name
table, built so that every branch of the formatter is met at a small size, plus the yardstick: the
same families as OutRecordsBam for the host writer (bam.write_fastq -> format_fastq)."""
import gzip
import os
from dataclasses import dataclass

import numpy as np

from bsseqconsensusreads_amd import bam


@dataclass
class FastqInput:
    stride: int
    status: np.ndarray  # u8 [F]
    length: np.ndarray  # i32 [F, 2]
    seq: np.ndarray     # u8 [F, 2, stride / 2] packed nt16, high nibble first
    qual: np.ndarray    # u8 [F, 2, stride]
    filt: np.ndarray    # u8 [F] reason bits (0 = kept)
    names: "bam.StringTable"

    @property
    def n_fam(self) -> int:
        return int(self.status.shape[0])

    def kept(self, with_filt: bool) -> np.ndarray:
        k = (self.status & 1) != 0
        return k & (self.filt == 0) if with_filt else k


def random_names(rng, nl) -> "bam.StringTable":
    """names of the lengths nl out of one draw: the table of a batch too large for a draw per name"""
    alphabet = np.frombuffer(b"ACGTNacgt0123456789:/-_", np.uint8)
    off = np.zeros(nl.shape[0] + 1, np.int64)
    np.cumsum(nl, out=off[1:])
    return bam.StringTable(alphabet[rng.integers(0, alphabet.shape[0], int(off[-1]))], off)


def make(stride: int, n_fam: int = 300, seed: int = 0, written: str = "mixed", vector_names: bool = False) -> FastqInput:
    """vector_names: the name table by random_names (other names than the per-name draws give).
    written: "mixed" (unemitted and filtered families at the front, at the back and in runs),
    "none" (no family emitted), "all", "first_off" / "last_off" (only that family unemitted).
    Lengths 0, 1, 2, 3, 4, 5, an odd value and stride - 2 recur; name lengths 1..5, 254 and every
    length 1..254 once n_fam allows; every nt16 code and every quality byte 0..255 occur."""
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
        fl = rng.random(F) < 0.15
        fl[3:5] = True
        fl[-4:-2] = True
        fl[100:111] = True
        filt[fl] = rng.integers(1, 16, int(fl.sum())).astype(np.uint8)
    elif written == "none":
        status &= 0xFE
    elif written == "first_off":
        status[0] &= 0xFE
    elif written == "last_off":
        status[-1] &= 0xFE
    special = [0, 1, 2, 3, 4, 5, min(7, stride - 3) | 1, stride - 2]
    length = rng.integers(0, stride - 1, (F, 2)).astype(np.int32)
    for f in range(F):
        if f % 3 == 0:
            length[f, 0] = special[(f // 3) % len(special)]
        if f % 3 == 1:
            length[f, 1] = special[(f // 3 + 3) % len(special)]
    length = np.minimum(length, stride - 2)
    seq = rng.integers(0, 256, (F, 2, stride // 2)).astype(np.uint8)  # (every code, also past the lengths)
    qual = rng.integers(0, 256, (F, 2, stride)).astype(np.uint8)
    seq[:min(F, 8), :, :8] = np.asarray([0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xCD, 0xEF], np.uint8)
    q = np.arange(256, dtype=np.uint8)
    free = np.nonzero(((status & 1) != 0) & (filt == 0) & (np.arange(F) % 3 == 2))[0]
    if stride >= 258 and free.shape[0]:  # one kept family holds them all, in both files
        length[free[0], :] = (stride - 3) | 1
        qual[free[0], :, :256] = q
    else:  # short rows: the 256 values spread over the leading bases of consecutive families
        k = 0
        for f in range(F):
            for d in range(2):
                n = int(length[f, d])
                take = min(n, 256 - k) if k < 256 else 0
                qual[f, d, :take] = q[k:k + take]
                k += take
            if k >= 256:
                break
    nl = rng.integers(1, 12, F)
    nl[:6] = [1, 2, 3, 4, 5, 254][:min(F, 6)]
    nl[-1] = 254
    if F >= 270:
        nl[8:8 + 254] = np.arange(1, 255)
    if vector_names:
        return FastqInput(stride, status, length, seq, qual, filt, random_names(rng, nl))
    alphabet = np.frombuffer(b"ACGTNacgt0123456789:/-_", np.uint8)
    names = bam.StringTable.from_list([bytes(alphabet[rng.integers(0, alphabet.shape[0], int(n))]) for n in nl])
    return FastqInput(stride, status, length, seq, qual, filt, names)


def gather_index(fams, L, seq_off, stride) -> np.ndarray:
    """where the bases of records 2k, 2k + 1 = rows (fams[k], 0), (fams[k], 1) lie in a flattened [F, 2, stride] array"""
    row = 2 * np.repeat(np.asarray(fams, np.int64), 2) + np.tile(np.arange(2), fams.shape[0])
    return np.repeat(row * stride - seq_off[:-1], L) + np.arange(int(seq_off[-1]), dtype=np.int64)


def records(x: FastqInput, fams: np.ndarray) -> "bam.OutRecordsBam":
    """Families `fams` (indices) as the R1 / R2 records duplex_records would make of them."""
    fams = np.asarray(fams, np.int64)
    n = 2 * fams.shape[0]
    L = x.length[fams].reshape(-1).astype(np.int64)
    seq_off = np.zeros(n + 1, np.int64)
    seq_off[1:] = np.cumsum(L)
    codes = np.stack([x.seq >> 4, x.seq & 15], axis=-1).reshape(x.n_fam, 2, x.stride)
    idx = gather_index(fams, L, seq_off, x.stride)
    seq, qual = codes.reshape(-1)[idx], x.qual.reshape(-1)[idx]
    names = bam._take_table(x.names, np.repeat(fams, 2))
    empty = bam.StringTable(np.zeros(0, np.uint8), np.zeros(n + 1, np.int64))
    return bam.OutRecordsBam(
        flag=np.tile(np.asarray([77, 141], np.uint16), n // 2), tid=np.full(n, -1, np.int32),
        pos=np.full(n, -1, np.int32), mapq=np.zeros(n, np.uint8), next_tid=np.full(n, -1, np.int32),
        next_pos=np.full(n, -1, np.int32), tlen=np.zeros(n, np.int32), names=names, cig_off=np.zeros(n + 1, np.int64),
        cigar=np.zeros(0, np.uint32), seq_off=seq_off, seq=seq, qual=qual, aux=empty)


def host_text(x: FastqInput, fams: np.ndarray, tmp: str, tag: str = "h"):
    """-> (file 1's text, file 2's) of the families through the host writer (bam.write_fastq)."""
    p = [os.path.join(tmp, "%s%d.fq.gz" % (tag, d)) for d in (1, 2)]
    bam.write_fastq(p[0], p[1], records(x, fams), level=1)
    return tuple(gzip.open(q).read() for q in p)


def name_table(x: FastqInput):
    off = np.ascontiguousarray(x.names.off, np.int64)
    return np.ascontiguousarray(x.names.buf, np.uint8), off


def text_blocks(seed: int = 5, n: int = 3) -> bytes:
    """n whole BGZF blocks of FASTQ-like text."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    k = 0
    while len(out) < n * 65280:
        L = int(rng.integers(50, 151))
        out += b"@x:%d/1\n" % k + bytes(np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, L)]) + b"\n+\n" + \
            bytes((33 + rng.integers(2, 46, L)).astype(np.uint8)) + b"\n"
        k += 1
    return bytes(out[:n * 65280])


def crc_contents() -> dict:
    """name -> bytes (whole blocks): the CRC32 test's contents."""
    rng = np.random.default_rng(17)
    rand = rng.integers(0, 256, 3 * 65280).astype(np.uint8).tobytes()
    out = {"zeros": b"\0" * (3 * 65280), "ff": b"\xff" * (3 * 65280), "ramp": bytes(range(256)) * (3 * 255),
           "random": rand, "fastq": text_blocks()}
    base = rand[:65280]
    for name, at in (("byte0", 0), ("last", 65279), ("seam254", 254), ("seam255", 255), ("dword", 1020 + 3),
                     ("dword_next", 1020 + 4)):
        b = bytearray(base)
        b[at] ^= 0x5A
        out["pair_" + name] = base + bytes(b)
    return out

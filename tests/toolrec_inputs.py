"""Fabricated records for the tool-stage record writer (csrc/bsdc_toolrec.hip) in named
sets, each aimed at one kind of edge: `cigar`, `lens`, `place`, `aux`, `bin` and `counts_N`.  A record
is a dict as tests/toolrec_ref.record_bytes takes it; build() lays the set out as the library sees
it: the input records (RawRecords), the converted mask, and a stage dump with one slot per record
(slot starts at multiples of 4, round4(len + 2) long, as a family batch's)."""
from dataclasses import dataclass

import numpy as np

from bsseqconsensusreads_amd import records as R

M, I, D, N, S, EQ, X = 0, 1, 2, 3, 4, 7, 8
NAMES = ("cigar", "lens", "place", "aux", "bin", "counts_0", "counts_1", "counts_63", "counts_64", "counts_65")
MAX_LEN = 65527 + 2  # the longest record a family slot holds (batch.py) with both tools' bases


def op(n, k):
    return (n << 4) | k


def rec(rng, i, cigar, tags, L=None, name=None, aux=b"", pos=None, flag=None):
    L = int(rng.integers(1, 40)) if L is None else L
    return dict(name=("q%d" % i).encode() if name is None else name, flag=(99, 147, 83, 163)[i % 4] if flag is None else flag,
                ref_id=i % 3, mapq=int(rng.integers(0, 61)), next_ref_id=(i + 1) % 3, next_pos=int(rng.integers(0, 1 << 20)),
                tlen=int(rng.integers(-500, 500)), cigar=list(cigar), aux=bytes(aux),
                pos=int(rng.integers(0, 1 << 20)) if pos is None else pos, seq=rng.integers(0, 16, L).astype(np.uint8),
                qual=rng.integers(0, 256, L).astype(np.uint8), tags=tags)


def _aux(*tags):
    return R.encode_aux([tuple(t) for t in tags])


MI = ("MI", "Z", "17/A")
RX = ("RX", "Z", "ACGT-TTGA")


def make(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    out = []
    if name == "cigar":
        i = 0
        for t in (0, 4, 6, 7, 15, 8, 12, 1, 5, 13):  # the values the kernels write, then extend-only ones
            for clips in ((0, 0), (3, 0), (0, 2), (5, 6)):
                for last in (1, 9):
                    ops = ([op(clips[0], S)] if clips[0] else []) + [op(20, M), op(last, M)] + ([op(clips[1], S)] if clips[1] else [])
                    out.append(rec(rng, i, ops, t, aux=_aux(MI)))
                    i += 1
        out.append(rec(rng, i, [op(1, M)], 7, L=1))                       # 1M, RD: ends as 1M
        out.append(rec(rng, i + 1, [op(4, S), op(1, M), op(4, S)], 7, L=1))
        out.append(rec(rng, i + 2, [op(1, M)], 15, L=2))
        out.append(rec(rng, i + 3, [op(10, EQ), op(1, X), op(5, EQ)], 6))
        out.append(rec(rng, i + 4, [op(10, EQ), op(1, X)], 7))             # RD drops the 1X
        out.append(rec(rng, i + 5, [op(10, M), op(2, I), op(5, M), op(3, D), op(7, M), op(100, N), op(4, M)], 0))
        out.append(rec(rng, i + 6, [op(2, S), op(10, M), op(2, I), op(5, M), op(1, D)], 7))  # RD drops the 1D
        out.append(rec(rng, i + 7, [op(10, M), op(1, I)], 7))              # RD drops an op that holds no reference base
        out.append(rec(rng, i + 8, [], 0, L=3, flag=77))                   # no cigar at all
        out.append(rec(rng, i + 9, [], 7, L=1))
        out.append(rec(rng, i + 10, [op(3, S)], 4, L=1))
    elif name == "lens":
        for i, L in enumerate((1, 2, 15, 16, 17, 255, 256, 257, MAX_LEN, 3)):
            out.append(rec(rng, i, [op(max(L - 1, 1), M)], (0, 6, 7, 15)[i % 4], L=L, aux=_aux(MI, RX)))
    elif name == "place":
        i = 0
        for nl in list(range(1, 9)) + [254]:
            for t in (0, 6, 15):
                for al in (0, 1, 2, 3):
                    aux = _aux(MI) + b"XAZ" + b"a" * (al - 1) + b"\0" if al else b""  # 0, 12, 13, 14 bytes
                    out.append(rec(rng, i, [op(30, M)], t, L=int(rng.integers(1, 9)), name=b"n" * nl, aux=aux))
                    i += 1
        big = b"XBBC" + (70000).to_bytes(4, "little") + rng.integers(0, 256, 70000).astype(np.uint8).tobytes()
        out.append(rec(rng, i, [op(30, M)], 7, L=33, aux=_aux(MI) + big + _aux(("RD", "C", 0))))  # spans a BGZF block
        out.append(rec(rng, i + 1, [op(30, M)], 0, L=5, aux=b""))
    elif name == "aux":
        rd, la = ("RD", "C", 1), ("LA", "C", 1)
        arr = b"XBBC" + (6).to_bytes(4, "little") + b"RDCLAC"      # a B:C array whose payload reads RDC LAC
        zs = b"XZZRDC-LAC\0"                                        # a Z string that holds both
        blocks = [_aux(rd, MI, RX), _aux(MI, rd, RX), _aux(MI, RX, rd), _aux(la, MI, RX), _aux(MI, la, RX), _aux(MI, RX, la),
                  _aux(rd, la, MI), _aux(MI, la, RX, rd), _aux(rd, la), arr + _aux(MI), _aux(MI) + zs, arr + zs,
                  _aux(rd) + arr + _aux(la) + zs, _aux(("RD", "i", 70000), MI, ("LA", "Z", "x")), _aux(MI, ("XS", "f", 1.5)),
                  _aux(MI, ("LA", "Z", "x")), _aux(("RD", "c", -1), MI)]  # tags a decoder of integers reads as absent
        i = 0
        for b in blocks:
            for t in (0, 4, 6, 7, 15):
                out.append(rec(rng, i, [op(12, M)], t, L=int(rng.integers(2, 20)), aux=b))
                i += 1
    elif name == "bin":
        out.append(rec(rng, 0, [op(10, M)], 0, pos=0))
        out.append(rec(rng, 1, [op(10, M)], 6, pos=(1 << 14) - 5))          # crosses a 16 KiB boundary
        out.append(rec(rng, 2, [op(10, M)], 0, pos=(1 << 14) - 10))         # ends exactly at it
        out.append(rec(rng, 3, [op(5, M), op(200, N), op(5, M)], 6, pos=(1 << 17) - 100))  # a 128 KiB boundary
        out.append(rec(rng, 4, [op(5, M), op(3000, D), op(5, M)], 7, pos=(1 << 20) - 7))
        out.append(rec(rng, 5, [op(5, I)], 0, pos=12345))                    # reference length 0
        out.append(rec(rng, 6, [], 0, pos=-1, flag=77))                      # unplaced: bin 4680
        out.append(rec(rng, 7, [op(1, M)], 7, pos=(1 << 14) - 1, L=1))
        out.append(rec(rng, 8, [op(9, M)], 8, pos=(1 << 14) - 9))           # the appended M crosses
        out.append(rec(rng, 9, [op(100, M)], 0, pos=(1 << 29) - 50))
    elif name.startswith("counts_"):
        for i in range(int(name.split("_")[1])):
            out.append(rec(rng, i, [op(2, S), op(25, M)], (0, 4, 6, 7, 15)[i % 5], aux=_aux(MI, RX) if i % 3 else b""))
    else:
        raise KeyError(name)
    return out


@dataclass
class Case:
    recs: list
    raw: R.RawRecords
    conv: np.ndarray
    rec_off: np.ndarray
    dump_pos: np.ndarray
    dump_len: np.ndarray
    dump_tags: np.ndarray
    dump_seq: np.ndarray
    dump_qual: np.ndarray


def build(recs, fill=0xA5) -> Case:
    b = R._Builder()
    e = np.zeros(0, np.uint8)
    for r in recs:
        b.add(r["name"], r["flag"], r["ref_id"], 0, r["mapq"], r["cigar"], e, e, r["next_ref_id"], r["next_pos"], r["tlen"],
              r["aux"], tags=[])
    raw = b.finish()
    n = len(recs)
    L = np.asarray([len(r["seq"]) for r in recs], np.int64)
    size = (L + 2 + 3) // 4 * 4
    rec_off = (np.cumsum(size) - size).astype(np.uint32)
    n_dump = int(size.sum()) + 16
    ds, dq = np.full(n_dump, fill, np.uint8), np.full(n_dump, fill ^ 0xFF, np.uint8)
    for r, o in zip(recs, rec_off):
        ds[int(o):int(o) + len(r["seq"])] = r["seq"]
        dq[int(o):int(o) + len(r["seq"])] = r["qual"]
    return Case(recs, raw, np.asarray([bool(r["tags"] & 2) for r in recs], bool), rec_off,
                np.asarray([r["pos"] for r in recs], np.int32).reshape(n), L.astype(np.uint16),
                np.asarray([r["tags"] for r in recs], np.uint8).reshape(n), ds, dq)

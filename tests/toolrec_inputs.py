"""Fabricated records for the tool-stage record writer (csrc/bsdc_toolrec.hip) in named
sets, each aimed at one kind of edge: `cigar`, `lens`, `place`, `aux`, `bin`, `counts_N`, `longcigar`
(more ops than a wavefront has lanes), `hugeref` (reference lengths past 2^32), `phases` (every
section's source phase against every destination phase) and `tight_L` (the dump ends with the last
record's L bases).  A record is a dict as tests/toolrec_ref.record_bytes takes it; build() lays the
set out as the library sees it: the input records (RawRecords), the converted mask, and a stage dump
with one slot per record (slot starts at multiples of 4, round4(len + 2) long, as a family batch's).
carry_case(), shared_case() and far_case() build their tables as arrays (Case.tab): batches too
large for a per-record loop, and tables no RawRecords gives (several records on the same bytes)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from bsseqconsensusreads_amd import _lib, toolrec
from bsseqconsensusreads_amd import records as R

M, I, D, N, S, EQ, X = 0, 1, 2, 3, 4, 7, 8
REF_OPS = (M, D, N, EQ, X)
NAMES = ("cigar", "lens", "place", "aux", "bin", "counts_0", "counts_1", "counts_63", "counts_64", "counts_65",
         "longcigar", "hugeref", "phases", "counts_1023", "counts_1024", "counts_1025",
         "tight_1", "tight_2", "tight_3", "tight_4", "tight_5", "tight_8", "tight_9", "tight_11")
TIGHT = (1, 2, 3, 4, 5, 8, 9, 11)  # (11: eight codes of packed SEQ reach into the dump's last, partial dword)
MAX_LEN = 65527 + 2  # the longest record a family slot holds (batch.py) with both tools' bases
MAX_OPS = 65533      # the most ops a table entry holds: n_cigar_op <= 65535 with both added 1M
MAX_OP_LEN = (1 << 28) - 1
LONG_OPS = (63, 64, 65, 128, 129, 1000)
PHASES = dict(nl=(1, 2, 3, 4), L=(7, 8, 9, 15, 16, 17, 23, 24), al=(0, 5, 6, 7, 8, 9), tags=(0, 7))
SCAN_GROUP = 1024    # the records one workgroup of the offset scan takes (bsdc_devtext.h kFamPerGroup)
SCAN_TILE = 256      # the workgroups' sums k_scan_scan takes in one round
CARRY_COUNTS = (SCAN_TILE * SCAN_GROUP, SCAN_TILE * SCAN_GROUP + 1, SCAN_TILE * SCAN_GROUP + SCAN_GROUP + 1)


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
    elif name == "longcigar":
        # more ops than lanes: a lane of k_toolrec_sizes takes ops lane, lane + 64, ..; the kinds are
        # random, so reference ops sit in every lane residue; the prepended 1M (tags 6, 7, 15) and a
        # last op RD drops (length 1) or shortens (tag 7, 15) move which lane reads which op.  The
        # position puts the first 64 ops of the NEW cigar just before a 16 KiB boundary: only the
        # ops a second round reads carry the record over it (set_edges() in the host test)
        i = 0
        for n in LONG_OPS + (MAX_OPS,):
            for t in (0, 6, 7, 15):
                for last in (1, 5):
                    if n == MAX_OPS and (t, last) not in ((0, 5), (7, 1), (15, 5)):
                        continue  # (65533, 65533 and 65535 ops out)
                    kinds = np.asarray((M, I, D, N, EQ, X), np.uint32)[rng.integers(0, 6, n)]
                    ops = ((rng.integers(1, 4, n).astype(np.uint32) << 4) | kinds).tolist()
                    ops[-2:] = [op(2, M), op(last, M)]  # (whichever of them RD leaves holds reference bases)
                    ops = [op(3, S)] + ops + ([op(2, S)] if i & 1 else [])
                    r = rec(rng, i, ops, t, L=int(rng.integers(1, 40)), aux=_aux(MI))
                    r["pos"] = ((1 + i) << 14) - ref_len(new_ops(r)[:64])
                    out.append(r)
                    i += 1
    elif name == "hugeref":
        big = op(MAX_OP_LEN, N)
        # the 64-bit add alone: at most one op a lane, every lane's share below 2^32
        out.append(rec(rng, 0, [big] * 20, 0, pos=0))
        out.append(rec(rng, 1, [op(1, M)] + [big] * 17 + [op(1, M)], 15, pos=1000))
        out.append(rec(rng, 2, [big] * 64, 6, pos=0))
        # the high half crosses lanes: the ops at one lane residue sum past 2^32 on their own, the
        # others are insertions, and the low 32 bits of the length stay small; lane 1 writes the bin,
        # so with the sum in lane 0 or 5 it has the high half from the shuffle alone
        i = 3
        for res, low, pos, t in ((0, 100, 0, 0), (0, 5000, 1000, 0), (5, 70000, 0, 0), (4, 100, 1000, 6), (0, 100, 1000, 8)):
            ops = [op(1, I)] * (17 * 64)
            for k in range(17):
                ops[64 * k + res] = big
            rest = (1 << 32) + low - 17 * MAX_OP_LEN - (1 if t & 6 else 0) - (1 if t & 8 else 0)
            assert rest < 0  # 17 ops at the limit pass 2^32 already: take the surplus off the last
            ops[64 * 16 + res] = op(MAX_OP_LEN + rest, N)
            out.append(rec(rng, i, ops, t, pos=pos, aux=_aux(MI)))
            i += 1
    elif name == "phases":
        # every (name length, L, aux length, tags) at every residue of the record's start mod 4: a
        # filler record in front of each brings the running total to the residue wanted
        letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
        total = i = 0
        for nl in PHASES["nl"]:
            for L in PHASES["L"]:
                for al in PHASES["al"]:
                    for t in PHASES["tags"]:
                        for want in range(4):
                            fl = 1 + (want - total - size_of(dict(name=b"f", cigar=[op(5, M)], seq=[0] * 3, aux=b"", tags=0))) % 4
                            f = rec(rng, i, [op(5, M)], 0, L=3, name=bytes(letters[rng.integers(0, 26, fl)]))
                            aux = b"XAZ" + bytes(letters[rng.integers(0, 26, al - 4)]) + b"\0" if al else b""
                            r = rec(rng, i + 1, [op(L, M)], t, L=L, name=bytes(letters[rng.integers(0, 26, nl)]), aux=aux)
                            total += size_of(f)
                            assert total % 4 == want
                            total += size_of(r)
                            out += [f, r]
                            i += 2
    elif name.startswith("tight_"):
        for i in range(5):
            out.append(rec(rng, i, [op(20, M)], (0, 6, 7, 15)[i % 4], aux=_aux(MI)))
        L = int(name.split("_")[1])
        out.append(rec(rng, 5, [op(L, M)], 7 if L & 1 else 0, L=L, name=b"t" * (1 + L % 4)))
    else:
        raise KeyError(name)
    return out


def new_ops(r):
    """the record's cigar after the tools, as the restatement's new_cigar has it"""
    ops = list(r["cigar"])
    if ops and (ops[0] & 15) == S:
        ops = ops[1:]
    if ops and (ops[-1] & 15) == S:
        ops = ops[:-1]
    t = r["tags"]
    if t & 6:
        ops = [op(1, M)] + ops
    if (t & 3) == 3:
        if (ops[-1] >> 4) > 1:
            ops[-1] -= 1 << 4
        else:
            ops.pop()
    if t & 8:
        ops = ops + [op(1, M)]
    return ops


def ref_len(ops):
    return sum(int(o) >> 4 for o in ops if (int(o) & 15) in REF_OPS)


def size_of(r):
    """the bytes of a record by the layout rule (aux without RD / LA)"""
    L = len(r["seq"])
    return 36 + len(r["name"]) + 1 + 4 * len(new_ops(r)) + (L + 1) // 2 + L + len(r["aux"]) + (8 if r["tags"] & 2 else 0)


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
    tab: Optional[toolrec.Tables] = None  # the tables as arrays, where no RawRecords gives them (recs, raw: None)

    @property
    def n(self) -> int:
        return int(self.dump_len.shape[0])

    def tables(self) -> toolrec.Tables:
        return self.tab if self.tab is not None else toolrec.tables(self.raw, np.arange(self.raw.n), self.conv)


def build_named(name) -> Case:
    """build() of make(name), laid out as the set's name asks"""
    return build(make(name), slack=0 if name.startswith("tight_") else 16)


def build(recs, fill=0xA5, slack=16) -> Case:
    """slack: spare bytes after the last slot.  slack=0 ends the dump with the last record: its slot
    is round4(len) long, so that a length of 4 or 8 ends with the dump's last byte and no dword
    lies behind any length's last base (the dump stays a multiple of 4 long)."""
    b = R._Builder()
    e = np.zeros(0, np.uint8)
    for r in recs:
        b.add(r["name"], r["flag"], r["ref_id"], 0, r["mapq"], r["cigar"], e, e, r["next_ref_id"], r["next_pos"], r["tlen"],
              r["aux"], tags=[])
    raw = b.finish()
    n = len(recs)
    L = np.asarray([len(r["seq"]) for r in recs], np.int64)
    size = (L + 2 + 3) // 4 * 4
    if slack == 0 and n:
        size[-1] = (L[-1] + 3) // 4 * 4
    rec_off = (np.cumsum(size) - size).astype(np.uint32)
    n_dump = int(size.sum()) + slack
    ds, dq = np.full(n_dump, fill, np.uint8), np.full(n_dump, fill ^ 0xFF, np.uint8)
    for r, o in zip(recs, rec_off):
        ds[int(o):int(o) + len(r["seq"])] = r["seq"]
        dq[int(o):int(o) + len(r["seq"])] = r["qual"]
    return Case(recs, raw, np.asarray([bool(r["tags"] & 2) for r in recs], bool), rec_off,
                np.asarray([r["pos"] for r in recs], np.int32).reshape(n), L.astype(np.uint16),
                np.asarray([r["tags"] for r in recs], np.uint8).reshape(n), ds, dq)


# ---- cases whose tables are built as arrays

_LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
_KINDS = np.asarray((M, I, D, N, EQ, X), np.uint32)


def _tab_case(rng, nl, names, n_cig, cigar, al, aux_off, aux, L, tags, off_of=None) -> Case:
    """A Case of table columns: record r's name is the next nl[r] bytes of `names` and its ops the
    next n_cig[r] of `cigar` (off_of: the record whose bytes r points at instead), its aux bytes
    aux[aux_off[r]:][:al[r]]; the fixed fields, the positions and a dump slot per record are random."""
    n = int(nl.shape[0])
    tab = np.zeros(n, _lib.TOOLREC_REC)
    nl, n_cig, al, L = (np.asarray(a, np.int64) for a in (nl, n_cig, al, L))
    tab["name_len"], tab["n_cig"], tab["aux_len"], tab["aux_off"] = nl, n_cig, al, aux_off
    tab["name_off"], tab["cig_off"] = np.cumsum(nl) - nl, np.cumsum(n_cig) - n_cig
    if off_of is not None:
        tab["name_off"], tab["cig_off"] = tab["name_off"][off_of], tab["cig_off"][off_of]
    tab["ref_id"], tab["next_ref_id"] = rng.integers(-1, 3, n), rng.integers(-1, 3, n)
    tab["next_pos"], tab["tlen"] = rng.integers(-1, 1 << 28, n), rng.integers(-500, 500, n)
    tab["flag"], tab["mapq"] = rng.integers(0, 1 << 16, n), rng.integers(0, 256, n)
    size = (L + 2 + 3) // 4 * 4
    n_dump = int(size.sum()) + 16
    aux = np.concatenate([aux, np.zeros((-int(aux.shape[0])) % 4 or (4 if aux.shape[0] == 0 else 0), np.uint8)])
    t = toolrec.Tables(tab, np.ascontiguousarray(names if names.shape[0] else np.zeros(1, np.uint8)),
                       np.ascontiguousarray(cigar if cigar.shape[0] else np.zeros(1, np.uint32), np.uint32), aux)
    tags = np.asarray(tags, np.uint8)
    return Case(None, None, (tags & 2) != 0, (np.cumsum(size) - size).astype(np.uint32),
                rng.integers(-1, 1 << 28, n).astype(np.int32), L.astype(np.uint16), tags,
                rng.integers(0, 256, n_dump).astype(np.uint8), rng.integers(0, 256, n_dump).astype(np.uint8), t)


def _small_columns(rng, n):
    """minimal records: name 1..3 bytes, 0..2 ops, L 1..6, aux 0 or 4 bytes (XA:C), the tags cycling"""
    nl, n_cig, L, has = rng.integers(1, 4, n), rng.integers(0, 3, n), rng.integers(1, 7, n), rng.integers(0, 2, n)
    tot = int(n_cig.sum())
    cigar = ((rng.integers(1, 21, tot).astype(np.uint32) << 4) | _KINDS[rng.integers(0, 6, tot)]).astype(np.uint32)
    k = int(has.sum())
    aux = np.tile(np.frombuffer(b"XAC\0", np.uint8), k)
    aux[3::4] = rng.integers(0, 256, k)
    tags = np.asarray((0, 6, 7, 15, 8, 4, 12), np.uint8)[np.arange(n) % 7]
    return nl, n_cig, cigar, 4 * has, aux, L, tags


def carry_case(n) -> Case:
    """n minimal records, vectorised: for the offset scan past one tile of workgroup sums"""
    rng = np.random.default_rng(n)
    nl, n_cig, cigar, al, aux, L, tags = _small_columns(rng, n)
    return _tab_case(rng, nl, _LETTERS[rng.integers(0, 26, int(nl.sum()))], n_cig, cigar, al, np.cumsum(al) - al, aux, L, tags)


def scan_groups(n):
    return (n + SCAN_GROUP - 1) // SCAN_GROUP


def shared_case(n=200) -> Case:
    """n records whose table entries all point at record 0's name (8 bytes), ops (3) and aux bytes
    (40), each with a dump slot of its own: bsdc_toolrec_bytes_bound counts the shared bytes once,
    the records hold them n times, so a destination of exactly the bound ends inside the records.
    The dump's size is chosen so that the bound falls inside a record, at 2 mod 4."""
    arr = b"XBBC" + (24).to_bytes(4, "little")
    for pad in range(0, 256, 4):
        rng = np.random.default_rng(200)
        aux = np.frombuffer(_aux(MI) + arr + rng.integers(0, 256, 24).astype(np.uint8).tobytes(), np.uint8)
        one = np.ones(n, np.int64)
        c = _tab_case(rng, 8 * one, _LETTERS[rng.integers(0, 26, 8 * n)], 3 * one,
                      np.tile(np.asarray([op(10, M), op(2, I), op(5, M)], np.uint32), n), 40 * one, 0 * one, aux,
                      rng.integers(1, 31, n), np.asarray((0, 6, 7, 15), np.uint8)[np.arange(n) % 4],
                      off_of=np.zeros(n, np.int64))
        c.dump_seq, c.dump_qual = (np.concatenate([a, a[:pad]]) for a in (c.dump_seq, c.dump_qual))
        c.tab.names, c.tab.cigar = c.tab.names[:8].copy(), c.tab.cigar[:3].copy()
        cap = c.tab.bound(c.dump_seq.shape[0])
        off = np.concatenate([[0], np.cumsum(layout_sizes(c))])
        if cap % 4 == 2 and ((off > cap - 4) & (off < cap + 4)).sum() == 0:
            return c
    raise AssertionError("no dump size puts the bound inside a record at 2 mod 4")


def far_case(n=270, aux_len=1 << 24) -> Case:
    """n minimal records that share one aux block of the limit's size (a B:C array): the records
    pass 2^31 and 2^32 bytes in all"""
    rng = np.random.default_rng(n)
    nl, n_cig, cigar, _, _, L, tags = _small_columns(rng, n)
    nl = 1 + np.arange(n) % 3
    names = np.concatenate([(33 + (np.arange(w) * 7 + i // 3) % 94).astype(np.uint8) for i, w in enumerate(nl)])
    aux = np.concatenate([np.frombuffer(b"XBBC" + (aux_len - 8).to_bytes(4, "little"), np.uint8),
                          rng.integers(0, 256, aux_len - 8).astype(np.uint8)])
    return _tab_case(rng, nl, names, n_cig, cigar, np.full(n, aux_len), np.zeros(n, np.int64), aux, L, tags)


def layout_sizes(c: Case) -> np.ndarray:
    """the records' sizes by the layout rule, in numpy: 36 + name + NUL + 4 per op of the new cigar
    + packed SEQ + QUAL + aux + RD and LA of a converted record"""
    e = c.tables().tab
    t, n_in, L = c.dump_tags.astype(np.int64), e["n_cig"].astype(np.int64), c.dump_len.astype(np.int64)
    last = np.ones(c.n, np.int64)
    has = n_in > 0
    last[has] = c.tables().cigar[e["cig_off"][has] + n_in[has] - 1] >> 4
    nc = ((t & 6) != 0).astype(np.int64) + n_in - (((t & 3) == 3) & (last <= 1)) + ((t & 8) != 0)
    return 36 + e["name_len"].astype(np.int64) + 1 + 4 * nc + (L + 1) // 2 + L + e["aux_len"].astype(np.int64) + 8 * ((t & 2) != 0)


def record_of(c: Case, r, aux=None):
    """record r of a Case as the dict tests/toolrec_ref.record_bytes takes (aux: in place of its own)"""
    t = c.tables()
    e = t.tab[r]
    o, L = int(c.rec_off[r]), int(c.dump_len[r])
    no, co, ao = int(e["name_off"]), int(e["cig_off"]), int(e["aux_off"])
    return dict(name=t.names[no:no + int(e["name_len"])].tobytes(), flag=int(e["flag"]), ref_id=int(e["ref_id"]),
                mapq=int(e["mapq"]), next_ref_id=int(e["next_ref_id"]), next_pos=int(e["next_pos"]), tlen=int(e["tlen"]),
                cigar=[int(x) for x in t.cigar[co:co + int(e["n_cig"])]],
                aux=t.aux[ao:ao + int(e["aux_len"])].tobytes() if aux is None else aux, pos=int(c.dump_pos[r]),
                seq=c.dump_seq[o:o + L], qual=c.dump_qual[o:o + L], tags=int(c.dump_tags[r]))

"""Raw-DEFLATE blocks for the BGZF inflate (csrc/bsdc_inflate.hip: the kernel and its host twin),
each with the isize and the bytes it promises.  Valid ones come from Python's zlib (wbits -15) or
from the small assembler below where zlib's deflate never writes the case (distance 32768, chosen
repeat codes); corrupt ones are valid ones with bits edited, one per status code, each of which
zlib rejects too (or inflates to another size than the isize claimed).  `ref()` is zlib's answer.
"""
from __future__ import annotations

import functools
import heapq
import zlib
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from bsseqconsensusreads_amd import _lib as L


@dataclass
class Block:
    name: str
    comp: bytes
    isize: int
    want: Optional[bytes]  # the bytes (valid blocks); None: corrupt
    code: int = 0          # the status expected


def ref(comp: bytes) -> bytes:
    """zlib's inflate of a raw stream; raises zlib.error on a corrupt or incomplete one."""
    d = zlib.decompressobj(-15)
    out = d.decompress(comp)
    if not d.eof:
        raise zlib.error("incomplete stream")
    return out


def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


# ---- a DEFLATE assembler ------------------------------------------------------------------------
class BitW:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v: int, n: int):  # n bits, least significant first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c: int, n: int):  # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            self.put((c >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self) -> bytes:
        self.align()
        return bytes(self.out)


def canon(lens: Sequence[int]) -> List[int]:
    """canonical codes of the lengths (RFC 1951 3.2.2)."""
    cnt = [0] * 17
    for x in lens:
        cnt[x] += 1
    cnt[0] = 0
    nxt, c = [0] * 17, 0
    for b in range(1, 17):
        c = (c + cnt[b - 1]) << 1
        nxt[b] = c
    out = []
    for x in lens:
        out.append(nxt[x] if x else 0)
        nxt[x] += 1 if x else 0
    return out


def huff_lens(freq: Sequence[int]) -> List[int]:
    """plain Huffman code lengths (no limit; the callers' alphabets stay within theirs)."""
    h = [(f, i, (i,)) for i, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(h) == 1:
        lens[h[0][1]] = 1
        return lens
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        for i in a[2] + b[2]:
            lens[i] += 1
        heapq.heappush(h, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    return lens


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def put_tokens(w: BitW, toks, lit_lens, dist_lens):
    """tokens: ("L", byte) | ("M", length, distance) | ("E",) end of block | ("S", lit/len symbol)
    | ("D", length, distance symbol, extra bits' value): a raw symbol."""
    lc, dc = canon(lit_lens), canon(dist_lens)

    def sym(s):
        assert lit_lens[s], s
        w.code(lc[s], lit_lens[s])

    def length(n):
        k = max(i for i in range(29) if LEN_BASE[i] <= n) if n < 258 else 28
        sym(257 + k)
        w.put(n - LEN_BASE[k], LEN_EXTRA[k])

    for t in toks:
        if t[0] == "L":
            sym(t[1])
        elif t[0] == "E":
            sym(256)
        elif t[0] == "S":
            sym(t[1])
        elif t[0] == "M":
            length(t[1])
            k = max(i for i in range(30) if DIST_BASE[i] <= t[2])
            assert dist_lens[k]
            w.code(dc[k], dist_lens[k])
            w.put(t[2] - DIST_BASE[k], DIST_EXTRA[k])
        else:
            length(t[1])
            w.code(dc[t[2]], dist_lens[t[2]])
            w.put(t[3], DIST_EXTRA[t[2]] if t[2] < 30 else 0)


def fixed_block(w: BitW, toks, final=True):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_tokens(w, toks, FIXED_LIT, FIXED_DIST)


def stored_block(w: BitW, data: bytes, final=True, nlen: Optional[int] = None):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
    w.out += data


def dynamic_block(w: BitW, lit_lens, dist_lens, toks, cl_seq=None, cl_lens=None, final=True, hlit=None, hdist=None):
    """cl_seq: the code-length symbols as (symbol, extra value) -- default: every length as itself;
    cl_lens: the code-length code's lengths -- default: Huffman over cl_seq's symbols."""
    hlit = len(lit_lens) if hlit is None else hlit
    hdist = len(dist_lens) if hdist is None else hdist
    if cl_seq is None:
        cl_seq = [(x, 0) for x in list(lit_lens) + list(dist_lens)]
    if cl_lens is None:
        f = [0] * 19
        for s, _ in cl_seq:
            f[s] += 1
        if sum(1 for x in f if x) == 1:  # (a one-symbol code-length code is incomplete: add a second)
            f[0 if not f[0] else 1] += 1
        cl_lens = huff_lens(f)
        assert max(cl_lens) <= 7
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    hclen = max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]] or k < 4)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_lens[CL_ORDER[k]], 3)
    cc = canon(cl_lens)
    for s, e in cl_seq:
        assert cl_lens[s], s
        w.code(cc[s], cl_lens[s])
        if s >= 16:
            w.put(e, {16: 2, 17: 3, 18: 7}[s])
    put_tokens(w, toks, list(lit_lens) + [0] * (288 - len(lit_lens)), list(dist_lens) + [0] * (32 - len(dist_lens)))


def _rng(*k):
    return np.random.default_rng([91, *k])


def _bamlike(n: int, seed: int = 0) -> bytes:
    """record-like bytes: a small alphabet, repeated fields, some noise."""
    rng = _rng(1, seed)
    words = [rng.integers(0, 256, int(rng.integers(4, 40)), dtype=np.uint8).tobytes() for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 40))]
        out += rng.integers(65, 69, int(rng.integers(0, 30)), dtype=np.uint8).tobytes()
    return bytes(out[:n])


def _repeat_codes_block() -> bytes:
    """a dynamic header written with 16, 17 and 18, the 16 copying symbol 256's length over symbol
    257 and the four distance lengths (across the HLIT / HDIST boundary)."""
    lit = [0] * 258
    for s in (97, 98, 256, 257):
        lit[s] = 2
    dist = [2, 2, 2, 2]
    seq = [(18, 97 - 11), (2, 0), (2, 0), (18, 138 - 11), (18, 11 - 11), (17, 8 - 3), (2, 0), (16, 5 - 3)]
    w = BitW()
    dynamic_block(w, lit, dist, [("L", 97), ("L", 98), ("M", 3, 2), ("M", 3, 1), ("M", 3, 4), ("E",)], cl_seq=seq)
    return w.bytes()


def _far_block() -> bytes:
    """32768 stored bytes, then copies at distance exactly 32768: length 3 at the far end of the
    window, then 258."""
    head = _rng(2).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = BitW()
    stored_block(w, head, final=False)
    fixed_block(w, [("M", 3, 32768), ("M", 258, 32768), ("L", 7), ("M", 3, 32768), ("E",)])
    return w.bytes()


@functools.lru_cache(maxsize=None)
def valid() -> List[Block]:
    from oracle import oracle

    import bgzf_inputs as B

    out: List[Block] = []

    def add(name, comp, want=None):
        want = ref(comp) if want is None else want
        assert ref(comp) == want, name
        out.append(Block(name, comp, len(want), want))

    rnd = _rng(3).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    text = _bamlike(65536)
    add("stored", deflate(rnd[:1000], 0), rnd[:1000])
    add("stored_65535", deflate(rnd[:65535], 0), rnd[:65535])
    add("stored_empty", deflate(b"", 0), b"")
    add("empty_fixed", deflate(b"", 6), b"")
    add("fixed", deflate(text[:5000], 6, zlib.Z_FIXED), text[:5000])
    for lv in (1, 6, 9):
        add("dynamic_l%d" % lv, deflate(text[:40000], lv), text[:40000])
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    multi = c.compress(text[:20000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[20000:45000]) + c.flush()
    add("multi_full_flush", multi, text[:45000])
    add("isize_1", deflate(b"x", 6), b"x")
    add("isize_65280", deflate(text[:65280], 6), text[:65280])
    add("isize_65536", deflate(text, 6), text)
    lits = _rng(4).integers(0, 64, 30000, dtype=np.uint8).tobytes()
    add("all_literals", deflate(lits, 6, zlib.Z_HUFFMAN_ONLY), lits)
    add("one_byte_60k", deflate(b"\x5a" * 60000, 6), b"\x5a" * 60000)
    add("period_3", deflate(b"abc" * 15000, 9), b"abc" * 15000)
    add("distance_32768", _far_block())
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    skew = np.repeat(np.arange(22, dtype=np.uint8), fib)
    _rng(5).shuffle(skew)
    add("codes_15_bits", deflate(skew.tobytes(), 6, zlib.Z_HUFFMAN_ONLY), skew.tobytes())
    add("repeat_16_17_18", _repeat_codes_block())
    for case in B.edge_cases():
        add("zlib_" + case.name, deflate(case.data, 6), case.data)
        blk = oracle.bgzf_block(case.data)
        if blk:
            add("encoder_" + case.name, blk[18:-8], case.data)
    for k in range(8):
        add("zlib_sweep_%d" % k, deflate(B.sweep_block(k), 1 + k), None)
    for n in (1, 2, 255, 65279):
        blk = oracle.bgzf_block(B.sized(n))
        add("encoder_sized_%d" % n, blk[18:-8], B.sized(n))
    return out


def many() -> List[Block]:
    """a launch of 260 mixed blocks, some with isize 0."""
    v = {b.name: b for b in valid()}
    pick = [v[k] for k in ("dynamic_l6", "stored_empty", "fixed", "one_byte_60k", "empty_fixed", "stored", "isize_1",
                           "multi_full_flush", "distance_32768", "all_literals")]
    return [pick[(7 * i) % len(pick)] for i in range(260)]


def _flip(comp: bytes, bit: int) -> bytes:
    b = bytearray(comp)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def corrupt() -> List[Block]:
    """one block per status code (some codes by two routes); zlib rejects each, or inflates it to a
    size other than the isize claimed (tests/test_inflate_host.py asserts that)."""
    v = {b.name: b for b in valid()}
    out: List[Block] = []

    def add(name, comp, isize, code):
        out.append(Block(name, comp, isize, None, code))

    fx = v["fixed"]
    add("btype_3", bytes([fx.comp[0] | 6]) + fx.comp[1:], fx.isize, L.INFLATE_EBTYPE)
    st = v["stored"]
    add("nlen_flipped", _flip(st.comp, 8 * 3 + 5), st.isize, L.INFLATE_ESTORED)
    # code lengths: three literal codes of one bit (over-subscribed); two of two bits (incomplete)
    for name, n2 in (("oversubscribed", None), ("incomplete", 2)):
        lit = [0] * 257
        for s in (97, 98, 256):
            lit[s] = 1 if n2 is None else 2
        if n2:
            lit[98] = 0
        w = BitW()
        dynamic_block(w, lit, [1], [], cl_seq=[(x, 0) for x in lit + [1]])
        w.put(0, 16)
        add(name + "_lengths", w.bytes(), 1, L.INFLATE_ELENGTHS)
    # the same header's code-length code made incomplete: zlib's "invalid code lengths set"
    w = BitW()
    dynamic_block(w, [0] * 256 + [1], [1], [], cl_seq=[(0, 0)] * 256 + [(1, 0), (1, 0)], cl_lens=[2, 2] + [0] * 17)
    w.put(0, 16)
    add("incomplete_codelen_code", w.bytes(), 1, L.INFLATE_ELENGTHS)
    w = BitW()
    dynamic_block(w, [0] * 256 + [1], [1], [], cl_seq=[(16, 0), (1, 0), (0, 0)], cl_lens=[2, 2] + [0] * 14 + [1, 0, 0])
    w.put(0, 16)
    add("repeat_16_first", w.bytes(), 1, L.INFLATE_EREPEAT)
    w = BitW()
    seq = [(18, 138 - 11), (18, 118 - 11), (1, 0), (18, 0)]  # 256 zeros, the end-of-block code, 11 zeros for 1 place
    dynamic_block(w, [0] * 256 + [1], [1], [], cl_seq=seq)
    w.put(0, 16)
    add("repeat_overrun", w.bytes(), 1, L.INFLATE_EREPEAT)
    for name, toks in (("symbol_286", [("L", 65), ("S", 286), ("E",)]), ("symbol_287", [("L", 65), ("S", 287), ("E",)]),
                       ("distance_30", [("L", 65), ("L", 66), ("L", 67), ("D", 3, 30, 0), ("E",)]),
                       ("distance_31", [("L", 65), ("L", 66), ("L", 67), ("D", 3, 31, 0), ("E",)])):
        w = BitW()
        fixed_block(w, toks)
        add(name, w.bytes(), 6, L.INFLATE_ESYMBOL)
    w = BitW()
    fixed_block(w, [("L", 65), ("L", 66), ("M", 3, 3), ("E",)])
    add("distance_before_start", w.bytes(), 5, L.INFLATE_EDIST)
    d6 = v["dynamic_l6"]
    add("isize_one_less", d6.comp, d6.isize - 1, L.INFLATE_EOVERFLOW)
    add("isize_one_more", d6.comp, d6.isize + 1, L.INFLATE_ESHORT)
    add("stored_isize_one_less", st.comp, st.isize - 1, L.INFLATE_EOVERFLOW)
    add("clen_cut", d6.comp[:len(d6.comp) // 2], d6.isize, L.INFLATE_EINPUT)
    add("clen_cut_header", d6.comp[:20], d6.isize, L.INFLATE_EINPUT)
    add("stored_cut", st.comp[:500], st.isize, L.INFLATE_EINPUT)
    add("clen_0", b"", 0, L.INFLATE_EINPUT)
    # HLIT = 287 (zlib: too many length or distance symbols)
    w = BitW()
    w.put(1, 1)
    w.put(2, 2)
    w.put(30, 5)
    w.put(0, 5)
    w.put(0, 4)
    w.put(0, 64)
    add("hlit_287", w.bytes(), 1, L.INFLATE_ECOUNTS)
    w = BitW()
    dynamic_block(w, [1, 1], [1], [], hlit=257, cl_seq=[(1, 0), (1, 0)] + [(0, 0)] * 255 + [(1, 0)])
    w.put(0, 16)
    add("no_end_of_block", w.bytes(), 1, L.INFLATE_ENOEOB)
    # one distance code of one bit (accepted, incomplete); the stream uses the other bit
    w = BitW()
    lit = [0] * 258
    for s in (97, 256, 257):
        lit[s] = 2
    lit[98] = 2
    dynamic_block(w, lit, [1], [("L", 97), ("L", 98), ("L", 97)])
    w.code(canon(lit)[257], 2)
    w.put(1, 1)  # the distance code's unused bit
    w.put(0, 16)
    add("unused_distance_code", w.bytes(), 6, L.INFLATE_ECODE)
    return out

"""Inputs of cli zipper --stream true's tests (test_zipper_stream.py, test_gpu_zipper_stream.py):
ALIGNED / UNMAPPED record lists in one template order, built with zipper_inputs' rec / pair / tag,
and a BAM writer with small BGZF blocks, so that a few hundred records span many blocks and pieces."""
import struct
import zlib

import numpy as np

import zipper_inputs as ZI
import zipper_ref as ZR

TEXT_A = ZI.HEADER_A
TEXT_U = ZI.HEADER_U
REFS = ZI.REFS
PERBASE = ZI.tag("MI", "Z", "7/B") + ZI.tag("RX", "Z", "ACG-TTA") + ZI.tag("cd", "B", ("s", [1, 2, 3, 4, 5])) + \
    ZI.tag("ac", "Z", "ACGTN") + ZI.tag("aq", "Z", "IJKLM") + ZI.tag("cD", "i", 3)


def write_bam(path, text, refs, records: bytes, block=3000):
    """zipper_ref.write_bam with blocks of `block` bytes"""
    s = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for nm, ln in refs:
        s += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    s += records
    with open(path, "wb") as fh:
        for i in range(0, len(s), block):
            b = s[i:i + block]
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            z = c.compress(b) + c.flush()
            fh.write(bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(z) + 25) + z +
                     struct.pack("<II", zlib.crc32(b), len(b)))
        fh.write(ZR.EOF_BLOCK)


def _pair_at(name, ref, pos, rev, aux=ZI.ALN, unmapped=False):
    f1, f2 = (83, 163) if rev else (99, 147)
    if unmapped:
        return [ZI.rec(name, 77, aux=aux), ZI.rec(name, 141, aux=aux)]
    return [ZI.rec(name, f1, ref, pos, aux=aux), ZI.rec(name, f2, ref, pos + 3, aux=aux)]


def _upair(name, k=0):
    return ZI.pair(name, PERBASE + ZI.tag("RG", "Z", "A"), PERBASE + ZI.tag("cE", "f", 0.5 + k))


def case(name):
    """-> (ALIGNED's records, UNMAPPED's records): lists of record bytes, ALIGNED's templates a
    subsequence of UNMAPPED's"""
    rng = np.random.default_rng(len(name) + 11)
    a, u = [], []
    if name == "contigs3":  # shuffled coordinates on 3 contigs; UNMAPPED templates with no aligned record before, between, after
        for k in range(300):
            nm = "t%04d" % k
            u += _upair(nm, k)
            if k in (0, 1, 150, 151, 152, 298, 299):
                continue
            a += _pair_at(nm, int(rng.integers(0, 3)), int(rng.integers(0, 4000)), bool(rng.integers(0, 2)))
    elif name == "ties":  # many records of one (refID, pos, strand) all over the file, between others
        for k in range(240):
            nm = "k%04d" % k
            u += _upair(nm, k)
            a += _pair_at(nm, 1, 500, False) if k % 3 else _pair_at(nm, int(rng.integers(0, 3)), int(rng.integers(400, 600)), k % 2 == 0)
    elif name == "one_key":  # every record of one key, no end bit: fragments
        for k in range(60):
            nm = "o%03d" % k
            u.append(ZI.rec(nm, 4, aux=PERBASE))
            a.append(ZI.rec(nm, 16, 2, 77, aux=ZI.ALN))
    elif name == "short_run":  # the first templates end long before the others; then ascending, disjoint runs
        for k in range(200):
            nm = "s%04d" % k
            u += _upair(nm, k)
            a += _pair_at(nm, 0, k if k < 20 else 1000 + 10 * k, k % 2 == 1)
    elif name == "descending":  # every run lies wholly before the run before it
        for k in range(150):
            nm = "d%04d" % k
            u += _upair(nm, k)
            a += _pair_at(nm, 1, 4000 - 20 * k, k % 2 == 1)
    elif name == "flag4":  # stretches of templates whose records all have 0x4: at the front, in the middle, at the end
        for k in range(120):
            nm = "f%04d" % k
            u += _upair(nm, k)
            un = k < 12 or 50 <= k < 64 or k >= 108
            a += _pair_at(nm, 0, int(rng.integers(0, 3000)), k % 2 == 1, unmapped=un)
    elif name == "sec_supp":  # secondary and supplementary records, a mate with 0x4, a record with neither end bit
        for k in range(80):
            nm = "p%04d" % k
            if k % 7 == 3:
                u.append(ZI.rec(nm, 4, aux=PERBASE))
                a.append(ZI.rec(nm, 16 * (k % 2), 1, int(rng.integers(0, 900)), aux=ZI.ALN))
                continue
            u += _upair(nm, k)
            t = _pair_at(nm, 0, int(rng.integers(0, 900)), k % 2 == 1)
            if k % 5 == 0:
                t.insert(0, ZI.rec(nm, 99 | 0x800, 2, int(rng.integers(0, 900)), aux=ZI.ALN))
                t.append(ZI.rec(nm, 147 | 0x100, 1, int(rng.integers(0, 900)), aux=ZI.ALN))
            if k % 11 == 0:
                t[-1] = ZI.rec(nm, 133, 0, 5, cigar=[], aux=ZI.tag("YD", "Z", "f"))
            a += t
    elif name == "big":  # one record far larger than the others (and than a small chunk_bytes)
        for k in range(40):
            nm = "b%04d" % k
            u += _upair(nm, k)
            if k == 17:
                a += [ZI.rec(nm, 83, 0, 700, l_seq=30001, aux=ZI.ALN), ZI.rec(nm, 163, 0, 20, aux=ZI.ALN)]
            else:
                a += _pair_at(nm, 0, int(rng.integers(0, 1500)), k % 2 == 1)
    elif name == "empty":  # no aligned record at all
        for k in range(5):
            u += _upair("e%d" % k, k)
    elif name == "bound":  # a few thousand records for the memory bound: ~0.7 MB of record bytes
        long_aux = PERBASE + ZI.tag("ad", "B", ("s", list(range(60)))) + ZI.tag("bd", "B", ("s", list(range(60))))
        for k in range(1100):
            nm = "m%05d" % k
            u += ZI.pair(nm, long_aux, long_aux)
            a += _pair_at(nm, int(rng.integers(0, 3)), int(rng.integers(0, 100000)), bool(rng.integers(0, 2)))
    else:
        raise KeyError(name)
    return a, u


CASES = ["contigs3", "ties", "one_key", "short_run", "descending", "flag4", "sec_supp", "big", "empty"]


def budget(a, u) -> int:
    """the bytes chunk_bytes budgets: ALIGNED's records, and their partners' aux of those without flag 0x4"""
    aux = {(r["name"], r["flag"] & 0xC0): len(r["aux"]) for r in ZR.parse_records(b"".join(u))}
    pa = ZR.parse_records(b"".join(a))
    return sum(len(r) for r in a) + sum(aux[(r["name"], r["flag"] & 0xC0)] for r in pa if not r["flag"] & 4)


def gather_lengths():
    """bsdc_zip_gather's record lengths: the copy's edges, four residues mod 4, one of about 70,000 bytes"""
    return [38, 39, 40, 41, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 70001]


def gather_case(n, seed=3):
    """-> (src uint8 padded to 4, src_off int64 [n], src_len int32 [n]): records of gather_lengths()
    at source offsets of all four residues mod 4 (gaps of 0..3 bytes between them)"""
    rng = np.random.default_rng(seed)
    lens = gather_lengths()
    ln = np.asarray([lens[k % len(lens)] if (k % len(lens) != len(lens) - 1 or k < len(lens)) else 38 + k % 200 for k in range(n)],
                    np.int32)
    gap = np.asarray([(k * 7 + 1) % 4 for k in range(n)], np.int64)
    off = np.cumsum(ln.astype(np.int64) + gap) - ln
    total = int(off[-1] + ln[-1]) if n else 0
    src = np.zeros(max((total + 3) // 4 * 4, 4), np.uint8)
    src[:total] = rng.integers(0, 256, total, dtype=np.uint8)
    return src, off.astype(np.int64), ln


def gather_orders(n, seed=5):
    ident = np.arange(n, dtype=np.uint32)
    return {"identity": ident, "reverse": ident[::-1].copy(), "shuffle": np.random.default_rng(seed).permutation(n).astype(np.uint32)}

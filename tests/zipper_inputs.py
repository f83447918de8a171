"""Small aligned / unmapped record sets on cli zipper's edges, and the sort's inputs (test_zipper_*.py,
test_gpu_zipper.py).  Records are built as bytes here, with no code of the package."""
import struct

import numpy as np

SETTINGS = {"none": dict(reverse=[], revcomp=[], remove=[]),
            "consensus": dict(reverse=["Consensus"], revcomp=["Consensus"], remove=[]),
            "remove": dict(reverse=["cd"], revcomp=[], remove=["XR", "NM"])}
HEADER_A = "@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:chr1\tLN:900000000\n@SQ\tSN:chr2\tLN:5000\n@SQ\tSN:chr3\tLN:5000\n" \
           "@PG\tID:bwameth\tPN:bwameth\n@PG\tID:samtools\tPN:samtools\n@CO\taligned\n"
HEADER_U = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n@RG\tID:A\tSM:s\n@PG\tID:fgbio\tPN:fgbio\n@PG\tID:samtools\tPN:other\n@CO\tunmapped\n"
REFS = [("chr1", 900000000), ("chr2", 5000), ("chr3", 5000)]


def tag(nm: str, t: str, v) -> bytes:
    h = nm.encode() + t.encode()
    if t in "ZH":
        return h + (v.encode() if isinstance(v, str) else bytes(v)) + b"\0"
    if t == "B":
        sub, vals = v
        return h + sub.encode() + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]), *vals)
    return h + struct.pack("<" + {"A": "c", "c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[t],
                           v.encode() if t == "A" else v)


def rec(name, flag, ref=-1, pos=-1, cigar=None, l_seq=5, aux=b"", mapq=30, next_ref=-1, next_pos=-1, tlen=0) -> bytes:
    name = name if isinstance(name, bytes) else name.encode()
    cigar = [l_seq << 4] if cigar is None else cigar
    seq = bytes((17 * (k + len(name))) & 0xff for k in range((l_seq + 1) // 2))
    if l_seq & 1:
        seq = seq[:-1] + bytes([seq[-1] & 0xf0])
    qual = bytes((k * 7 + flag) % 42 for k in range(l_seq))
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, mapq, 4680 + (pos >> 14 if pos > 0 else 0) % 100, len(cigar),
                       flag, l_seq, next_ref, next_pos, tlen) + name + b"\0" + struct.pack("<%dI" % len(cigar), *cigar) + \
        seq + qual + aux
    return struct.pack("<i", len(body)) + body


def pair(name, aux1=b"", aux2=b"", f1=77, f2=141):
    return [rec(name, f1, aux=aux1), rec(name, f2, aux=aux2)]


CONS = tag("MI", "Z", "12/A") + tag("RX", "Z", "ACG-TTA") + tag("RG", "Z", "A") + tag("cD", "i", 7) + \
    tag("cd", "B", ("s", [1, 2, 3])) + tag("ad", "B", ("s", [4, 5])) + tag("ac", "Z", "ACGTNacgt-") + tag("aq", "Z", "IJK") + \
    tag("XR", "Z", "gone")
ALN = tag("NM", "i", 2) + tag("MD", "Z", "5") + tag("YD", "Z", "f")


def _cases():
    c = {}
    long_name = b"n" * 254
    c["names"] = ([rec("a", 99, 0, 10, aux=ALN), rec(long_name, 147, 0, 20, aux=ALN)],
                  [rec("a", 77, aux=CONS), rec(long_name, 141, aux=CONS)])
    c["aux_empty"] = ([rec("e1", 99, 0, 5), rec("e1", 147, 0, 6, aux=ALN), rec("e2", 83, 1, 7)],
                      [rec("e1", 77, aux=CONS), rec("e1", 141), rec("e2", 77), rec("e2", 141)])
    c["both_sides"] = ([rec("b", 83, 0, 30, aux=tag("NM", "i", 2) + tag("RG", "Z", "bwa") + tag("MD", "Z", "5") + tag("MI", "Z", "x"))],
                       [rec("b", 77, aux=CONS + tag("NM", "C", 9))])
    spell = tag("zz", "B", ("C", list(b"MIZxRGZy\0XRZ"))) + tag("zy", "Z", "NMiXRZcdBs") + tag("zh", "H", "1AE3")
    c["spelled"] = ([rec("s", 99, 0, 40, aux=spell + ALN), rec("s", 147, 0, 41, aux=ALN)],
                    [rec("s", 77, aux=CONS), rec("s", 141, aux=spell + CONS)])
    subs = b"".join(tag(nm, "B", (sub, [(-1) ** k * (k + 1) if sub in "csi" else k + 1.5 if sub == "f" else k + 1 for k in range(cnt)]))
                    for nm, sub, cnt in (("cd", "s", 5), ("ce", "S", 2), ("ad", "c", 1), ("ae", "C", 0), ("bd", "i", 5),
                                         ("be", "I", 2), ("aq", "f", 5), ("bq", "c", 2)))
    c["b_subtypes"] = ([rec("t", 83, 0, 50, aux=ALN), rec("t", 163, 0, 51, aux=ALN)],
                       [rec("t", 77, aux=subs), rec("t", 141, aux=subs)])
    zl = tag("ac", "Z", "") + tag("bc", "Z", "C") + tag("aq", "Z", "AB") + tag("bq", "Z", "") + tag("cd", "Z", "x")
    c["z_lens"] = ([rec("z", 83, 0, 60), rec("z", 163, 0, 61)], [rec("z", 77, aux=zl), rec("z", 141, aux=zl)])
    c["odd_zero"] = ([rec("o", 99, 0, 70, l_seq=7, aux=ALN), rec("o", 147, 0, 71, cigar=[], aux=ALN), rec("o2", 83, 0, 72, l_seq=0, cigar=[])],
                     [rec("o", 77, aux=CONS), rec("o", 141, aux=CONS), rec("o2", 77, aux=CONS)])
    c["sec_supp"] = ([rec("p", 99 | 0x800, 1, 5, aux=ALN), rec("p", 99, 0, 80, aux=ALN), rec("p", 83 | 0x100, 2, 9, aux=ALN),
                      rec("p", 147, 0, 81, aux=ALN)],
                     [rec("p", 77, aux=CONS), rec("p", 141, aux=tag("MI", "Z", "12/A"))])
    c["fragment"] = ([rec("f", 16, 0, 90, aux=ALN), rec("g", 0, 0, 91, aux=ALN)],
                     [rec("f", 4, aux=CONS), rec("g", 4, aux=CONS)])
    c["bit200"] = ([rec("q", 99, 0, 100, aux=ALN), rec("q", 147 | 0x200, 0, 101, aux=ALN)],
                   [rec("q", 77 | 0x200, aux=CONS), rec("q", 141, aux=CONS)])
    c["unmapped_mate"] = ([rec("m", 73, 0, 110, aux=ALN), rec("m", 133, 0, 110, cigar=[], aux=tag("YD", "Z", "f"))],
                          [rec("m", 77, aux=CONS), rec("m", 141, aux=CONS)] + pair("lonely", CONS, CONS) + pair("lonely2"))
    c["long"] = ([rec("L", 83, 0, 120, l_seq=50001, aux=ALN), rec("L", 163, 0, 121, aux=ALN)],
                 [rec("L", 77, aux=CONS), rec("L", 141, aux=tag("cd", "B", ("s", list(range(-9000, 9000)))) + CONS)])
    c["ties"] = ([rec("k3", 99, 1, 500, aux=ALN), rec("k1", 83, 0, 500, aux=ALN), rec("k2", 99, 0, 500, aux=ALN),
                  rec("k4", 99, 0, 500, aux=ALN), rec("k5", 83, 0, 500, aux=ALN), rec("k6", 99, 0, 0, aux=ALN),
                  rec("k7", 99, 0, 1 << 29, aux=ALN), rec("k8", 83, 2, 499, aux=ALN)],
                 [rec("k%d" % k, 77, aux=CONS) for k in range(1, 9)])
    return c


def case(name):
    """-> (ALIGNED's records, UNMAPPED's records) as lists of record bytes"""
    c = _cases()
    if name == "all":  # every case in one file, the aligned records interleaved out of coordinate order
        a = [r for k in sorted(c) for r in c[k][0]]
        u = [r for k in sorted(c) for r in c[k][1]]
        return a[::2] + a[1::2], u[::-1]
    return c[name]


NAMES = sorted(_cases()) + ["all"]


def error_case(name):
    """-> (ALIGNED's records, UNMAPPED's records, a word of the message)"""
    if name == "missing_partner":
        return [rec("x", 99, 0, 1)], [rec("x", 141)], "x"
    if name == "duplicate_partner":
        return [rec("y", 99, 0, 1)], [rec("y", 77), rec("y", 141), rec("y", 77, aux=CONS)], "y"
    if name == "truncated_aux":
        return [rec("tr", 99, 0, 1)], [rec("tr", 77, aux=tag("cd", "B", ("s", [1, 2, 3]))[:-1])], "tr"
    if name == "truncated_z":
        return [rec("tz", 99, 0, 1, aux=b"MDZ12")], [rec("tz", 77)], "tz"
    if name == "unknown_type":
        return [rec("un", 99, 0, 1, aux=b"XYq\1\2")], [rec("un", 77, aux=CONS)], "un"
    raise KeyError(name)


ERRORS = ["missing_partner", "duplicate_partner", "truncated_aux", "truncated_z", "unknown_type"]


def sort_case(name, tile=2048):
    """-> (refID, pos, flag) int arrays of the sort's input"""
    rng = np.random.default_rng(len(name))
    z = lambda n: np.zeros(n, np.int64)  # noqa: E731

    def rand(n):
        return rng.integers(0, 3, n), rng.integers(0, 70000, n), rng.choice([0, 16, 99, 83], n)
    if name == "n0":
        return z(0), z(0), z(0)
    if name == "n1":
        return z(1) + 2, z(1) + 77, z(1) + 16
    if name == "two_equal":
        return z(2) + 1, z(2) + 5, z(2)
    if name == "all_equal":
        return z(700), z(700) + 300, z(700) + 16
    if name == "strand_only":
        return z(300), z(300) + 9, rng.choice([0, 16], 300)
    if name == "ref_only":
        return rng.integers(0, 400, 300), z(300) + 9, z(300)
    if name == "pos_edges":
        return z(6), np.asarray([1 << 29, 0, 1 << 29, 0, 255, 256]), np.asarray([0, 16, 16, 0, 0, 0])
    if name in ("n255", "n256", "n257"):
        return rand(int(name[1:]))
    if name == "tile_plus_1":
        return rand(tile + 1)
    if name == "two_tiles_plus_1":
        return rand(2 * tile + 1)
    raise KeyError(name)


SORTS = ["n0", "n1", "two_equal", "all_equal", "strand_only", "ref_only", "pos_edges", "n255", "n256", "n257", "tile_plus_1",
         "two_tiles_plus_1"]

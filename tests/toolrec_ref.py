"""A pure Python / numpy restatement of DESIGN.md 3.10: the BAM record bytes of one record after
tool 1 and tool 2, from the input record's fields and its stage-dump entry.  Nothing here calls the
library: tests/test_toolrec_host.py compares the host twin with it byte for byte."""
import struct

import numpy as np

OP_S = 4
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def reg2bin(beg, end):
    end -= 1
    for sh, k in ((14, 15), (17, 12), (20, 9), (23, 6), (26, 3)):
        if beg >> sh == end >> sh:
            return (((1 << k) - 1) // 7 + (beg >> sh)) & 0xFFFF
    return 0


def strip_clips(ops):
    ops = list(ops)
    if ops and (ops[0] & 15) == OP_S:
        ops = ops[1:]
    if ops and (ops[-1] & 15) == OP_S:
        ops = ops[:-1]
    return ops


def new_cigar(ops, tags):
    ops = strip_clips(ops)
    if tags & 2:
        ops = [1 << 4] + ops
        if tags & 1:
            if (ops[-1] >> 4) > 1:
                ops[-1] -= 1 << 4
            else:
                ops.pop()
    elif tags & 4:
        ops = [1 << 4] + ops
    if tags & 8:
        ops = ops + [1 << 4]
    return ops


def aux_tags(aux):
    """[(tag bytes, whole tag bytes)] by a walk over the types"""
    out, i = [], 0
    while i < len(aux):
        t = chr(aux[i + 2])
        if t in FIXED:
            j = i + 3 + FIXED[t]
        elif t in "ZH":
            j = aux.index(b"\0", i + 3) + 1
        else:
            assert t == "B"
            j = i + 8 + FIXED[chr(aux[i + 3])] * struct.unpack_from("<I", aux, i + 4)[0]
        out.append((bytes(aux[i:i + 2]), bytes(aux[i:j])))
        i = j
    assert i == len(aux)
    return out


def new_aux(aux, tags):
    if not tags & 2:
        return bytes(aux)
    kept = b"".join(b for t, b in aux_tags(aux) if t not in (b"RD", b"LA"))
    return kept + b"RDC" + bytes([tags & 1]) + b"LAC\x01"


def record_bytes(r):
    """r: name (bytes), flag, ref_id, mapq, next_ref_id, next_pos, tlen, cigar (the input's ops,
    clips included), aux (bytes); the dump entry: pos, seq (nt16 codes), qual, tags."""
    t = int(r["tags"])
    seq = np.asarray(r["seq"], np.uint8) & 15
    L = int(seq.shape[0])
    ops = new_cigar(r["cigar"], t)
    reflen = sum(o >> 4 for o in ops if (o & 15) in REF_OPS)
    pos = int(r["pos"])
    b = reg2bin(pos, pos + (reflen if reflen > 0 else 1))
    codes = np.concatenate([seq, np.zeros(L & 1, np.uint8)])
    packed = ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8).tobytes()
    name = bytes(r["name"])
    body = struct.pack("<iiBBHHHiiii", r["ref_id"], pos, len(name) + 1, r["mapq"], b, len(ops), r["flag"], L,
                       r["next_ref_id"], r["next_pos"], r["tlen"])
    body += name + b"\0" + struct.pack("<%dI" % len(ops), *ops) + packed + np.asarray(r["qual"], np.uint8).tobytes()
    body += new_aux(r["aux"], t)
    return struct.pack("<i", len(body)) + body


def stream(recs):
    """-> (off [n + 1], bytes) of the records back to back"""
    parts = [record_bytes(r) for r in recs]
    off = np.zeros(len(parts) + 1, np.int64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    return off, b"".join(parts)

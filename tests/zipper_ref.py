"""cli zipper's rules restated in pure Python, record by record on parsed records.
Shares no code with the package: its own BAM record parser and encoder, its own aux walk, its own
BGZF reader and writer (zlib)."""
import struct
import zlib

FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
CONSENSUS_REVERSE = ["ad", "ae", "bd", "be", "cd", "ce", "aq", "bq"]
CONSENSUS_REVCOMP = ["ac", "bc"]
COMP = {ord(a): ord(b) for a, b in zip("ACGTacgt", "TGCAtgca")}
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def parse_records(data: bytes):
    """BAM record bytes -> [dict]: every fixed field, name, cigar (uint32 ops), seq (packed bytes), qual, aux"""
    out, i = [], 0
    while i < len(data):
        bs, ref, pos, lrn, mapq, bin_, nc, flag, ls, nref, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", data, i)
        o = i + 36
        name = data[o:o + lrn - 1]
        assert data[o + lrn - 1] == 0
        o += lrn
        cigar = list(struct.unpack_from("<%dI" % nc, data, o))
        o += 4 * nc
        seq = data[o:o + (ls + 1) // 2]
        o += (ls + 1) // 2
        qual = data[o:o + ls]
        o += ls
        assert o <= i + 4 + bs
        out.append(dict(name=name, flag=flag, ref=ref, pos=pos, mapq=mapq, bin=bin_, next_ref=nref, next_pos=npos,
                        tlen=tlen, cigar=cigar, l_seq=ls, seq=seq, qual=qual, aux=data[o:i + 4 + bs]))
        i += 4 + bs
    assert i == len(data)
    return out


def encode(r: dict) -> bytes:
    body = struct.pack("<iiBBHHHiiii", r["ref"], r["pos"], len(r["name"]) + 1, r["mapq"], r["bin"], len(r["cigar"]), r["flag"],
                       r["l_seq"], r["next_ref"], r["next_pos"], r["tlen"]) + r["name"] + b"\0" + \
        struct.pack("<%dI" % len(r["cigar"]), *r["cigar"]) + r["seq"] + r["qual"] + r["aux"]
    return struct.pack("<i", len(body)) + body


def walk(aux: bytes):
    """aux bytes -> [(two-byte name, type letter, the tag's bytes whole)], by type; ValueError when malformed"""
    out, i, n = [], 0, len(aux)
    while i < n:
        if i + 3 > n:
            raise ValueError("trailing aux bytes")
        t = chr(aux[i + 2])
        if t in FIXED:
            j = i + 3 + FIXED[t]
        elif t in "ZH":
            j = aux.find(b"\0", i + 3)
            if j < 0:
                raise ValueError("aux tag %r runs past the record" % aux[i:i + 2])
            j += 1
        elif t == "B":
            if i + 8 > n:
                raise ValueError("aux tag %r runs past the record" % aux[i:i + 2])
            st = chr(aux[i + 3])
            if st not in FIXED or st == "A":
                raise ValueError("aux tag %r has an unknown type" % aux[i:i + 2])
            j = i + 8 + FIXED[st] * struct.unpack_from("<I", aux, i + 4)[0]
        else:
            raise ValueError("aux tag %r has an unknown type" % aux[i:i + 2])
        if j > n:
            raise ValueError("aux tag %r runs past the record" % aux[i:i + 2])
        out.append((aux[i:i + 2], t, aux[i:j]))
        i = j
    return out


def flip(tag: bytes, t: str, rev: bool, rc: bool) -> bytes:
    """rule 5 on one tag of the partner (of an output record with flag 0x10)"""
    if t == "Z" and (rev or rc):
        s = tag[3:-1][::-1]
        if not rev:
            s = bytes(COMP.get(c, c) for c in s)
        return tag[:3] + s + b"\0"
    if t == "B" and rev:
        es = FIXED[chr(tag[3])]
        el = [tag[8 + k * es:8 + (k + 1) * es] for k in range((len(tag) - 8) // es)]
        return tag[:8] + b"".join(el[::-1])
    return tag


def expand(names, word):
    out = []
    for x in names:
        for t in (word if x == "Consensus" else [x]):
            if t.encode() not in out:
                out.append(t.encode())
    return out


def end_of(flag: int) -> int:
    return flag & 0xC0


def zip_records(aligned, unmapped, reverse=(), revcomp=(), remove=()):
    """Rules 1-6 -> (the output records in order, dict of counts)"""
    reverse, revcomp = expand(reverse, CONSENSUS_REVERSE), expand(revcomp, CONSENSUS_REVCOMP)
    remove = expand(remove, [])
    part = {}
    for u in unmapped:
        k = (u["name"], end_of(u["flag"]))
        if k in part:
            raise ValueError("UNMAPPED holds read %r twice" % u["name"])
        part[k] = u
    out, seen = [], set()
    for i, a in enumerate(aligned):
        u = part.get((a["name"], end_of(a["flag"])))
        if u is None:
            raise ValueError("aligned read %r has no partner" % a["name"])
        seen.add(a["name"])
        if a["flag"] & 4:
            continue
        if a["ref"] < 0 or a["pos"] < -1:
            raise ValueError("aligned read %r is mapped but has no reference" % a["name"])
        flag = (a["flag"] & ~0x200) | (u["flag"] & 0x200)
        pt = walk(u["aux"])
        theirs = {nm for nm, _, _ in pt}
        aux = [b for nm, _, b in walk(a["aux"]) if nm not in theirs and nm not in remove]
        for nm, t, b in pt:
            if nm in remove:
                continue
            aux.append(flip(b, t, nm in reverse, nm in revcomp) if flag & 0x10 else b)
        out.append((a["ref"], a["pos"], int(flag & 0x10 != 0), i, dict(a, flag=flag, aux=b"".join(aux))))
    out.sort(key=lambda x: x[:4])
    lonely = len({u["name"] for u in unmapped} - seen)
    return [x[4] for x in out], dict(records_in=len(aligned), records_out=len(out), unmapped_dropped=len(aligned) - len(out),
                                     templates_without_aligned=lonely)


def header_text(ta: str, tu: str) -> str:
    """rule 7"""
    la, lu = [x for x in ta.split("\n") if x], [x for x in tu.split("\n") if x]
    ident = lambda x: [f[3:] for f in x.split("\t")[1:] if f[:3] == "ID:"][:1]  # noqa: E731
    pg = [x for x in la if x[:3] == "@PG"]
    for x in lu:
        if x[:3] == "@PG" and ident(x) not in [ident(y) for y in pg]:
            pg.append(x)
    lines = ["@HD\tVN:1.6\tSO:coordinate"] + [x for x in la if x[:3] == "@SQ"] + [x for x in lu if x[:3] == "@RG"] + pg + \
        [x for x in la + lu if x[:3] == "@CO"]
    return "\n".join(lines) + "\n"


def read_bam(path):
    """-> (header text, [(reference name, length)], record bytes, the blocks' count); every block's CRC32 and ISIZE checked"""
    data = open(path, "rb").read()
    assert data.endswith(EOF_BLOCK) and not data[:-len(EOF_BLOCK)].endswith(EOF_BLOCK), path + ": not exactly one EOF block"
    raw, i, nblk = [], 0, 0
    while i < len(data):
        bsize = struct.unpack_from("<H", data, i + 16)[0] + 1
        b = zlib.decompress(data[i + 18:i + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", data, i + bsize - 8)
        assert zlib.crc32(b) == crc and len(b) == isize
        raw.append(b)
        i += bsize
        nblk += 1
    s = b"".join(raw)
    assert s[:4] == b"BAM\1"
    lt = struct.unpack_from("<i", s, 4)[0]
    text = s[8:8 + lt].decode()
    o = 8 + lt
    nref = struct.unpack_from("<i", s, o)[0]
    o += 4
    refs = []
    for _ in range(nref):
        ln = struct.unpack_from("<i", s, o)[0]
        refs.append((s[o + 4:o + 4 + ln - 1].decode(), struct.unpack_from("<i", s, o + 4 + ln)[0]))
        o += 8 + ln
    return text, refs, s[o:], nblk


def write_bam(path, text: str, refs, records: bytes):
    s = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for nm, ln in refs:
        s += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    s += records
    with open(path, "wb") as fh:
        for i in range(0, len(s), 60000):
            b = s[i:i + 60000]
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            z = c.compress(b) + c.flush()
            fh.write(bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(z) + 25) + z +
                     struct.pack("<II", zlib.crc32(b), len(b)))
        fh.write(EOF_BLOCK)

"""cli group's rules in plain Python, template by template, with dicts and lists:
what the host twin and the kernels are held to.  No code of the package is used here.

run(records, ...) takes BAM records as bytes (block_size first) and returns Result: the output
records in order, every kept template's tag, and the info counters."""
import struct
from collections import namedtuple

Result = namedtuple("Result", "records tags info")
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
DROPS = ("secondary_supplementary_records", "not_paired", "unmapped_or_mate_unmapped", "no_reference", "non_pf",
         "low_mapq", "umi_other_letters")


class Rec:
    def __init__(self, b):
        self.b = b
        (bs, self.ref, self.pos, l_name, self.mapq, _bin, n_cig, self.flag, l_seq) = struct.unpack_from("<iiiBBHHHi", b, 0)
        assert bs + 4 == len(b)
        self.name = b[36:36 + l_name - 1]
        c = 36 + l_name
        self.cigar = [(w & 15, w >> 4) for w in struct.unpack_from("<%dI" % n_cig, b, c)]
        self.aux_at = c + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        self.rev = bool(self.flag & 0x10)

    def aux(self):
        """[(name, type, start, end)] of the aux block, walked by type"""
        b, i, out = self.b, self.aux_at, []
        while i < len(b):
            t = chr(b[i + 2])
            if t in FIXED:
                j = i + 3 + FIXED[t]
            elif t in "ZH":
                j = b.index(0, i + 3) + 1
            elif t == "B":
                j = i + 8 + FIXED[chr(b[i + 3])] * struct.unpack_from("<I", b, i + 4)[0]
            else:
                raise ValueError("unknown aux type")
            out.append((b[i:i + 2], t, i, j))
            i = j
        return out

    def pos5(self):
        clip = [k for k, (op, _) in enumerate(self.cigar) if op not in (4, 5)]
        lead = sum(n for op, n in self.cigar[:clip[0]]) if clip else sum(n for _, n in self.cigar)
        trail = sum(n for op, n in self.cigar[clip[-1] + 1:]) if clip else 0
        ref_len = sum(n for op, n in self.cigar if op in (0, 2, 3, 7, 8))
        return self.pos + max(ref_len, 1) - 1 + trail if self.rev else self.pos - lead


def hamming(a, b):
    return sum(x != y for x, y in zip(a[0] + a[1], b[0] + b[1]))


def run(records, edits=1, min_map_q=1, include_non_pf=False, raw_tag=b"RX", assign_tag=b"MI"):
    info = {"records_in": len(records)}
    recs = [Rec(b) for b in records]
    info["secondary_supplementary_records"] = sum(1 for r in recs if r.flag & 0x900)
    by_name = {}
    for r in recs:
        if r.flag & 0x900:
            continue
        t = by_name.setdefault(r.name, {"R1": [], "R2": [], "other": []})
        t["R1" if r.flag & 0xC0 == 0x40 else "R2" if r.flag & 0xC0 == 0x80 else "other"].append(r)
    for name, t in by_name.items():
        if len(t["R1"]) > 1 or len(t["R2"]) > 1:
            raise ValueError("read %r occurs twice" % name.decode())
    info["templates_in"] = len(by_name)
    for k in DROPS[1:]:
        info[k] = 0
    kept = []
    for name in sorted(by_name):
        t = by_name[name]
        if len(t["R1"]) != 1 or len(t["R2"]) != 1 or t["other"]:
            info["not_paired"] += 1
            continue
        r1, r2 = t["R1"][0], t["R2"][0]
        if not (r1.flag & r2.flag & 1) or (r1.flag | r2.flag) & 0xC:
            info["unmapped_or_mate_unmapped"] += 1
        elif r1.ref < 0 or r2.ref < 0:
            info["no_reference"] += 1
        elif (r1.flag | r2.flag) & 0x200 and not include_non_pf:
            info["non_pf"] += 1
        elif r1.mapq < min_map_q or r2.mapq < min_map_q:
            info["low_mapq"] += 1
        else:
            kept.append((name, r1, r2))
    groups = {}
    templates = []
    for name, r1, r2 in kept:
        umi = [r1.b[i + 3:j - 1] for nm, t, i, j in r1.aux() if nm == raw_tag and t == "Z"]
        if not umi:
            raise ValueError("read %r has no raw tag" % name.decode())
        halves = umi[0].split(b"-")
        if len(halves) != 2 or not halves[0] or not halves[1]:
            raise ValueError("read %r: the raw tag is not two halves" % name.decode())
        if any(c not in b"ACGT" for c in halves[0] + halves[1]):
            info["umi_other_letters"] += 1
            continue
        if max(len(halves[0]), len(halves[1])) > 16:
            raise ValueError("read %r: more than 16 bases in a half" % name.decode())
        e1, e2 = (r1.ref, r1.pos5(), int(r1.rev)), (r2.ref, r2.pos5(), int(r2.rev))
        top = e1[:2] < e2[:2] or (e1[:2] == e2[:2] and not r1.rev)
        key = e1 + e2 if top else e2 + e1
        canon = (halves[0], halves[1]) if top else (halves[1], halves[0])
        t = {"name": name, "r1": r1, "r2": r2, "strand": "top" if top else "bottom", "canon": canon}
        templates.append(t)
        groups.setdefault(key, []).append(t)
    next_id, out, tags, fam, max_nodes = 0, [], {}, {}, 0
    for key in sorted(groups):
        g = groups[key]
        for t in g[1:]:
            if tuple(map(len, t["canon"])) != tuple(map(len, g[0]["canon"])):
                raise ValueError("reads %r and %r: half lengths differ in one position group" % (g[0]["name"].decode(), t["name"].decode()))
        nodes = {}
        for t in g:  # (in name order: kept is)
            nodes.setdefault(t["canon"], []).append(t)
        order = sorted(nodes, key=lambda c: (-len(nodes[c]), c))
        max_nodes = max(max_nodes, len(order))
        assigned, mols = {}, []
        for c in order:
            if c in assigned:
                continue
            mid = next_id
            next_id += 1
            assigned[c] = mid
            mols.append((mid, c))
            fifo = [c]
            rest = [d for d in order if d not in assigned]  # the still-unassigned nodes, in node order
            while fifo:
                p = fifo.pop(0)
                stay = []
                for d in rest:
                    if len(nodes[d]) <= len(nodes[p]) // 2 + 1 and hamming(p, d) <= edits:
                        assigned[d] = mid
                        fifo.append(d)
                    else:
                        stay.append(d)
                rest = stay
        rows = []
        for mid, root in mols:
            a_strand = nodes[root][0]["strand"]  # the root node's first template by name
            for c in order:
                if assigned[c] == mid:
                    for t in nodes[c]:
                        ab = "A" if t["strand"] == a_strand else "B"
                        rows.append((mid, ab, t["name"], t))
        assert len(rows) == len(g)
        for mid, ab, name, t in sorted(rows, key=lambda x: x[:3]):
            tag = b"%d/%s" % (mid, ab.encode())
            assert name not in tags  # every kept template gets exactly one id
            tags[name] = tag
            fam[tag] = fam.get(tag, 0) + 1
            for r in (t["r1"], t["r2"]):
                body = r.b[4:r.aux_at] + b"".join(r.b[i:j] for nm, _, i, j in r.aux() if nm != assign_tag) + \
                    assign_tag + b"Z" + tag + b"\0"
                out.append(struct.pack("<i", len(body)) + body)
    hist = {}
    for n in fam.values():
        hist[str(n)] = hist.get(str(n), 0) + 1
    info.update({"templates_out": len(templates), "position_groups": len(groups), "molecules": next_id,
                 "max_nodes_in_group": max_nodes, "family_size_histogram": hist})
    # the restatement's own invariants
    assert len(tags) == len(templates)
    assert sorted({int(v.split(b"/")[0]) for v in tags.values()}) == list(range(next_id))  # dense from 0
    assert sum(int(s) * c for s, c in hist.items()) == info["templates_out"]
    return Result(out, tags, info)

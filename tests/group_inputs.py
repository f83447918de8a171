"""Named inputs of cli group (test_group_ref.py, test_group_host.py, test_gpu_group.py): BAM records
as bytes, built with the record builders of zipper_inputs.py and no code of the package.  Each
case states the path it must reach (PATHS)."""
import random

import zipper_inputs as ZI

HEADER = "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:chr1\tLN:900000000\n@SQ\tSN:chr2\tLN:5000\n@SQ\tSN:chr3\tLN:5000\n" \
         "@RG\tID:A\tSM:s\n@PG\tID:bwameth\tPN:bwameth\n@CO\ttagged\n"
REFS = ZI.REFS
SMALL_NODES = 64  # k_group_small's most nodes


def tpl(name, umi, p1=100, p2=300, top=True, ref=0, ref2=None, aux=b"", aux2=b"", mapq=30, mapq2=None, cig1=None, cig2=None,
        f_or=0, f2_or=0, rx=True):
    """A template's two records.  top: R1 forward at p1, R2 reverse at p2; bottom: R1 reverse at p2, R2
    forward at p1 -- the same two ends, so the same position group."""
    ref2 = ref if ref2 is None else ref2
    mapq2 = mapq if mapq2 is None else mapq2
    a1 = (ZI.tag("RX", "Z", umi) if rx else b"") + aux
    if top:
        return [ZI.rec(name, 99 | f_or, ref, p1, cig1, aux=a1, mapq=mapq), ZI.rec(name, 147 | f2_or, ref2, p2, cig2, aux=aux2, mapq=mapq2)]
    return [ZI.rec(name, 83 | f_or, ref2, p2, cig2, aux=a1, mapq=mapq), ZI.rec(name, 163 | f2_or, ref, p1, cig1, aux=aux2, mapq=mapq2)]


def node(prefix, umi, count, **kw):
    return [r for k in range(count) for r in tpl("%s_%03d" % (prefix, k), umi, **kw)]


def counter_umi(k, digits):
    """k in base 4 over `digits` bases, split in two halves"""
    s = "".join("ACGT"[(k >> (2 * (digits - 1 - d))) & 3] for d in range(digits))
    return s[:digits // 2] + "-" + s[digits // 2:]


def singletons(prefix, n, digits, **kw):
    """n one-template nodes whose UMIs count in base 4: one connected molecule at one edit"""
    return [r for k in range(n) for r in tpl("%s%06d" % (prefix, k), counter_umi(k, digits), **kw)]


PATHS = {
    "chain": "counts 10, 5, 2 at one edit each: the walk reaches the third node through the second",
    "fence": "parent 4: child 3 joins (3 <= 4/2+1), child 4 does not and is a root; parent 1: child 1 joins",
    "tie": "two nodes of equal count 4 (neither joins the other): the smaller UMI is numbered first",
    "two_roots": "a child within one edit of two roots joins the earlier",
    "duplex": "top and bottom templates of one UMI: /A follows the root node's first template",
    "bottom_only": "a molecule of bottom templates alone is /A",
    "edits": "one group walked with --edits 0, 1, 2, 3",
    "halves": "half lengths 1+1, 16+16 and 6+8",
    "nodes_1": "one node", "nodes_2": "two nodes", "nodes_63": "63 nodes: k_group_small",
    "nodes_64": "64 nodes: k_group_small's last size", "nodes_65": "65 nodes: k_group_large",
    "chain3000": "3,000 singleton nodes in one molecule: 3,000 serial rounds of k_group_large in LDS",
    "near_groups": "position groups that differ in one strand bit only, and in pos5_hi only",
    "clipped": "soft and hard clips: pos5 is not pos, and two different pos share one pos5",
    "drops": "every drop reason once",
    "shuffled": "shuffled record order, an existing MI tag, a B array whose payload reads MIZ",
}


def _cases():
    c = {}
    c["chain"] = node("a", "AAAA-CCCC", 10) + node("b", "AAAT-CCCC", 5) + node("c", "AATT-CCCC", 2)
    c["fence"] = node("p", "AAAA-AAAA", 4) + node("j", "AAAC-AAAA", 3) + node("r", "AAAG-AAAA", 4) + \
        node("q", "TTTT-TTTT", 1, p1=500, p2=700) + node("s", "TTTT-TTTG", 1, p1=500, p2=700)
    c["tie"] = node("x", "CCCC-AAAT", 4) + node("y", "CCCC-AAAA", 4)
    c["two_roots"] = node("r1", "AAAA-AAAA", 5) + node("r2", "AATT-AAAA", 5) + node("ch", "AAAT-AAAA", 1)
    c["duplex"] = tpl("d3", "ACGT-TTGA") + tpl("d1", "TTGA-ACGT", top=False) + tpl("d2", "ACGT-TTGA") + \
        tpl("d4", "TTGA-ACGA", top=False)
    c["bottom_only"] = tpl("b1", "GGGG-ACAC", top=False) + tpl("b2", "GGGG-ACAC", top=False) + tpl("t9", "CCCC-GGGG", p1=900, p2=990)
    c["edits"] = node("e0", "AAAAAA-CCCCCC", 8) + node("e1", "AAAAAT-CCCCCC", 1) + node("e2", "AAAATT-CCCCCC", 1) + \
        node("e3", "AAATTT-CCCCCC", 1) + node("e4", "AATTTT-CCCCCC", 1) + node("sw", "CCCCCC-AAAAAA", 1)
    c["halves"] = node("h1", "A-C", 2, p1=10, p2=50) + node("h1b", "A-G", 1, p1=10, p2=50) + \
        node("h16", "ACGTACGTACGTACGT-TTTTTTTTTTTTTTTT", 2, p1=20, p2=60) + node("h16b", "ACGTACGTACGTACGT-TTTTTTTTTTTTTTTG", 1, p1=20, p2=60) + \
        node("h68", "ACGTAC-GGGGGGGG", 3, p1=30, p2=70) + node("h68b", "ACGTAC-GGGGGGGT", 1, p1=30, p2=70)
    for n in (1, 2, 63, 64, 65):
        # spread counts so that rule 4's order is not the UMI order, and some nodes do not join
        c["nodes_%d" % n] = [r for k in range(n) for r in node("n%02d" % k, counter_umi(k * 7 % 256, 8), 1 + (k * 5) % 4)]
    c["chain3000"] = singletons("c", 3000, 12)
    c["near_groups"] = tpl("g1", "AAAA-CCCC", 100, 300) + tpl("g2", "AAAA-CCCC", 100, 301) + \
        [ZI.rec("g3", 99, 0, 100, aux=ZI.tag("RX", "Z", "AAAA-CCCC")), ZI.rec("g3", 131, 0, 304)] + tpl("g4", "AAAA-CCCC", 100, 300)
    S, H, M = 4, 5, 0
    c["clipped"] = tpl("k1", "ACAC-GTGT", 103, 300, cig1=[3 << 4 | S, 2 << 4 | M]) + tpl("k2", "ACAC-GTGT", 100, 300) + \
        tpl("k3", "ACAC-GTGT", 105, 298, cig1=[2 << 4 | H, 3 << 4 | S, 2 << 4 | M], cig2=[5 << 4 | M, 2 << 4 | S]) + \
        tpl("k4", "GTGT-ACAC", 100, 300, top=False, cig2=[2 << 4 | S, 3 << 4 | M, 2 << 4 | H])
    c["drops"] = tpl("ok", "AAAA-CCCC") + [ZI.rec("ok", 99 | 0x800, 1, 5), ZI.rec("ok", 147 | 0x100, 1, 9)] + \
        [ZI.rec("single", 99, 0, 100, aux=ZI.tag("RX", "Z", "AAAA-CCCC"))] + \
        [ZI.rec("frag", 0, 0, 100, aux=ZI.tag("RX", "Z", "AAAA-CCCC"))] + \
        [ZI.rec("mateun", 73, 0, 100, aux=ZI.tag("RX", "Z", "AAAA-CCCC")), ZI.rec("mateun", 133, 0, 100, cigar=[])] + \
        [ZI.rec("noref", 99, -1, 100, aux=ZI.tag("RX", "Z", "AAAA-CCCC")), ZI.rec("noref", 147, 0, 300)] + \
        tpl("nonpf", "AAAA-CCCC", f2_or=0x200) + tpl("lowq", "AAAA-CCCC", mapq2=0) + tpl("umin", "AANA-CCCC") + \
        tpl("umilower", "AAaA-CCCC")
    sh = c["chain"] + c["duplex"] + c["clipped"] + \
        tpl("m1", "GGGG-TTTT", 100, 300, aux=ZI.tag("MI", "Z", "77/B") + ZI.tag("NM", "i", 1), aux2=ZI.tag("MI", "i", 5) + ZI.tag("MD", "Z", "5")) + \
        tpl("m2", "GGGG-TTTT", 100, 300, aux=ZI.tag("zz", "B", ("C", list(b"MIZ9/A\0MIZ"))), aux2=ZI.tag("zy", "Z", "MIZ"))
    random.Random(5).shuffle(sh)
    c["shuffled"] = sh
    return c


_C = None


def case(name):
    global _C
    if _C is None:
        _C = _cases()
    return _C[name]


NAMES = sorted(PATHS)
PARAMS = {"drops": [dict()], "edits": [dict(edits=e) for e in (0, 1, 2, 3)]}  # the parameter sets a case runs with


def params(name):
    return PARAMS.get(name, [dict()])


LDS_EDITS = 3  # the --edits the two cases below are walked with


def ball(prefix, n, digits=14):
    """One position group of n nodes: a root of two templates and n - 1 one-template nodes, every one
    within three edits of it (10,690 such UMIs of 14 bases exist).  With --edits 3 the root's round
    takes them all, and each then has a round of its own: n rounds, the FIFO filled to its end."""
    import itertools
    out = node(prefix + "root", counter_umi(0, digits), 2)
    k = 0
    for edits in (1, 2, 3):
        for at in itertools.combinations(range(digits), edits):
            for letters in itertools.product("CGT", repeat=edits):
                if k == n - 1:
                    return out
                u = ["A"] * digits
                for p, c in zip(at, letters):
                    u[p] = c
                u = "".join(u)
                out += tpl("%s%06d" % (prefix, k), u[:digits // 2] + "-" + u[digits // 2:])
                k += 1
    raise ValueError("no %d UMIs within three edits" % n)


def at_lds(lds_nodes):
    """A group of exactly lds_nodes nodes (the caller takes it from bsdc_group_lds_nodes: 7710 as
    built): the largest group k_group_large walks in LDS, its arrays ending at the arena's last byte."""
    return ball("K", lds_nodes)


def past_lds(lds_nodes):
    """A group of lds_nodes + 1 nodes: just past what k_group_large holds in LDS, so the FIFO and
    the assigned bytes lie in the scratch arena."""
    return ball("L", lds_nodes + 1)


def error_case(name):
    """-> (records, a word of the message)"""
    if name == "missing_tag":
        return tpl("ok", "AAAA-CCCC") + tpl("notag", "", rx=False), "notag"
    if name == "long_half":
        return tpl("long", "A" * 17 + "-CCCC"), "long"
    if name == "duplicate":
        return tpl("dup", "AAAA-CCCC") + [ZI.rec("dup", 99, 0, 100, aux=ZI.tag("RX", "Z", "AAAA-CCCC"))], "dup"
    if name == "half_lengths":
        return tpl("len1", "AAAA-CCCC") + tpl("len2", "AAAAA-CCC"), "len2"
    if name == "r1_z_without_nul":
        return tpl("ok", "AAAA-CCCC") + tpl("cutz", "", rx=False, aux=b"XYZab"), "cutz"
    if name == "r1_b_subtype":
        return tpl("subt", "", rx=False, aux=b"XYBq\1\0\0\0\7" + ZI.tag("RX", "Z", "AAAA-CCCC")), "subt"
    if name == "r1_cut_short":
        return tpl("shrt", "", rx=False, aux=ZI.tag("NM", "i", 1) + b"RX"), "shrt"
    raise KeyError(name)


ERRORS = ["missing_tag", "long_half", "duplicate", "half_lengths", "r1_z_without_nul", "r1_b_subtype", "r1_cut_short"]


def sweep(n_templates=20000, seed=11, err=0.01):
    """About n_templates templates: positions with Poisson molecule counts, molecules with Poisson
    template counts on both strands, UMI bases wrong at `err`; in shuffled record order."""
    rng = random.Random(seed)

    def poisson(lam):
        k, p, L = 0, 1.0, 2.718281828 ** -lam
        while True:
            p *= rng.random()
            if p <= L:
                return k
            k += 1
    tpls, t = [], 0
    while t < n_templates:
        ref, p1 = rng.randrange(3), rng.randrange(1, 4000)
        p2 = p1 + rng.randrange(50, 400)
        for _ in range(1 + poisson(1.5)):
            u = ["".join(rng.choice("ACGT") for _ in range(6)) for _ in range(2)]
            for _ in range(1 + poisson(2.0)):
                top = rng.random() < 0.5
                h = ["".join(rng.choice("ACGT") if rng.random() < err else b for b in x) for x in u]
                tpls.append(tpl("s%06d" % t, "-".join(h if top else h[::-1]), p1, p2, top, ref))
                t += 1
    recs = [r for x in tpls for r in x]
    rng.shuffle(recs)
    return recs

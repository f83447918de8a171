"""Alignment-edge input builder (a plain helper module, like edge_inputs.py, whose genome and
bisulfite read model it reuses).

edge_inputs.build writes every record as one `L M` cigar with a truthful `MC:Z:<Lm>M`.  This
module builds step-5 input from an explicit per-record description instead -- cigar string,
position, flag, MI strand and the mate fields (PNEXT, TLEN, MC), which a case may write stale on
purpose, plus base / quality overrides at read offsets -- so a test can put a record exactly on
an edge of what its alignment decides: the read-through trim, the trailing-N trim, the
most-common-alignment filter and the overlap consensus across indels.  Reads are 24-48 bases
(but where a case says otherwise), a case holds a few dozen families, and everything is
deterministic for a given seed.

Tool 1 drops converted-class records (flags 1 / 83 / 163) that carry I / D / H and tool 2 drops
every record with H, so most cases run the caller alone (Case.run_tools False: the records stand
for tool-2 output); `tools_case` keeps its indels on pass-through records (99 / 147) and runs
with the tools.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

import edge_inputs as E
from bsseqconsensusreads_amd import records as R

SPACING = 160  # families sit this far apart: no template's keys interleave with a neighbour's


@dataclass
class Rec:
    """One input record.  pos: absolute, of the first aligned base.  at: read offset -> (nt16
    base code or None to keep the modelled base, quality or None)."""
    name: str
    flag: int
    pos: int
    cigar: str
    strand: str            # "A" | "B" (MI k/A, k/B)
    next_pos: int
    tlen: int
    mc: Optional[str]      # None: no MC tag
    next_tid: int = 0
    q: Optional[int] = None  # one quality for the whole read (default: edge_inputs.q_bins)
    at: Dict[int, Tuple[Optional[int], Optional[int]]] = field(default_factory=dict)

    @property
    def ops(self):
        return [(c & 0xF, c >> 4) for c in R.parse_cigar_string(self.cigar)]

    @property
    def read_len(self) -> int:
        return sum(l for op, l in self.ops if op in (R.OP_M, R.OP_I, R.OP_S, R.OP_EQ, R.OP_X))

    @property
    def ref_len(self) -> int:
        return sum(l for op, l in self.ops if op in R.REF_CONSUMING)


@dataclass
class Fam:
    """One MI family: its records in input order, and what the case expects of it -- expect_lens:
    per set (0 AB-R1, 1 AB-R2, 2 BA-R1, 3 BA-R2) the source lengths the vote must see, in the
    filter's order (written by hand in the case); any other key is the case's own."""
    what: str
    recs: List[Rec]
    expect_lens: Optional[Dict[int, List[int]]] = None
    note: dict = field(default_factory=dict)


@dataclass
class Case:
    name: str
    fams: List[Fam]
    run_tools: bool
    raw: R.RawRecords = None
    ref: R.Reference = None


def ref_len_of(cigar: str) -> int:
    return sum(c >> 4 for c in R.parse_cigar_string(cigar) if (c & 0xF) in R.REF_CONSUMING)


def pair(name: str, strand: str, top: bool, fwd: Tuple[int, str], rev: Tuple[int, str], stale_fwd: Optional[dict] = None,
         stale_rev: Optional[dict] = None, **kw) -> List[Rec]:
    """One template as [R1, R2]: a forward record (pos, cigar) and a reverse one.  top: R1 is the
    forward record (99 / 147), else the reverse one (83 / 163).  The mate fields are truthful --
    PNEXT the mate's position, MC its cigar, TLEN from the forward start to the reverse end -- but
    where stale_fwd / stale_rev (keys next_pos, tlen, mc, next_tid, flag) say otherwise."""
    (pf, cf), (pr, cr) = fwd, rev
    tl = pr + ref_len_of(cr) - pf
    f = Rec(name, 99 if top else 163, pf, cf, strand, pr, tl, cr, **kw)
    r = Rec(name, 147 if top else 83, pr, cr, strand, pf, -tl, cf, **kw)
    for rec, st in ((f, stale_fwd), (r, stale_rev)):
        for k, v in (st or {}).items():
            setattr(rec, k, v)
    return [f, r] if top else [r, f]


def build(name: str, fams: List[Fam], run_tools: bool, seed: int = 1, second_contig: bool = False) -> Case:
    """The families as one record stream (family-major, each family's records in the order
    given) on one contig that holds them (second_contig: and a short second one, for mates that
    claim to lie there)."""
    rng = np.random.default_rng(seed)
    glen = max(r.pos + r.ref_len for f in fams for r in f.recs) + 100
    genome = E.make_genome(glen, rng)
    b = R._Builder()
    for k, f in enumerate(fams):
        for rec in f.recs:
            L = rec.read_len
            q = np.full(L, rec.q, np.uint8) if rec.q is not None else np.asarray(E.q_bins(rng, [L])[0], np.uint8)
            top = (rec.flag & 0x40 != 0) == (rec.flag & 16 == 0)  # R1 forward or R2 reverse: the top strand
            seq = np.zeros(L, np.uint8)
            rp, qp = rec.pos, 0
            for op, l in rec.ops:
                if op in (R.OP_M, R.OP_EQ, R.OP_X):
                    seq[qp:qp + l] = E._read(genome, k, rp, l, top, q[qp:qp + l], rng)
                elif op in (R.OP_I, R.OP_S):
                    seq[qp:qp + l] = np.array([E.A, E.C, E.G, E.T], np.uint8)[rng.integers(0, 4, size=l)]
                if op in R.REF_CONSUMING:
                    rp += l
                if op in (R.OP_M, R.OP_I, R.OP_S, R.OP_EQ, R.OP_X):
                    qp += l
            for o, (bb, qq) in rec.at.items():
                if bb is not None:
                    seq[o] = bb
                if qq is not None:
                    q[o] = qq
            tags = [("MI", "Z", "%d/%s" % (k, rec.strand))] + ([("MC", "Z", rec.mc)] if rec.mc is not None else [])
            b.add(("f%03d%s" % (k, rec.name)).encode(), rec.flag, 0, rec.pos, 60, R.parse_cigar_string(rec.cigar), seq, q,
                  rec.next_tid, rec.next_pos, rec.tlen, R.encode_aux(tags), tags)
    names, codes = ["chrE"], [genome]
    if second_contig:
        names.append("chrF")
        codes.append(E.make_genome(200, rng))
    return Case(name, fams, run_tools, b.finish(), R.Reference.from_codes(names, codes))


def _start(k: int) -> int:
    return 100 + SPACING * k


# ---- cigar shapes ------------------------------------------------------------------------------
# every read 30 bases (the hard clips aside: they hold no bases)
SHAPES = (
    "1M1I28M", "1M3I26M", "28M1I1M", "15M2I13M", "15M5I10M",            # I of 1 and 2-5: offset 1, last, middle
    "1M1D29M", "1M4D29M", "29M1D1M", "15M3D15M", "15M5D15M",            # D likewise
    "10M2I3D18M", "10M3D2I18M",                                          # I directly next to D
    "12M6N18M",                                                          # an N op
    "10=1X19=", "10=2I3X15=",                                            # = and X in place of M
    "8M1I8M2D13M", "5M1I5M2D5M1I13M",                                 # two and three indels
    "2M1I2M1D2M1I2M1D2M1I2M1D2M1I2M1D10M",                               # 17 ops on 30 bases
    "1S29M", "29M1S", "1S28M1S", "25S5M", "5M25S", "12S6M12S",           # soft clips of 1 and of most of the read
    "5H30M", "30M4H", "3H2S28M", "28M2S3H",                              # a hard clip alone and next to a soft clip
    "29S1M", "1M29S",                                                    # one base left aligned
)


def shapes_case(seed: int = 21) -> Case:
    """One family per shape, the caller alone: an AB template (99 / 147) and a BA template
    (83 / 163) whose four records all carry the shape -- forward and reverse, R1 and R2, AB and BA
    -- the forward records at the family's start and the reverse ones 12 bases on, so the mates
    overlap across the shape.  X = {AB-R1, BA-R2} and Y = {AB-R2, BA-R1} each hold one cigar, so
    the filter groups them and rejects nothing: every set keeps its one read whole."""
    fams = []
    for k, c in enumerate(SHAPES):
        s = _start(k)
        L = Rec("", 0, 0, c, "A", 0, 0, None).read_len
        recs = pair("a", "A", True, (s, c), (s + 12, c)) + pair("b", "B", False, (s, c), (s + 12, c))
        fams.append(Fam(c, recs, {0: [L], 1: [L], 2: [L], 3: [L]}))
    return build("shapes", fams, False, seed)


def tools_case(seed: int = 22) -> Case:
    """With the tools: indels and soft clips on pass-through records only.  Per shape a family of
    two AB templates (99 / 147) carrying it and one plain BA template (83 / 163, converted by tool
    1 and extended by tool 2): in X the two AB-R1 reads outvote BA-R2's plain cigar, in Y the two
    AB-R2 reads BA-R1's, so the filter rejects one read on each side."""
    fams = []
    for k, c in enumerate(("1M1I34M", "34M1I1M", "15M2I19M", "15M3D21M", "10M2I3D24M", "12M6N24M", "8M1I8M2D19M",
                           "2M1I2M1D2M1I2M1D2M1I2M1D22M", "3S33M", "33M3S")):
        s = _start(k)
        recs = pair("a", "A", True, (s, c), (s + 14, c)) + pair("b", "A", True, (s, c), (s + 14, c)) + \
            pair("c", "B", False, (s, "36M"), (s + 14, "36M"))
        fams.append(Fam(c, recs))
    return build("tools", fams, True, seed)


# ---- overlap consensus across indels -------------------------------------------------------------
def overlap_case(wild: bool = False, seed: int = 23) -> Case:
    """Single AB templates, the caller alone, so each set holds one read and the source reads are
    the records after the overlap consensus.  note["first"] / note["last"]: the first and last
    reference position both mates cover.  wild: one quality byte of 200 in each family (outside
    the overlap: the `wild` path runs, the expected values stay)."""
    F = []

    def fam(what, cf, cr, shift, **note):
        s = _start(len(F))
        recs = pair("a", "A", True, (s, cf), (s + shift, cr), q=30)
        recs[1].at[0] = (E.A, 20)  # R2's first base (the overlap's first position where R1 has a base there): A at Q20
        if wild:
            recs[0].at[0] = (None, 200)
        F.append(Fam(what, recs, {0: [recs[0].read_len], 1: [recs[1].read_len]}, note))

    fam("insertion in R1 inside the overlap", "20M3I13M", "36M", 10)
    fam("insertion in R2 inside the overlap", "36M", "10M3I23M", 10)
    fam("deletion in R1 inside the overlap", "20M4D16M", "36M", 10)
    fam("deletion in R2 inside the overlap", "36M", "10M4D26M", 10)
    fam("indels in both mates at different places", "14M2I20M", "18M3D18M", 8)
    fam("overlap begins on the base after R1's deletion", "20M4D16M", "36M", 24)
    fam("overlap begins inside R1's deletion", "20M4D16M", "36M", 22)
    fam("overlap ends on the base before R2's insertion", "30M", "1M3I26M", 29)
    fam("overlap ends on R1's last base, R2's deletion next", "30M", "1M2D29M", 29)
    fam("overlap of one position", "30M", "30M", 29)
    fam("overlap of one position, both complex", "10M1I19M", "20M1D10M", 28)
    fam("no overlap: the mates abut", "30M", "30M", 30)
    return build("overlap_wild" if wild else "overlap", F, False, seed)


# ---- read-through trim, trailing Ns, source reads ------------------------------------------------
def trim_case(seed: int = 24) -> Case:
    """Single AB templates, the caller alone, so no filter runs and each set's one source read
    is the record after its trims.  Each family names, per record, the stale or truthful mate
    fields; the expected kept lengths are derived in the test from this description."""
    F = []
    N2 = (E.N, 2)

    def fam(what, fwd, rev, stale_fwd=None, stale_rev=None, at_fwd=None, at_rev=None, **note):
        s = _start(len(F))
        recs = pair("a", "A", True, (s + fwd[0], fwd[1]), (s + rev[0], rev[1]),
                    stale_fwd={k: (v + s if k == "next_pos" else v) for k, v in (stale_fwd or {}).items()},
                    stale_rev={k: (v + s if k == "next_pos" else v) for k, v in (stale_rev or {}).items()})
        recs[0].q, recs[1].q = 35, 30  # (unequal: the overlap consensus then makes no N of its own)
        recs[0].at.update(at_fwd or {})
        recs[1].at.update(at_rev or {})
        F.append(Fam(what, recs, None, note))

    # forward record 0..29; the reverse mate ends d bases before the forward record does
    for d in (-3, -2, -1, 0, 1, 2, 12):
        fam("simple forward ends %d past the mate's end" % d, (0, "30M"), (0, "%dM" % (30 - d)))
    # reverse record starts d bases before the forward mate does
    for d in (-3, -2, -1, 0, 1, 2, 12):
        fam("simple reverse starts %d before the mate's start" % d, (10, "30M"), (10 - d, "%dM" % (30 + d)))
    # complex records: the boundary around a deletion (reference 10..12) and an insertion (read 10..12)
    for e in (8, 9, 10, 11, 12, 13, 14):
        fam("forward 10M3D20M, mate ends at +%d" % e, (0, "10M3D20M"), (0, "%dM" % (e + 1)))
    for e in (8, 9, 10, 11):
        fam("forward 10M3I17M, mate ends at +%d" % e, (0, "10M3I17M"), (0, "%dM" % (e + 1)))
    for b in (16, 17, 18, 19, 20, 21, 22):  # reverse 20M3D10M at 0: deletion at reference 20..22
        fam("reverse 20M3D10M, mate starts at +%d" % b, (b, "30M"), (0, "20M3D10M"))
    for b in (16, 17, 18, 19):  # reverse 17M3I10M at 0: the insertion between reference 16 and 17
        fam("reverse 17M3I10M, mate starts at +%d" % b, (b, "30M"), (0, "17M3I10M"))
    # complex records the candidate window passes but the trim leaves whole, and ones outside it
    for d in (-3, -2, -1, 0):
        fam("forward 10M2I18M1D2M ends %d past the mate's end" % d, (0, "10M2I18M1D2M"), (0, "%dM" % (31 - d)))
    # a trim to nothing: the mate claims to end before this record starts
    fam("forward trimmed to 0 bases", (20, "30M"), (0, "30M"), stale_fwd={"next_pos": 0, "mc": "10M", "tlen": 5})
    # (a reverse record cannot lose everything: PNEXT must lie before its last base for the pair to count as FR)
    fam("reverse trimmed to its last 2 bases", (0, "30M"), (0, "30M"), stale_rev={"next_pos": 28, "mc": "10M"})
    # a trim that uncovers trailing Ns (sequencing order: the forward read's bases before the cut,
    # the reverse read's after it)
    fam("forward trim uncovers 3 Ns", (0, "30M"), (0, "20M"), at_fwd={17: N2, 18: N2, 19: N2})
    fam("reverse trim uncovers 2 Ns", (10, "30M"), (0, "36M"), at_rev={10: N2, 11: N2})
    fam("complex forward trim uncovers Ns", (0, "10M3D20M"), (0, "16M"), at_fwd={11: N2, 12: N2})
    # MC with clips: the unclipped mate ends move by them
    fam("MC 3S20M: forward sees the mate end at +19", (0, "30M"), (0, "20M"), stale_fwd={"mc": "3S20M"})
    fam("MC 20M4S: mate end +4", (0, "30M"), (0, "20M"), stale_fwd={"mc": "20M4S"})
    fam("MC 20M2S3H: mate end +5", (0, "30M"), (0, "20M"), stale_fwd={"mc": "20M2S3H"})
    fam("MC 2H3S30M: reverse sees the mate start 5 earlier", (10, "30M"), (0, "36M"), stale_rev={"mc": "2H3S30M"})
    fam("MC 4S30M3H: mate start 4 earlier", (10, "30M"), (0, "36M"), stale_rev={"mc": "4S30M3H"})
    fam("MC 12S30M: mate start before this record, no trim", (10, "30M"), (0, "36M"), stale_rev={"mc": "12S30M"})
    # preconditions that switch the trim off (each record would lose 10 bases otherwise)
    fam("tlen 0", (0, "30M"), (0, "20M"), stale_fwd={"tlen": 0})
    fam("tlen of the wrong sign", (0, "30M"), (0, "20M"), stale_fwd={"tlen": -20})
    fam("reverse, PNEXT past its own end", (10, "30M"), (0, "36M"), stale_rev={"next_pos": 36})
    fam("flag & 32 equal to flag & 16 (forward)", (0, "30M"), (0, "20M"), stale_fwd={"flag": 99 & ~32})
    fam("flag & 32 equal to flag & 16 (reverse)", (10, "30M"), (0, "36M"), stale_rev={"flag": 147 | 32})
    fam("mate on another contig", (0, "30M"), (0, "20M"), stale_fwd={"next_tid": 1})
    fam("no MC", (0, "30M"), (0, "20M"), stale_fwd={"mc": None})
    fam("no MC (reverse)", (10, "30M"), (0, "36M"), stale_rev={"mc": None})
    # source reads
    alln = {o: N2 for o in range(30)}
    fam("all-N forward read: AB-R1 empty", (0, "30M"), (6, "30M"), at_fwd=alln)
    fam("all-N reverse read: AB-R2 empty", (0, "30M"), (6, "30M"), at_rev=alln)
    fam("forward read whose only base is the first", (0, "30M"), (6, "30M"), at_fwd={o: N2 for o in range(1, 30)})
    fam("reverse read whose only base is the first in record order", (0, "30M"), (6, "30M"),
        at_rev={o: N2 for o in range(1, 30)})
    fam("reverse read with a leading N run in record order", (0, "30M"), (6, "30M"), at_rev={o: N2 for o in range(0, 7)})
    fam("forward complex read with a trailing N run across its insertion", (0, "20M3I7M"), (6, "30M"),
        at_fwd={o: N2 for o in range(21, 30)})
    # a set emptied by a trim while the other strand survives: AB and BA templates, AB-R1 gone,
    # so the first duplex read comes from BA-R2 alone and X holds one live set beside an empty one
    for what, at, stale in (("AB-R1 all N, BA survives", alln, None),
                            ("AB-R1 trimmed to 0 bases, BA survives", None, {"next_pos": -20, "mc": "10M", "tlen": 5})):
        s = _start(len(F))
        ab = pair("a", "A", True, (s, "30M"), (s + 6, "30M"),
                  stale_fwd={k: (v + s if k == "next_pos" else v) for k, v in (stale or {}).items()})
        ba = pair("b", "B", False, (s, "30M"), (s + 6, "30M"))
        for t in (ab, ba):
            for rec in t:
                rec.q = 30 if rec.flag & 16 else 35
        ab[0].at.update(at or {})
        F.append(Fam(what, ab + ba, None, {}))
    return build("trim", F, False, seed, second_contig=True)


# ---- the most-common-alignment filter --------------------------------------------------------------
def filter_case(seed: int = 25) -> Case:
    """The caller alone.  Each family's X side (AB-R1 forward, BA-R2 forward) or Y side (AB-R2
    reverse, BA-R1 reverse) holds the cigars named; the other side is plain 30M.  Template
    names order the reads inside a set (TemplateCoordinate ties break on the name), source
    lengths are chosen distinct so the survivors can be told by length.  expect_lens is written
    by hand from fgbio's rule: sort by source length descending (stable), a read joins every
    group whose defining cigar it is a prefix of or opens a group, the first largest group wins."""
    F = []

    def fam(what, x, y=None, expect=None, stale=None, ba=(), ba_top=False, **note):
        """x, y: per template its forward / reverse cigar (y default 30M each); ba: indices of the
        BA templates (bottom strand: 83 / 163, so their forward record is R2 and lands in X;
        ba_top: flagged 99 / 147 like the AB ones, so their REVERSE record is the R2 in X)."""
        s = _start(len(F))
        y = y or ["30M"] * len(x)
        recs = []
        for t, (cx, cy) in enumerate(zip(x, y)):
            is_ba = t in ba
            recs += pair("t%02d" % t, "B" if is_ba else "A", ba_top or not is_ba, (s, cx), (s + 50, cy),
                         stale_fwd={k: (v + s if k == "next_pos" else v) for k, v in (stale or {}).get(t, {}).items()}, q=30)
        F.append(Fam(what, recs, expect, note))

    a, b, c = "10M2I20M", "12M2I16M", "14M1D14M"  # 32, 30 and 28 bases, pairwise incompatible
    fam("2 against 1", [a, a, b], expect={0: [32, 32], 1: [30, 30, 30]}, rejected=1)
    fam("1 against 2", [a, b, b], expect={0: [30, 30], 1: [30, 30, 30]}, rejected=1)
    fam("2 against 2: the first-defined (longer) group wins", [b, b, a, a], expect={0: [32, 32], 1: [30] * 4}, rejected=2)
    fam("2 against 2, equal lengths: the first in input order wins", ["10M2I18M", "12M2I16M", "10M2I18M", "12M2I16M"],
        expect={0: [30, 30], 1: [30] * 4}, rejected=2, groups=2)
    fam("three groups 1 / 2 / 3", [a, b, b, c, c, c], expect={0: [28, 28, 28], 1: [30] * 6}, rejected=3, groups=3)
    fam("three singletons: all but the longest rejected", [c, b, a], expect={0: [32], 1: [30] * 3}, rejected=2, groups=3)
    fam("a short M-only read is a prefix of two definers, which tie at 2", ["26M2I10M", "25M1D13M", "24M"],
        expect={0: [38, 24], 1: [30] * 3}, rejected=1, groups=2)
    fam("the same, the second group one larger", ["26M2I10M", "25M1D13M", "25M1D12M", "24M"],
        expect={0: [38, 37, 24], 1: [30] * 4}, rejected=1, groups=2)
    fam("insertions of different lengths at one offset", ["10M1I20M", "10M2I20M", "10M1I20M"],
        expect={0: [31, 31], 1: [30] * 3}, rejected=1, groups=2)
    # compatible only after the read-through trim cuts it before its insertion: the mate claims to end at +14
    fam("a cigar compatible only once truncated at srclen", ["20M2I10M", "18M1D12M", "18M1D12M"],
        stale={0: {"next_pos": 0, "mc": "15M", "tlen": 15}}, expect={0: [30, 30, 15], 1: [30] * 3}, rejected=0, groups=1)
    fam("the same without the trim: rejected", ["20M2I10M", "18M1D12M", "18M1D12M"],
        expect={0: [30, 30], 1: [30] * 3}, rejected=1, groups=2)
    # X = AB-R1 + BA-R2, both forward here; Y = AB-R2 + BA-R1, both reverse: the reversed cigar walk
    fam("one indel from AB-R1 and BA-R2", [a, a, b], ba=(1,), expect={0: [32], 3: [32], 1: [30, 30], 2: [30]}, rejected=1)
    fam("one indel from a forward AB-R1 and a reverse BA-R2", [a, "30M", b], y=["30M", "20M2I10M", "30M"], ba=(1,), ba_top=True,
        expect={0: [32], 3: [32], 1: [30, 30], 2: [30]}, rejected=1)
    fam("Y filtered, X untouched", ["30M"] * 3, y=["20M2I10M", "20M2I10M", "16M2I12M"],
        expect={0: [30] * 3, 1: [32, 32]}, rejected=1)
    fam("Y: the reverse records' cigars compared in sequencing order", ["30M"] * 3, y=["20M2I10M", "20M2I10M", "10M2I20M"],
        expect={0: [30] * 3, 1: [32, 32]}, rejected=1)
    fam("X and Y both filtered, BA in the minority", [a, a, b], y=["8M1D22M", "8M1D22M", "9M1D21M"], ba=(2,),
        expect={0: [32, 32], 1: [30, 30], 2: [], 3: []}, rejected=2)
    return build("filter", F, False, seed)


NEAR_TIE_COLUMNS = tuple(range(1, 10)) + tuple(range(12, 29))  # read offsets beside the insertion at 10


def near_tie_case(seed: int = 26) -> Case:
    """Near ties in a set the filter has reordered: X holds reads of one complex cigar family
    (10M1I19M and its longer form 10M1I23M, prefix-compatible) with the LONGER reads later in
    input order, plus one incompatible read it rejects.  At every offset of NEAR_TIE_COLUMNS the
    two short reads (t0, t1) show one base and the two long ones (t2, t3) another, at qualities
    (qa, qb) and (qb, qa): the same quality multiset on both bases, so the true likelihoods tie and
    the pick is the rounding of fgbio's fp64 sums, which run in the filter's order (t2, t3, t0,
    t1: longest first), not in input order.  The two orders give different term sequences
    (b2, b2, b1, b1 against b1, b1, b2, b2); tests/test_align_inputs.py shows columns where they
    pick differently."""
    rng = np.random.default_rng(seed)
    bases = np.array([E.A, E.C, E.G, E.T], np.uint8)
    F = []
    for k in range(8):
        s = _start(k)
        recs = []
        cols = {o: (rng.permutation(bases)[:2], int(rng.integers(60, 94)), int(rng.integers(60, 94))) for o in NEAR_TIE_COLUMNS}
        for t, cx in enumerate(("10M1I19M", "10M1I19M", "10M1I23M", "10M1I23M", "8M2D22M")):
            p = pair("t%02d" % t, "A", True, (s, cx), (s + 50, "30M"), q=30)
            if t < 4:
                for o, ((b1, b2), qa, qb) in cols.items():
                    p[0].at[o] = (int(b1 if t < 2 else b2), qa if t in (0, 3) else qb)
            recs += p
        F.append(Fam("near ties", recs, {0: [34, 34, 30, 30], 1: [30] * 5}, {"rejected": 1}))
    return build("near_tie", F, False, seed)


# ---- the filter's group count ------------------------------------------------------------------------
GROUP_SINGLES = 70


def group_count_case(trio_first: bool, seed: int = 27) -> Case:
    """One family of 73 AB templates (146 records: k_large at any routing) whose X side holds
    GROUP_SINGLES pairwise incompatible cigars (aM bI cM, every (a, b) once) and three reads that
    share 12M2D28M.  trio_first False: the singles are the longer reads (44 against 40 bases), so
    the trio's group is the 71st defined and the only one of size 3 -- fgbio keeps the trio.
    trio_first True (the control): the trio is longer (46 bases) and defines group 0.  Two small
    plain families beside it keep the case's emitted share up."""
    s = _start(0)
    singles = [(a, b) for b in (1, 2, 3, 4) for a in range(2, 20)][:GROUP_SINGLES]
    trio = "12M2D34M" if trio_first else "12M2D28M"
    x = ["%dM%dI%dM" % (a, b, 44 - a - b) for a, b in singles] + [trio] * 3
    recs = []
    for t, cx in enumerate(x):
        recs += pair("t%02d" % t, "A", True, (s, cx), (s + 60, "30M"), q=30)
    L = 46 if trio_first else 40
    fams = [Fam("70 singleton groups and a trio", recs, {0: [L] * 3, 1: [30] * 73}, {"rejected": GROUP_SINGLES, "groups": 71})]
    for k in (1, 2):
        s = _start(k)
        fams.append(Fam("plain", pair("a", "A", True, (s, "10M1I19M"), (s + 12, "30M")) +
                        pair("b", "B", False, (s, "10M1I19M"), (s + 12, "30M")), {0: [30], 1: [30], 2: [30], 3: [30]}))
    return build("groups_control" if trio_first else "groups", fams, False, seed)


# ---- the filter's op slots ------------------------------------------------------------------------------
SLOT_CIGAR = "2M1I2M1D2M1I2M1D2M1I2M1D2M1I2M1D10M"  # 17 ops: 19 slots a record


@functools.lru_cache(maxsize=None)
def slot_family(n_templates: int, seed: int = 28) -> Case:
    """(Built once per size; the tests leave it unchanged.)  One AB-only family of n_templates templates whose forward records all carry SLOT_CIGAR (one
    group in the filter); the reverse records are plain."""
    s = _start(0)
    recs = []
    for t in range(n_templates):
        recs += pair("t%05d" % t, "A", True, (s, SLOT_CIGAR), (s + 40, "30M"), q=30)
    return build("slots", [Fam("slots", recs)], False, seed)


CASES = {"shapes": shapes_case, "tools": tools_case, "overlap": overlap_case, "overlap_wild": lambda: overlap_case(True),
         "trim": trim_case, "filter": filter_case, "near_tie": near_tie_case,
         "groups": lambda: group_count_case(False), "groups_control": lambda: group_count_case(True)}
_cache: Dict[str, Case] = {}


def case(name: str) -> Case:
    """The named case, built once per session (the tests leave it unchanged)."""
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]

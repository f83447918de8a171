"""Edge-input builder for the parity tests (a plain helper module, like helpers.py).

synth.generate draws qualities from {37, 25, 12, 2}, one read length per run and family sizes from
a distribution.  This module builds step-5 input from an explicit per-family description instead
-- the number of AB and BA templates, every record's read length, the fragment's start and
length, a quality sampler -- so a test can put a family exactly on a kernel's edge: quality bytes
over the whole byte range, reads of 1 base, 64 against 65 records, max_len + 2 beside a multiple
of 16.  Pairing, flags (99/147 top, 83/163 bottom), MC, MI k/A | k/B, PNEXT/TLEN and the
bisulfite base model follow synth.generate; the records go through records._Builder, so the same
tool-1 / tool-2 / overlap code runs on them as on the configs.  The reference is one short
contig holding the input, with reads at position 0 and at the contig end.  Deterministic for a
given seed.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from bsseqconsensusreads_amd import records as R

A, C, G, T, N = 1, 2, 4, 8, 15

# the length sets of the read-length cases
LENGTH_SETS = {"tiny": (1, 2, 3, 4, 5, 7, 8, 9), "l16": (13, 14, 15, 16, 17, 18), "l32": (29, 30, 31, 32, 33, 34),
               "l64": (61, 62, 63, 64, 65, 66)}
# family sizes (records) where the code changes behaviour: k_small / k_large routing (64 | 65),
# k_large's partial-sum flush and deep-set path (64 | 65, 128 | 129 reads per set), MAX_PART_REC
# and the u8 depth saturation (254 | 255), WIDE_MIN_RECORDS (256)
FAMILY_SIZES = (1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 130, 254, 255, 256, 257, 258, 300)
DEEP_FAMILY = 520  # one more family: AB-only its sets hold 260 reads, a column depth past a byte
# error rates (pre-UMI, post-UMI) of the parameter cases; ACCEPTED is the library's domain
# (include/bsdc.h: pre below 46.999), REFUSED must fail cleanly
RATES_ACCEPTED = ((45.0, 30.0), (40.0, 20.0), (30.0, 20.0), (10.0, 5.0))
RATES_REFUSED = ((60.0, 40.0), (93.0, 93.0))


# ---- quality samplers: (rng, read lengths of the records) -> one uint8 array per record ----------
def q_bins(rng, lens):
    """synth.generate's bins (no Q2: Ns come from the base model here)."""
    return [rng.choice(np.array([37, 25, 12], np.uint8), size=int(n), p=[0.8, 0.15, 0.05]) for n in lens]


def q_full_range(rng, lens):
    """Uniform in 0..93: mates then often carry equal qualities (N / 2), sums above 93 (the cap)
    and small differences."""
    return [rng.integers(0, 94, size=int(n)).astype(np.uint8) for n in lens]


def q_high(rng, lens):
    """94..127: every overlap sum is 188..254, the SWAR overlap's branch for sums of 128 and over."""
    return [rng.integers(94, 128, size=int(n)).astype(np.uint8) for n in lens]


def q_wild(rng, lens):
    """About 5 % of the records with every quality byte 0xFF (BAM's missing quality), another 5 %
    with scattered bytes in 128..254, the rest uniform in 0..93."""
    out = []
    for n in lens:
        n = int(n)
        u = rng.random()
        q = rng.integers(0, 94, size=n).astype(np.uint8)
        if u < 0.05:
            q[:] = 0xFF
        elif u < 0.10:
            hit = rng.random(n) < 0.3
            hit[int(rng.integers(0, n))] = True
            q[hit] = rng.integers(128, 255, size=int(hit.sum())).astype(np.uint8)
        out.append(q)
    return out


SAMPLERS = {"bins": q_bins, "full_range": q_full_range, "high": q_high, "wild": q_wild}


@dataclass
class Family:
    """One MI family: n_ab + n_ba templates on the fragment [start, start + frag) of the contig.
    lens[t] = (R1 length, R2 length) of template t (AB templates first); unpaired_r1: one more AB
    template of which only R1 exists (an odd record count); ab_top: the AB strand is the top one
    (99/147), BA then the bottom (83/163)."""
    n_ab: int
    n_ba: int
    lens: List[Tuple[int, int]]
    start: int
    frag: int
    ab_top: bool = True
    unpaired_r1: Optional[int] = None  # its read length

    @property
    def n_records(self) -> int:
        return 2 * (self.n_ab + self.n_ba) + (self.unpaired_r1 is not None)


@dataclass
class EdgeSet:
    raw: R.RawRecords
    ref: R.Reference
    families: List[Family] = field(default_factory=list)


def _hash_u01(a, b):
    """Deterministic uniform [0, 1) per (family, site): the molecule's methylation, shared by both
    strands and every copy (synth._hash_u01)."""
    u = np.uint64
    m = u(0x3FFFFFFFFFFFFFFF)  # (the low 62 bits of a product do not depend on the wrap at 2^64)
    with np.errstate(over="ignore"):
        x = (np.asarray(a, np.int64).astype(u) * u(0x9E3779B1) + np.asarray(b, np.int64).astype(u) * u(0x85EBCA77)
             + u(0x27D4EB2F)) & m
        x = ((x ^ (x >> u(31))) * u(0x2545F4914F6CDD1D)) & m
    x = x ^ (x >> u(29))
    return (x & u(0xFFFFFF)).astype(np.float64) / float(1 << 24)


def make_genome(n, rng):
    u = rng.random(n)
    g = np.full(n, T, np.uint8)
    g[u < 0.705] = G
    g[u < 0.5] = C
    g[u < 0.295] = A
    return g


def _read(genome, fam, pos, L, top, q, rng, extra_error=0.0):
    """Bases of a read of L bases at pos: the reference with the strand's bisulfite conversion
    (top: unmethylated C -> T, bottom: unmethylated G -> A; CpG methylated with p = 0.75, other
    cytosines 0.005), sequencing errors at each base's own quality (and, with extra_error, at that
    rate whatever the quality: mates and copies that disagree at high qualities), Q2 bases N."""
    p = pos + np.arange(L, dtype=np.int64)
    n = genome.shape[0]
    ref = genome[p]
    nxt = genome[np.minimum(p + 1, n - 1)]
    prv = genome[np.maximum(p - 1, 0)]
    cpg_top = (ref == C) & (nxt == G)
    cpg_bot = (ref == G) & (prv == C)
    site = p if top else np.where(cpg_bot, p - 1, p)
    meth = _hash_u01(np.full(L, fam), site) < np.where(cpg_top if top else cpg_bot, 0.75, 0.005)
    b = ref.copy()
    if top:
        b[(ref == C) & ~meth] = T
    else:
        b[(ref == G) & ~meth] = A
    err = rng.random(L) < np.maximum(np.power(10.0, -q.astype(np.float64) / 10.0), extra_error)
    alt = np.array([A, C, G, T], np.uint8)[rng.integers(0, 4, size=L)]
    alt = np.where(alt == b, np.where(b == A, T, A), alt).astype(np.uint8)
    b = np.where(err, alt, b)
    b = np.where(q == 2, N, b)
    return b.astype(np.uint8)


def build(families: Sequence[Family], quals: Callable = q_bins, seed: int = 1, contig_len: Optional[int] = None,
          contig: str = "chrE", extra_error: float = 0.0) -> EdgeSet:
    """The families as one record stream (family-major, position-ordered inside a family, R1 first
    on ties) and its one-contig reference.  contig_len defaults to the end of the last fragment."""
    rng = np.random.default_rng(seed)
    glen = int(contig_len if contig_len is not None else max(f.start + f.frag for f in families))
    assert all(f.start >= 0 and f.start + f.frag <= glen for f in families)
    genome = make_genome(glen, rng)
    b = R._Builder()
    tmpl = 0
    for k, f in enumerate(families):
        assert len(f.lens) == f.n_ab + f.n_ba
        s, e = int(f.start), int(f.start + f.frag)
        recs = []
        tl = [(l1, l2, t >= f.n_ab, True) for t, (l1, l2) in enumerate(f.lens)]
        if f.unpaired_r1 is not None:
            tl.append((int(f.unpaired_r1), int(f.unpaired_r1), False, False))
        for l1, l2, is_ba, paired in tl:
            assert 1 <= l1 <= f.frag and 1 <= l2 <= f.frag
            top = f.ab_top ^ is_ba
            # top: R1 99 forward at s, R2 147 reverse ending at e; bottom: R1 83 reverse ending at e, R2 163 forward at s
            for r1 in ((True, False) if paired else (True,)):
                L, Lm = (l1, l2) if r1 else (l2, l1)
                fwd = top == r1
                pos, mpos = (s, e - Lm) if fwd else (e - L, s)
                flag = (99 if r1 else 147) if top else (83 if r1 else 163)
                recs.append((pos, 0 if r1 else 1, tmpl, flag, L, Lm, mpos, f.frag if fwd else -f.frag, top, is_ba))
            tmpl += 1
        recs.sort(key=lambda r: (r[0], r[1], r[2]))
        qs = quals(rng, [r[4] for r in recs])
        for (pos, _, t, flag, L, Lm, mpos, tlen, top, is_ba), q in zip(recs, qs):
            q = np.asarray(q, np.uint8)
            seq = _read(genome, k, pos, L, top, q, rng, extra_error)
            tags = [("MI", "Z", "%d/%s" % (k, "B" if is_ba else "A")), ("MC", "Z", "%dM" % Lm)]
            b.add(("t%d" % t).encode(), flag, 0, pos, 60, [(L << 4) | R.OP_M], seq, q, 0, mpos, tlen,
                  R.encode_aux(tags), tags)
    return EdgeSet(b.finish(), R.Reference.from_codes([contig], [genome]), list(families))


# ---- family descriptions ----------------------------------------------------------------------
def _place(rng, n_fam, frags, contig_len):
    """Fragment starts: family 0 at position 0, the last at the contig end, the rest uniform."""
    starts = [int(rng.integers(0, contig_len - fr + 1)) for fr in frags]
    starts[0] = 0
    starts[-1] = contig_len - frags[-1]
    return starts


def random_families(n_fam: int, templates: Tuple[int, int], lengths: Sequence[int], seed: int, frag_extra=(0, 12),
                    mixed: bool = True, ab_only_frac: float = 0.2, max_len: Optional[int] = None,
                    contig_len: int = 3000) -> List[Family]:
    """n_fam families of templates[0]..templates[1] templates (split Binomial(1/2), a fraction
    AB-only), every read's length drawn from `lengths` (mixed: per record; else per family), the
    fragment max(read lengths) + frag_extra[0]..frag_extra[1] long, so mates overlap nearly fully or
    not at all.  max_len: no read is longer, and family 0's first read is exactly that long."""
    rng = np.random.default_rng(seed)
    lengths = [l for l in lengths if max_len is None or l <= max_len]
    fams = []
    for k in range(n_fam):
        nt = int(rng.integers(templates[0], templates[1] + 1))
        na = nt if rng.random() < ab_only_frac else int(rng.binomial(nt, 0.5))
        if mixed:
            lens = [(int(rng.choice(lengths)), int(rng.choice(lengths))) for _ in range(nt)]
        else:
            lens = [(int(rng.choice(lengths)),) * 2] * nt
        if k == 0 and max_len is not None:
            lens[0] = (int(max_len), lens[0][1])
        frag = max(max(p) for p in lens) + int(rng.integers(frag_extra[0], frag_extra[1] + 1))
        fams.append(Family(na, nt - na, lens, 0, frag, ab_top=bool(rng.random() < 0.5)))
    for f, s in zip(fams, _place(rng, n_fam, [f.frag for f in fams], contig_len)):
        f.start = s
    return fams


def quality_case(sampler: str, seed: int = 3, n_fam: int = 150) -> EdgeSet:
    """About 150 families of 1-6 templates, L = 40, the mates overlapping by 20-40 bases; 15 % of
    the bases are wrong whatever their quality, so disagreements meet every quality."""
    fams = random_families(n_fam, (1, 6), (40,), seed, frag_extra=(0, 20), contig_len=4000)
    return build(fams, SAMPLERS[sampler], seed=seed + 1000, contig_len=4000, extra_error=0.15)


def size_case(ab_only: bool, seed: int = 5, L: int = 30, reps: int = 3, sizes: Sequence[int] = FAMILY_SIZES,
              deep: int = DEEP_FAMILY) -> EdgeSet:
    """`reps` families of exactly each size in `sizes` (records) and one of `deep`; odd counts from
    one unpaired R1.  ab_only: every template AB, so the AB-R1 / AB-R2 sets hold n / 2 reads each."""
    rng = np.random.default_rng(seed)
    fams = []
    for n in tuple(sizes) + ((deep,) if deep else ()):
        for _ in range(reps if n != deep else 1):
            nt = n // 2
            na = nt if ab_only else (nt + 1) // 2
            frag = L + int(rng.integers(0, 16))
            fams.append(Family(na, nt - na, [(L, L)] * nt, 0, frag, ab_top=bool(rng.random() < 0.5),
                               unpaired_r1=L if n % 2 else None))
    glen = 2500
    fams = [fams[int(i)] for i in rng.permutation(len(fams))]  # (the sizes in no particular order along the contig)
    for f, s in zip(fams, _place(rng, len(fams), [f.frag for f in fams], glen)):
        f.start = s
    return build(fams, q_bins, seed=seed + 1000, contig_len=glen)


def length_case(name: str, seed: int = 7, n_fam: int = 120) -> EdgeSet:
    """One of LENGTH_SETS (every record's length drawn from the set), or "mixed": lengths 1..66
    varying inside each family, as adapter trimming leaves them."""
    lengths = LENGTH_SETS[name] if name != "mixed" else tuple(range(1, 67))
    fams = random_families(n_fam, (1, 5), lengths, seed, frag_extra=(0, 6), contig_len=3000)
    return build(fams, q_full_range if name == "tiny" else q_bins, seed=seed + 1000, contig_len=3000)


def stride_case(stride_arg: int, seed: int = 9, n_fam: int = 60) -> EdgeSet:
    """A batch whose longest read is exactly stride_arg - 2 bases (max_len + 2 == stride_arg)."""
    ml = stride_arg - 2
    fams = random_families(n_fam, (1, 5), tuple(range(max(1, ml - 6), ml + 1)), seed + stride_arg, frag_extra=(0, 6),
                           max_len=ml, contig_len=2000)
    return build(fams, q_bins, seed=seed + 1000 + stride_arg, contig_len=2000)


def params_case(seed: int = 11, n_fam: int = 300) -> EdgeSet:
    """300 C2-like families (Poisson(4) templates, zero redrawn) of 40-base reads with full-range
    qualities: the input of the parameter cases."""
    rng = np.random.default_rng(seed)
    fams = []
    for _ in range(n_fam):
        nt = 0
        while nt == 0:
            nt = int(rng.poisson(4.0))
        na = int(rng.binomial(nt, 0.5))
        fams.append(Family(na, nt - na, [(40, 40)] * nt, 0, 40 + int(rng.integers(0, 30)), ab_top=bool(rng.random() < 0.5)))
    for f, s in zip(fams, _place(rng, n_fam, [f.frag for f in fams], 6000)):
        f.start = s
    return build(fams, q_full_range, seed=seed + 1000, contig_len=6000)


# ---- what a case must contain (asserted on the CPU in test_edge_inputs.py and before each GPU call) ----
def overlap_pairs(raw: R.RawRecords):
    """(q1, q2, b1, b2) over every reference position both mates of a template cover, on the raw
    input (simple cigars; the oracle's overlap consensus runs on the tool-2 records, which differ
    from these by the tools' one prepended / appended base at most)."""
    first = {}
    out = [[], [], [], []]
    for k in range(raw.n):
        key = (int(raw.mi_id[k]), int(raw.name_id[k]))
        if key not in first:
            first[key] = k
            continue
        a, b = first[key], k
        s = max(int(raw.pos[a]), int(raw.pos[b]))
        e = min(int(raw.pos[a] + raw.l_seq[a]), int(raw.pos[b] + raw.l_seq[b]))
        if e <= s:
            continue
        ia, ib = s - int(raw.pos[a]), s - int(raw.pos[b])
        out[0].append(raw.record_qual(a)[ia:ia + e - s])
        out[1].append(raw.record_qual(b)[ib:ib + e - s])
        out[2].append(raw.record_seq(a)[ia:ia + e - s])
        out[3].append(raw.record_seq(b)[ib:ib + e - s])
    return [np.concatenate(x).astype(np.int64) if x else np.zeros(0, np.int64) for x in out]


def family_has_wild(raw: R.RawRecords) -> np.ndarray:
    """Per MI family: it holds a quality byte of 128 or more."""
    n_fam = int(raw.mi_id.max()) + 1
    rec = np.repeat(np.arange(raw.n), raw.l_seq)
    has = np.zeros(n_fam, bool)
    has[raw.mi_id[rec[raw.qual >= 128]]] = True
    return has


def assert_quality_edges(sampler: str, raw: R.RawRecords):
    q1, q2, b1, b2 = overlap_pairs(raw)
    acgt = (b1 != N) & (b2 != N)
    if sampler == "full_range":
        assert int((acgt & (q1 + q2 > 93)).sum()) > 200
        assert int((acgt & (q1 == q2) & (b1 != b2)).sum()) > 50
    elif sampler == "high":
        assert q1.size > 1000 and int((q1 + q2).min()) >= 128 and int((q1 + q2).max()) <= 254
    elif sampler == "wild":
        has = family_has_wild(raw)
        assert int(has.sum()) > 10 and int((~has).sum()) > 10
        assert (raw.qual == 0xFF).any() and ((raw.qual >= 128) & (raw.qual < 0xFF)).any()

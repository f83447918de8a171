"""Fabricated inputs for the consensus filter kernel (csrc/bsdc_filter.hip): the
arrays bsdc_filter reads -- status, len, packed seq, qual, ss_len, the four single-strand rows,
ss_wide with its wide rows -- built with no vote, so that the filter's edges are met on purpose: rates
exactly at a threshold and one count to either side, depths on and beside min_reads, u16 rows up to
32767, sums past 2^31, every column position of a lane, lengths around a round, family counts around
a workgroup, and bytes a vote never writes.  A plain helper module like bamrec_inputs.py:
test_filter_rows.py checks on the CPU (with filter_ref alone) that every set holds its edges,
test_gpu_filter_rows.py runs the same sets through the kernel.

Every byte past a read's length, every row of a strand that is absent or of a family that is not
emitted, and the byte rows of a family that has a wide row are random (the `garbage` seed); what a
set is about is drawn from a seed of its own, so re-drawing the garbage changes no verdict.  Each set
is built once per process (make) and must not be modified; so is each reference (reference)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import filter_ref as FR
from filter_inputs import LAX, PARAM_SETS

A, C, G, T, N = 1, 2, 4, 8, 15
F32_THIRD = float(np.float32(1) / np.float32(3))
F32_THIRD_BELOW = float(np.nextafter(np.float32(1) / np.float32(3), np.float32(0)))
WIDE_MAX = 32767


@dataclass
class Strand:
    """one single-strand row cut to the end's length: scalars stand for every column"""
    depth: object
    err: object = 0
    base: object = A
    qual: object = 40


@dataclass
class End:
    """one consensus read: bases, qualities, its AB row `a` and BA row `b` (None: that strand is
    absent, ss_len 0).  Molecular sets use `a` alone."""
    seq: object
    qual: object
    a: Strand = None
    b: Strand = None

    @property
    def L(self):
        return len(self.seq)


def end(L, a=None, b=None, seq=A, qual=40):
    bc = lambda v: np.broadcast_to(np.asarray(v, np.int64), (L,)).copy()  # noqa: E731
    return End(bc(seq), bc(qual), a, b)


@dataclass
class FilterRows:
    name: str
    kind: int            # 0 duplex, 1 molecular (bsdc_filter's kind)
    stride: int
    status: np.ndarray   # u8 [F]
    length: np.ndarray   # i32 [F, 2]
    seq: np.ndarray      # u8 [F, 2, stride / 2] packed nt16, high nibble first
    qual: np.ndarray     # u8 [F, 2, stride]
    ss_len: np.ndarray   # i32 [F, 4]
    ss_base: np.ndarray  # u8 [F, 4, stride]
    ss_qual: np.ndarray
    ss_depth: np.ndarray
    ss_err: np.ndarray
    ss_wide: np.ndarray  # i32 [F]: the family's wide row, -1 none; None: no wide table at all
    ss_wdepth: np.ndarray  # u16 [W, 4, stride]
    ss_werr: np.ndarray
    params: dict         # name -> keyword arguments of filter_ref.apply, the sets this input runs under
    notes: dict = field(default_factory=dict)  # edge -> the family (or families) that hold it
    fam: list = field(default_factory=list)    # per family: what it was built as (a dict)

    @property
    def n_fam(self) -> int:
        return int(self.status.shape[0])

    def ref_args(self):
        """the arrays as filter_ref.apply takes them: (ss, cons_seq unpacked, cons_qual, cons_len, status)"""
        ss = {"len": self.ss_len, "base": self.ss_base, "qual": self.ss_qual, "depth": self.ss_depth, "err": self.ss_err,
              "wide": self.ss_wide, "wdepth": self.ss_wdepth, "werr": self.ss_werr}
        return ss, unpack(self.seq), self.qual, self.length, self.status

    def apply(self, p: dict):
        return FR.apply(*self.ref_args(), molecular=bool(self.kind), **p)

    def sums(self, f, e):
        """int64 (Σ a.err, Σ a.depth, Σ b.err, Σ b.depth) of family f's end e over its length (b: row 3 - e)"""
        ss = self.ref_args()[0]
        L = int(self.length[f, e])
        _, _, ad, ae = FR._row(ss, f, e, L)
        _, _, bd, be = FR._row(ss, f, 3 - e, L)
        return int(ae.sum()), int(ad.sum()), int(be.sum()), int(bd.sum())


def unpack(seq: np.ndarray) -> np.ndarray:
    return np.stack([seq >> 4, seq & 15], axis=-1).reshape(seq.shape[:-1] + (2 * seq.shape[-1],))


def pack(codes: np.ndarray) -> np.ndarray:
    return ((codes[..., 0::2] << 4) | (codes[..., 1::2] & 15)).astype(np.uint8)


class _Builder:
    def __init__(self, name, kind, stride=16):
        self.name, self.kind, self.stride = name, kind, stride
        self.fams, self.meta, self.notes = [], [], {}

    def add(self, e0, e1=None, emitted=True, wide=None, note=None, **meta):
        """a family of ends e0, e1 (e1 None: alike); wide None: a wide row iff a count needs one"""
        f = len(self.fams)
        self.fams.append((e0, e0 if e1 is None else e1, emitted, wide))
        self.meta.append(dict(meta))
        if note:
            self.notes.setdefault(note, []).append(f)
        return f

    def skip(self, note="not_emitted"):
        """a family that is not emitted: garbage throughout"""
        return self.add(None, None, emitted=False, note=note)

    def build(self, params, garbage, wide_table="auto") -> FilterRows:
        """wide_table: "auto" (a table iff some family has a wide row), "minus1" (a table whose every
        entry is -1, one garbage row behind it), "none" (no table; no family may need one)"""
        g = np.random.default_rng([garbage, 0x51F7])
        F, S = len(self.fams), self.stride
        rnd = lambda shape, dt=np.uint8, hi=256: g.integers(0, hi, shape).astype(dt)  # noqa: E731
        status = (rnd(F) & 0xFE)
        length = g.integers(0, S + 1, (F, 2)).astype(np.int32)
        codes, qual = rnd((F, 2, S), hi=16), rnd((F, 2, S))
        ss_len = g.integers(1, S + 1, (F, 4)).astype(np.int32)
        ss_base, ss_qual, ss_depth, ss_err = (rnd((F, 4, S)) for _ in range(4))
        wide = np.full(F, -1, np.int32)
        wd, we = [], []
        for f, (e0, e1, emitted, want_wide) in enumerate(self.fams):
            if not emitted:
                if g.random() < 0.5:
                    ss_len[f, g.integers(0, 4)] = 0
                continue
            status[f] |= 1
            rows = {}
            for e, x in enumerate((e0, e1)):
                L = x.L
                length[f, e] = L
                codes[f, e, :L], qual[f, e, :L] = x.seq, x.qual
                for s, r in ((e, x.a), (3 - e, x.b)):
                    if self.kind == 1 and s >= 2:
                        continue  # (never looked at: garbage, its length too)
                    if r is None:
                        ss_len[f, s] = 0
                        continue
                    ss_len[f, s] = max(L, 1)
                    rows[s] = (L, [np.broadcast_to(np.asarray(v, np.int64), (L,)) for v in (r.base, r.qual, r.depth, r.err)])
            big = any(int(v.max(initial=0)) > 255 for _, r in rows.values() for v in r[2:])
            if want_wide if want_wide is not None else big:
                wide[f] = len(wd)
                wd.append(rnd((4, S), np.uint16, WIDE_MAX + 1))
                we.append(rnd((4, S), np.uint16, WIDE_MAX + 1))
            else:
                assert not big, "family %d needs a wide row" % f
            for s, (L, (b, q, d, er)) in rows.items():
                ss_base[f, s, :L], ss_qual[f, s, :L] = b, q
                if wide[f] >= 0:  # (the byte rows stay garbage)
                    wd[-1][s, :L], we[-1][s, :L] = d, er
                else:
                    ss_depth[f, s, :L], ss_err[f, s, :L] = d, er
        if wide_table == "minus1":
            assert not wd
            table, wd, we = wide, [rnd((4, S), np.uint16, 65536)], [rnd((4, S), np.uint16, 65536)]
        elif wide_table == "none":
            assert not wd
            table = None
        else:
            table = wide if wd else None
        W = len(wd)
        return FilterRows(self.name, self.kind, S, status, length, pack(codes), qual, ss_len, ss_base, ss_qual, ss_depth,
                          ss_err, table, np.stack(wd) if W else np.zeros((0, 4, S), np.uint16),
                          np.stack(we) if W else np.zeros((0, 4, S), np.uint16), params, self.notes, self.meta)


def spread(total, caps):
    """`total` laid over the columns from the left, at most caps[j] in column j"""
    out, left = np.zeros(len(caps), np.int64), int(total)
    for j, c in enumerate(caps):
        out[j] = min(int(c), left)
        left -= out[j]
    assert left == 0, "does not fit"
    return out


def level(total, n, cap):
    """`total` laid over n columns as evenly as it goes"""
    out = np.full(n, total // n, np.int64)
    out[:total % n] += 1
    assert out.max(initial=0) <= cap
    return out


def _slots(v, others=1.0):
    """the threshold v in each of the three slots in turn, the other slots at `others`"""
    return [tuple(v if k == s else others for k in range(3)) for s in range(3)]


# ---- gate32: float32 read-rate ties ----------------------------------------------------------------

# (numerator, denominator) of a pair type k * num / k * den -> the thresholds it ties with, and
# whether the read is dropped at the tie (the float32 quotient lies above the double threshold)
GATE_PAIRS = {(1, 40): [(0.025, True)], (1, 10): [(0.1, True)], (7, 10): [(0.7, False)], (7, 20): [(0.35, False)],
              (1, 3): [(F32_THIRD, False), (F32_THIRD_BELOW, True)], (1, 8): [(0.125, False)]}
GATE_THRESHOLDS = (0.025, 0.1, 0.7, 0.35, F32_THIRD, F32_THIRD_BELOW, 0.125)
GATE_L = 8


def gate_ks(den):
    """several k: the smallest, the last whose depth sum fits byte rows, the first that needs wide
    rows, one in between and the largest wide rows hold"""
    kb, kw = GATE_L * 255 // den, GATE_L * WIDE_MAX // den
    return sorted({1, 2, 3, 7, kb, kb + 1, (kb + kw) // 2, kw})


def _gate_params():
    p = {}
    for t in GATE_THRESHOLDS:
        for s, v in enumerate(_slots(t)):
            p["E%r_slot%d" % (t, s)] = dict(LAX, max_read_error_rate=v)
    p["lax"] = LAX
    p["E0.1_all"] = dict(LAX, max_read_error_rate=(0.1, 0.1, 0.1))
    for s, v in enumerate(_slots(1.0, others=0.1)):
        p["E0.1_all_but%d" % s] = dict(LAX, max_read_error_rate=v)
    return p


def _pair_rows(E, D):
    cap = 255 if D <= GATE_L * 255 else WIDE_MAX
    d = level(D, GATE_L, cap)
    return d, spread(E, d)


def _gate32(kind):
    b = _Builder("gate32" if kind == 0 else "gate32_mol", kind)
    L = GATE_L
    zero, one = Strand(1, 0), Strand(3, 3)  # rates 0 and 1
    for (num, den), ties in GATE_PAIRS.items():
        for k in gate_ks(den):
            for delta in (-1, 0, 1):
                E, D = k * num + delta, k * den
                d, er = _pair_rows(E, D)
                m = dict(pair=(num, den), k=k, delta=delta)
                pair = Strand(d, er)
                if kind == 1:
                    b.add(end(L, pair), slots=(0,), shape="mol", **m)
                    continue
                b.add(end(L, pair, zero), slots=(2,), shape="a_max", **m)       # max(aE, bE) = aE
                b.add(end(L, zero, pair), slots=(2,), shape="b_max", **m)
                b.add(end(L, pair, one), slots=(1,), shape="a_min", **m)        # min(aE, bE) = aE
                b.add(end(L, one, pair), slots=(1,), shape="b_min", **m)
                ad = (d + 1) // 2                                               # cE alone: the pair split over both
                ae = np.minimum(er, ad)
                b.add(end(L, Strand(ad, ae), Strand(d - ad, er - ae)), slots=(0,), shape="c", **m)
                if er[0] >= 1 and d[0] >= 2:
                    # column 0: the BA strand's one read calls another base at the lower quality, so it
                    # counts as one error whatever its own error byte says
                    a1, bb = ad.copy(), np.full(L, A)
                    a1[0], bb[0] = d[0] - 1, G | 0xB0
                    a2 = np.minimum(er, a1)
                    be = er - a2
                    a2[0], be[0] = er[0] - 1, 0
                    b.add(end(L, Strand(a1, a2), Strand(d - a1, be, base=bb, qual=39)), slots=(0,), shape="c_disagree", **m)
                if k == 1:  # the nan0 / fminf / fmaxf path
                    nodepth = Strand(0, 0)
                    b.add(end(L, pair, None), slots=(0, 2), shape="ab_only", note="ab_only", **m)
                    b.add(end(L, None, pair), slots=(0, 2), shape="ba_only", note="ba_only", **m)
                    b.add(end(L, nodepth, pair), slots=(0, 2), shape="a_nodepth", note="a_nodepth", **m)  # aE NaN, bE finite
                    b.add(end(L, pair, nodepth), slots=(0, 2), shape="b_nodepth", note="b_nodepth", **m)
    if kind == 0:
        # no error in either strand, two columns where they disagree: cE = 10 / 80 with aE = bE = 0
        bb = np.asarray([A, A, T | 0x40, A, A, N, A, A])
        b.add(end(L, Strand(5, 0), Strand(5, 0, base=bb, qual=39)), slots=(), shape="c_only", note="c_only")
        b.add(end(L, Strand(0, 0), Strand(0, 0)), slots=(), shape="no_depth", note="no_depth")
        b.add(end(L, Strand(0, 3), Strand(0, 0)), slots=(), shape="err_no_depth", note="err_no_depth")  # 24 / 0 = inf
    else:
        b.add(end(L, Strand(0, 0)), slots=(), shape="no_depth", note="no_depth")
    return b


# ---- base64: per-base fp64 ties --------------------------------------------------------------------

# (the last: the double below 0.1, which float32 cannot tell from 0.1 -- 4 / 40 exceeds it)
BASE_THRESHOLDS = (0.0, 0.1, 0.025, 1 / 3, 0.5, 1.0, float(np.nextafter(0.1, 0.0)))
BASE_GRID = [(e, d) for d in range(41) for e in range(d + 2)]
# application -> the slots in which the column's verdict is e / d > T
BASE_APPS = {"a": (2,), "b": (2,), "a_min": (1,), "b_min": (1,), "c": (0,), "a_zero": (0, 2), "b_zero": (0, 2), "both": (0, 1, 2)}


def _base_strands(app, e, d):
    """the (a, b) columns (depth, err) each of the application `app` for the grid's (e, d)"""
    if app in ("a", "b"):        # the other strand errs nowhere: max = this one's rate, the combined rate lower
        x, y = (d, e), (50, 0)
    elif app in ("a_min", "b_min"):  # the other strand at 59 / 60: min = this one's rate up to there
        x, y = (d, e), (60, 59)
    elif app in ("a_zero", "b_zero"):  # the other strand has no read in the column: its rate is 0
        x, y = (d, e), (0, 0)
    elif app == "both":
        x, y = (d, e), (d, e)
    else:                        # "c": (e, d) split over the strands
        ad = (d + 1) // 2
        ae = min(e, ad)
        x, y = (ad, ae), (d - ad, e - ae)
    return (y, x) if app.startswith("b_") or app == "b" else (x, y)


def _base64(kind):
    b = _Builder("base64" if kind == 0 else "base64_mol", kind)
    S = b.stride
    for app in (BASE_APPS if kind == 0 else ("mol",)):
        for i in range(0, len(BASE_GRID), 2 * S):
            ends, cols = [], []
            for part in (BASE_GRID[i:i + S], BASE_GRID[i + S:i + 2 * S]):
                if kind == 1:
                    a, bb = ([(d, e) for e, d in part], None)
                else:
                    ab = [_base_strands(app, e, d) for e, d in part]
                    a, bb = [x for x, _ in ab], [y for _, y in ab]
                mk = lambda v: Strand(np.asarray([x[0] for x in v], np.int64), np.asarray([x[1] for x in v], np.int64))  # noqa: E731
                ends.append(end(len(part), mk(a), mk(bb) if bb is not None else None, seq=C))
                cols.append(part)
            b.add(ends[0], ends[1], app=app, slots=BASE_APPS.get(app, (0,)), cols=cols, note=app)
    p = {}
    for t in BASE_THRESHOLDS:
        for s, v in enumerate(_slots(t)):
            p["B%r_slot%d" % (t, s)] = dict(LAX, max_base_error_rate=v)
    return b, p


# ---- reads: depth thresholds -----------------------------------------------------------------------

READS_MIN = {"M3_2_1": (3, 2, 1), "M2_1_0": (2, 1, 0), "M1": (1,), "M0": (0,), "M65535": (65535, 32767, 32767),
             "M65534": (65534, 32767, 32767), "M256_255_1": (256, 255, 1)}


def _reads(kind, with_wide):
    b = _Builder("reads", kind)
    L = 8
    grid = [(x, y) for x in range(5) for y in range(5)]
    if kind == 1:
        for x in range(5):
            b.add(end(L, Strand(x)), depth=(x,), note="per_read")
        b.add(end(6, Strand(np.asarray([4, 0, 1, 2, 3, 4]))), note="per_base")
    else:
        for x, y in grid:  # per read: every (aD, bD) of 0..4
            b.add(end(L, Strand(x), Strand(y)), depth=(x, y), note="per_read")
            if (x == 0) != (y == 0):  # and the same with that strand absent
                b.add(end(L, Strand(x) if x else None, Strand(y) if y else None), depth=(x, y), note="per_read_one_strand")
        for part in (grid[0::2], grid[1::2]):  # per base: column 0 lets the read pass every gate below 4
            ad, bd = np.asarray([4] + [x for x, _ in part]), np.asarray([4] + [y for _, y in part])
            b.add(end(len(ad), Strand(ad), Strand(bd)), note="per_base")
        for x, y in ((255, 1), (254, 1), (255, 0), (254, 2)):  # byte rows at 255
            b.add(end(L, Strand(x), Strand(y)), depth=(x, y), note="byte255")
    if with_wide and kind == 0:
        for x, y in ((256, 1), (255, 1), (256, 0), (254, 1), (257, 0)):  # wide rows at 256 beside them
            b.add(end(L, Strand(x), Strand(y)), depth=(x, y), wide=True, note="wide256")
        for x, y in ((32767, 32767), (32767, 32766), (32766, 32767)):  # duplex depth 65534
            b.add(end(L, Strand(x), Strand(y)), depth=(x, y), note="wide_max")
        ad = np.asarray([32767, 32767, 32766, 32767, 0, 32767, 1, 32767])
        bd = np.asarray([32767, 32766, 32767, 0, 32767, 1, 32767, 32767])
        b.add(end(L, Strand(ad), Strand(bd)), note="wide_max_per_base")
    p = {k: dict(LAX, min_reads=v) for k, v in READS_MIN.items()}
    if kind == 1:
        p = {k: v for k, v in p.items() if k in ("M1", "M0", "M3_2_1")}
    return b, p


# ---- after: the two checks after masking -----------------------------------------------------------

NOCALL_AT = {0.25: (8, 2), 0.2: (10, 2), 0.0: (8, 0), 1.0: (8, 8)}  # fraction -> (L, N columns) exactly at it


def _after(kind):
    b = _Builder("after" if kind == 0 else "after_mol", kind)
    ok = Strand(5, 0)
    two = lambda L, **kw: end(L, ok, ok if kind == 0 else None, **kw)  # noqa: E731
    for frac, (L, n0) in NOCALL_AT.items():
        for n in (n0 - 1, n0, n0 + 1):
            if not 0 <= n <= L:
                continue
            for old in sorted({0, n // 2, n}):  # N columns there before / masked now (quality 5 < 10)
                seq, q = np.full(L, G), np.full(L, 40)
                cols = np.arange(n) * (L // max(n, 1)) if n < L else np.arange(L)
                seq[cols[:old]] = N
                q[cols[:old]] = 33  # (a no-call whose quality is not 2)
                q[cols[old:n]] = 5
                b.add(two(L, seq=seq, qual=q), nocall=(frac, n - n0), n=n, old=old, note="nocall")
    for mq in (30, 93):
        L = 8
        for delta in (0, -1):
            q = np.full(L, mq)
            q[3] += delta
            b.add(two(L, qual=q), meanq=(mq, delta), note="meanq")
            # the same sum with a no-call at quality 60 in it, paid for by its neighbours
            seq = np.full(L, T)
            seq[5] = N
            q = np.full(L, mq)
            q[5], q[0], q[1] = min(mq + 30, 255), q[0] - (min(mq + 30, 255) - mq) // 2, q[1] - (min(mq + 30, 255) - mq + 1) // 2
            q[3] += delta
            b.add(two(L, seq=seq, qual=q), meanq=(mq, delta), note="meanq_old_n")
    b.add(two(8, qual=np.asarray([0, 2, 93, 94, 255, 1, 3, 92])), note="qual_bytes")
    b.add(two(8, seq=np.asarray([A, N, C, N, G, N, T, N]), qual=np.asarray([0, 0, 93, 94, 255, 255, 3, 2])), note="qual_bytes_n")
    b.add(two(0), two(8), note="len0_end0")
    b.add(two(8), two(0), note="len0_end1")
    b.add(two(0), note="len0_both")
    bad = Strand(5, 5)
    b.add(end(8, bad, bad if kind == 0 else None), note="readerr")
    p = {}
    for frac in NOCALL_AT:
        p["n%r" % frac] = dict(LAX, min_base_quality=10, max_no_call_fraction=frac)
    for mq in (30, 93):
        p["q%d" % mq] = dict(LAX, min_mean_base_quality=mq)
    for nq in (0, 2, 93):
        p["N%d" % nq] = dict(LAX, min_base_quality=nq)
    p["N93_n0.25_q30"] = dict(LAX, min_base_quality=93, max_no_call_fraction=0.25, min_mean_base_quality=30)
    p["E0.5"] = dict(LAX, max_read_error_rate=(0.5,))
    p["M1"] = dict(LAX, min_reads=(1,))
    return b, p


# ---- lanes: column position ------------------------------------------------------------------------

LANE_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025)


def _random_end(rng, L, kind, strands=3):
    """a messy read of L columns: depths 0..6, errors mostly at most the depth, strands that mostly
    agree, high nibbles set in the rows' bases, every quality byte; strands: 1 AB, 2 BA, 3 both"""
    def row():
        d = rng.integers(0, 7, L)
        e = np.where(rng.random(L) < 0.9, (d * rng.random(L) * 0.5).astype(np.int64), rng.integers(0, 256, L))
        return d, e
    base = np.asarray([A, C, G, T])[rng.integers(0, 4, L)]
    other = np.where(rng.random(L) < 0.85, base, np.asarray([A, C, G, T, N])[rng.integers(0, 5, L)])
    hi = lambda: rng.integers(0, 16, L) << 4  # noqa: E731
    qa, qb = rng.integers(0, 256, L), rng.integers(0, 256, L)
    qb = np.where(rng.random(L) < 0.3, qa, qb)
    a = Strand(*row(), base=base | hi(), qual=qa) if strands & 1 else None
    b = Strand(*row(), base=other | hi(), qual=qb) if strands & 2 and kind == 0 else None
    if kind == 1 and a is None:
        a = Strand(*row(), base=base | hi(), qual=qa)
    seq = np.where(rng.random(L) < 0.1, N, base)
    q = np.where(rng.random(L) < 0.8, rng.integers(20, 61, L), rng.integers(0, 256, L))
    return End(seq, q, a, b)


LANE_PARAMS = {"q10": dict(LAX, min_reads=(1, 1, 0), min_base_quality=10),
               "q10_agree": dict(LAX, min_reads=(1, 1, 0), min_base_quality=10, require_single_strand_agreement=True),
               "typical": PARAM_SETS["typical"], "single_ok": PARAM_SETS["single_ok"],
               "fgbio_defaults": PARAM_SETS["fgbio_defaults"]}


def _lanes(stride, kind=0):
    b = _Builder("lanes%d" % stride, kind, stride)
    rng = np.random.default_rng([stride, 77])
    for L in sorted({x for x in LANE_LENGTHS + (stride - 1, stride) if x <= stride}):
        for strands in (3, 3, 1, 2):
            b.add(_random_end(rng, L, kind, strands), _random_end(rng, L, kind, strands), note="L%d" % L)
    ok = Strand(5, 0, base=C, qual=40)
    cols = range(16) if stride == 16 else sorted({c for c in (0, 15, 16, 31, 511, 512, 1023, 1024, stride - 1) if c < stride})
    for c in cols:  # exactly one column masked: its quality is low
        q = np.full(stride, 40)
        q[c] = 5
        b.add(end(stride, ok, ok, seq=C, qual=q), one_hot=c, note="one_hot")
    c = min(stride - 1, 523) - 2
    bb = np.full(stride, C) | (np.arange(stride) % 15 + 1 << 4)  # high nibbles set: no disagreement by themselves
    bb2 = bb.copy()
    bb2[c] = G | 0x70
    b.add(end(stride, Strand(5, 0, bb, 40), Strand(5, 0, bb2, 40), seq=C), disagree=c, note="disagree")
    q = np.full(stride, 40)
    q[stride // 2] = 5
    fail, good = end(stride, Strand(0), Strand(0), seq=G, qual=q), end(stride, ok, ok, seq=G, qual=q)
    b.add(fail, good, note="end0_fails")  # end 0: no depth, dropped by min_reads and left untouched
    b.add(good, fail, note="end1_fails")
    return b, LANE_PARAMS


# ---- long: sums past 2^31 --------------------------------------------------------------------------

LONG_STRIDE, LONG_L = 65520, 65519


def _long():
    b = _Builder("long", 0, LONG_STRIDE)
    L = LONG_L
    # duplex: 32767 on both strands in every column but the first, so that the depth sum is a
    # multiple of 10; errors 7/10 of it: both sums past 2^31, below 2^32
    D = L * 2 * WIDE_MAX
    D -= D % 10
    cd = np.full(L, 2 * WIDE_MAX, np.int64)
    cd[0] -= L * 2 * WIDE_MAX - D
    ad = np.minimum(cd, WIDE_MAX)
    ce = spread(D // 10 * 7, cd)
    ae = np.minimum(ce, ad)
    q = np.full(L, 40)
    q[[0, 7, 511, 512, 65518]] = 5
    b.add(end(L, Strand(ad, ae), Strand(cd - ad, ce - ae), qual=q), note="duplex", sums=(D // 10 * 7, D))
    Da = L * WIDE_MAX - (L * WIDE_MAX) % 10
    d1 = np.full(L, WIDE_MAX, np.int64)
    d1[0] -= L * WIDE_MAX - Da
    b.add(end(L, Strand(d1, spread(Da // 10 * 7, d1)), None, qual=q), note="ab_only", sums=(Da // 10 * 7, Da))
    # the thresholds: 0.7, and the float32 quotient of the duplex family itself and its neighbour below
    r = float(np.float32(D // 10 * 7) / np.float32(D))
    p = {"E0.7": dict(LAX, min_base_quality=10, max_read_error_rate=(0.7,)),
         "E_at": dict(LAX, min_base_quality=10, max_read_error_rate=(r, 1.0, 1.0)),
         "E_below": dict(LAX, min_base_quality=10, max_read_error_rate=(float(np.nextafter(np.float32(r), np.float32(0))), 1.0, 1.0))}
    return b, p


# ---- counts: family counts around the four-families-per-workgroup cut ------------------------------

COUNTS = {0: "", 1: "1", 3: "101", 4: "0111", 5: "11110", 9: "010110110"}


def _counts(n):
    b = _Builder("counts%d" % n, 0)
    rng = np.random.default_rng([n, 99])
    for ch in COUNTS[n]:
        if ch == "1":
            L = int(rng.integers(1, 17))
            b.add(_random_end(rng, L, 0), _random_end(rng, L, 0))
        else:
            b.skip()
    return b, {k: LANE_PARAMS[k] for k in ("q10", "typical")}


SETS = ("gate32", "gate32_mol", "base64", "base64_mol", "reads", "reads_mol", "reads_nowide", "reads_minus1", "after",
        "after_mol", "lanes16", "lanes32", "lanes1040", "long") + tuple("counts%d" % n for n in COUNTS)


@functools.lru_cache(maxsize=None)
def make(name: str, garbage: int = 0) -> FilterRows:
    wide_table = "auto"
    if name.startswith("gate32"):
        b, p = _gate32(int(name.endswith("_mol"))), _gate_params()
    elif name.startswith("base64"):
        b, p = _base64(int(name.endswith("_mol")))
    elif name.startswith("reads"):
        b, p = _reads(int(name == "reads_mol"), with_wide=name == "reads")
        wide_table = {"reads_nowide": "none", "reads_minus1": "minus1"}.get(name, "auto")
    elif name.startswith("after"):
        b, p = _after(int(name.endswith("_mol")))
    elif name.startswith("lanes"):
        b, p = _lanes(int(name[5:]))
    elif name == "long":
        b, p = _long()
    elif name.startswith("counts"):
        b, p = _counts(int(name[6:]))
    else:
        raise KeyError(name)
    x = b.build(p, garbage, wide_table)
    x.name = name
    return x


@functools.lru_cache(maxsize=None)
def reference(name: str, pn: str, garbage: int = 0):
    """filter_ref.apply on the set under its parameter set pn -> (filt, masked, seq unpacked, qual)"""
    x = make(name, garbage)
    return x.apply(x.params[pn])

"""Fabricated inputs for the metrics kernel (csrc/bsdc_metrics.hip), in the
style of filter_rows.py: the arrays bsdc_metrics reads -- status, len, packed seq, qual, ss_len, the
four single-strand rows, ss_wide with its wide rows -- built with no vote, so that the reduction's
edges are met on purpose.  A plain helper module: test_metrics_host.py runs the sets through the
host twin, test_gpu_metrics.py through the kernel, both against metrics_ref.

Every byte past a read's length, every row of a family that is not emitted and the byte rows of a
family that has a wide row are random.  Each set is built once per process (make) and must not be
modified; so is each reference (reference)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import metrics_ref as MR

A, C, G, T, N = 1, 2, 4, 8, 15
LENGTHS = (1, 15, 16, 17, 511, 512, 513)


@dataclass
class Rows:
    name: str
    kind: int            # 0 duplex, 1 molecular
    stride: int
    cycles: int
    status: np.ndarray   # u8 [F]
    length: np.ndarray   # i32 [F, 2]
    seq: np.ndarray      # u8 [F, 2, stride / 2] packed nt16, high nibble first
    qual: np.ndarray     # u8 [F, 2, stride]
    ss_len: np.ndarray   # i32 [F, 4]
    ss_base: np.ndarray  # u8 [F, 4, stride]
    ss_qual: np.ndarray
    ss_depth: np.ndarray
    ss_err: np.ndarray
    ss_wide: np.ndarray  # i32 [F] or None
    ss_wdepth: np.ndarray  # u16 [W, 4, stride]
    ss_werr: np.ndarray
    bad: tuple = ()      # families the kernel must skip and count
    notes: dict = field(default_factory=dict)

    @property
    def n_fam(self) -> int:
        return int(self.status.shape[0])

    def ss(self):
        return {"len": self.ss_len, "base": self.ss_base, "qual": self.ss_qual, "depth": self.ss_depth, "err": self.ss_err,
                "wide": self.ss_wide, "wdepth": self.ss_wdepth, "werr": self.ss_werr}


def unpack(seq: np.ndarray) -> np.ndarray:
    return np.stack([seq >> 4, seq & 15], axis=-1).reshape(seq.shape[:-1] + (2 * seq.shape[-1],))


def pack(codes: np.ndarray) -> np.ndarray:
    return ((codes[..., 0::2] << 4) | (codes[..., 1::2] & 15)).astype(np.uint8)


class _Builder:
    """Families are added as dicts: emitted, wide (bool), and per end e a dict with L, seq, qual and
    the strand rows "a" / "b" (None: absent), each (depth, err, base, qual) of scalars or arrays."""

    def __init__(self, name, kind, stride, cycles, seed):
        self.name, self.kind, self.stride, self.cycles = name, kind, stride, cycles
        self.g = np.random.default_rng([seed, 0x3E7])
        self.fams, self.notes = [], {}

    def add(self, e0=None, e1=None, emitted=True, wide=False, note=None):
        self.fams.append((e0, e0 if e1 is None else e1, emitted, wide))
        if note:
            self.notes.setdefault(note, []).append(len(self.fams) - 1)
        return len(self.fams) - 1

    def build(self, wide_table=True) -> Rows:
        g, F, S = self.g, len(self.fams), self.stride
        rnd = lambda shape, hi=256, dt=np.uint8: g.integers(0, hi, shape).astype(dt)  # noqa: E731
        status = rnd(F) & 0xFE
        length = g.integers(0, S + 1, (F, 2)).astype(np.int32)
        codes, qual = rnd((F, 2, S), 16), rnd((F, 2, S))
        ss_len = g.integers(0, S + 1, (F, 4)).astype(np.int32)
        ss_base, ss_qual, ss_depth, ss_err = rnd((F, 4, S), 16), rnd((F, 4, S)), rnd((F, 4, S)), rnd((F, 4, S))
        wide = np.full(F, -1, np.int32)
        wd, we = [], []
        bc = lambda v, L: np.broadcast_to(np.asarray(v, np.int64), (L,))  # noqa: E731
        for f, (e0, e1, emitted, is_wide) in enumerate(self.fams):
            if not emitted:
                continue
            status[f] |= 1
            if is_wide:
                wide[f] = len(wd)
                wd.append(rnd((4, S), 32768, np.uint16))
                we.append(rnd((4, S), 32768, np.uint16))
            for e, end in enumerate((e0, e1)):
                L = int(end["L"])
                length[f, e] = L
                codes[f, e, :L], qual[f, e, :L] = bc(end["seq"], L), bc(end["qual"], L)
                for s, row in ((e, end.get("a")), (3 - e, end.get("b"))):
                    if self.kind == 1 and s != e:
                        continue
                    if row is None:
                        ss_len[f, s] = 0
                        continue
                    d, er, b, q = (bc(x, L) for x in row)
                    assert (er <= d).all() and d.max(initial=0) <= (32767 if is_wide else 255)
                    ss_len[f, s] = max(L, 1)
                    ss_base[f, s, :L], ss_qual[f, s, :L] = b, q
                    if is_wide:
                        wd[-1][s, :L], we[-1][s, :L] = d, er
                    else:
                        ss_depth[f, s, :L], ss_err[f, s, :L] = d, er
        if wide_table:
            W = len(wd)
            wdepth = np.stack(wd) if W else np.zeros((0, 4, S), np.uint16)
            werr = np.stack(we) if W else np.zeros((0, 4, S), np.uint16)
        else:
            assert not wd
            wide, wdepth, werr = None, np.zeros((0, 4, S), np.uint16), np.zeros((0, 4, S), np.uint16)
        return Rows(self.name, self.kind, S, self.cycles, status, length, pack(codes), qual, ss_len, ss_base, ss_qual,
                    ss_depth, ss_err, wide, wdepth, werr, notes=self.notes)


def _strand(g, L, wide):
    hi = 32768 if wide and g.random() < 0.5 else 256
    d = g.integers(0, hi, L)
    if g.random() < 0.1:
        d[:] = 0
    e = (d * g.random(L) * (0.2 if g.random() < 0.7 else 1.0)).astype(np.int64)
    b = g.choice([A, C, G, T, N, 0, 3], L, p=[0.22, 0.22, 0.22, 0.22, 0.1, 0.01, 0.01])
    return d, e, b, g.integers(0, 256, L)


def _random_end(g, L, kind, wide):
    seq = g.choice([A, C, G, T, N], L, p=[0.23, 0.23, 0.23, 0.23, 0.08])
    end = {"L": L, "seq": seq, "qual": g.integers(0, 94, L)}
    present = (True, False) if kind == 1 else ((True, True), (True, True), (True, False), (False, True),
                                               (False, False))[int(g.integers(0, 5))]
    if present[0]:
        end["a"] = _strand(g, L, wide)
    if present[1]:
        end["b"] = _strand(g, L, wide)
        if present[0] and g.random() < 0.5:  # mostly agreeing strands
            end["b"] = (end["b"][0], end["b"][1], np.where(g.random(L) < 0.9, end["a"][2], end["b"][2]), end["b"][3])
    return end


def _random(name, kind, stride, cycles, F, seed):
    b = _Builder(name, kind, stride, cycles, seed)
    g = np.random.default_rng([seed, 7])
    Ls = [x for x in LENGTHS if x <= stride]
    for f in range(F):
        if f % 4 == 1 and F > 1:  # unemitted families between emitted ones
            b.add(emitted=False, note="not_emitted")
            continue
        wide = bool(g.random() < 0.15)
        ends = [_random_end(g, int(g.choice(Ls)) if g.random() < 0.8 else int(g.integers(0, stride + 1)), kind, wide)
                for _ in range(2)]
        b.add(ends[0], ends[1], wide=wide)
    return b.build()


def _edges(name, kind, stride=32, cycles=512):
    """The named edges, one family each (both ends alike unless said)."""
    b = _Builder(name, kind, stride, cycles, 5)
    L = 20
    ok = (4, 0, A, 40)
    end = lambda **kw: dict({"L": L, "seq": A, "qual": 40, "a": ok, "b": ok}, **kw)  # noqa: E731
    b.add(end(a=(0, 0, A, 40), b=None), note="no_depth")                       # NaN: cE, aE in bin 101
    b.add(end(a=(0, 0, A, 40), b=(200, 3, A, 40)), note="zero_next_to_deep")   # aE NaN, bE a number
    b.add(end(a=(3, 1, A, 40), b=None), note="one_strand")
    b.add(end(a=None, b=(3, 1, A, 40)), note="ba_only")
    b.add(end(a=None, b=None), note="no_strand")
    # rates on bin edges: 1/1000 and 100/1000 as float32, 1/40 (float32 rounds it up past 0.025)
    b.add(end(L=10, a=(100, np.r_[1, np.zeros(9, np.int64)], A, 40), b=None), note="rate_1_1000")
    b.add(end(L=10, a=(100, 10, A, 40), b=None), note="rate_100_1000")
    b.add(end(L=10, a=(4, np.r_[1, np.zeros(9, np.int64)], A, 40), b=None), note="rate_1_40")
    b.add(end(L=10, a=(100, 99, A, 40), b=(1, 1, A, 40)), note="rate_high")
    # depths 255, 256, 32767 through wide rows, next to byte rows saturated at 255
    for d in (255, 256, 32767):
        b.add(end(a=(d, 1, A, 40), b=(d, 0, A, 40)), wide=True, note="wide_%d" % d)
    b.add(end(a=(255, 1, A, 40), b=(255, 0, A, 40)), note="byte_255")
    # N against a base, N against N, two bases that differ, a non-ACGT code against a base
    codes = np.full(L, A, np.int64)
    b.add(end(a=(2, 0, np.r_[N, N, C, 3, codes[4:]], 40), b=(2, 0, np.r_[A, N, G, A, codes[4:]], 30),
              seq=np.r_[N, N, C, A, codes[4:]]), note="n_columns")
    # every quality 0..93 (and bytes past it, capped at 93)
    b.add({"L": 32, "seq": A, "qual": np.arange(32), "a": ok, "b": ok},
          {"L": 32, "seq": A, "qual": np.arange(32, 64), "a": ok, "b": ok}, note="quals")
    b.add({"L": 32, "seq": A, "qual": np.r_[np.arange(64, 94), 200, 255], "a": ok, "b": ok}, note="quals")
    b.add(end(L=0), note="empty")
    return b.build()


def _bad(name, kind):
    """Families that must be skipped and counted: a length beyond the stride, a wide row outside the
    table -- between good ones.  (The arrays stay their exact sizes: a kernel that read a bad family
    would read outside them.)"""
    b = _Builder(name, kind, 16, 512, 9)
    ok = (4, 1, A, 40)
    end = {"L": 16, "seq": A, "qual": 30, "a": ok, "b": ok}
    for f in range(9):
        b.add(end, wide=f in (2, 5))
    x = b.build()
    x.length[1, 0] = 17          # L > stride
    x.length[4, 1] = 65535
    x.ss_wide[5] = 2             # the table has rows 0 and 1
    x.ss_wide[7] = 1 << 30
    x.ss_wide[8] = -7            # (any negative entry: no wide row)
    x.bad = (1, 4, 5, 7)
    return x


# name -> (stride, cycles, families); every one as duplex ("" suffix) and molecular ("_mol")
RANDOM = {"s16_f1": (16, 512, 1), "s16_f3": (16, 512, 3), "s16_f65": (16, 512, 65), "s16_f300": (16, 512, 300),
          "s32_f300": (32, 512, 300), "s32_c2_f65": (32, 2, 65), "s16_c2_f1": (16, 2, 1), "s528_f3": (528, 512, 3),
          "s528_f65": (528, 512, 65), "s528_c2_f3": (528, 2, 3),
          "s16_f3100": (16, 512, 3100)}  # more families than one pass of the grid holds: workgroups stride
NAMES = tuple(n + sfx for n in list(RANDOM) + ["edges", "edges_c2", "bad"] for sfx in ("", "_mol"))


@functools.lru_cache(maxsize=None)
def make(name: str) -> Rows:
    kind = 1 if name.endswith("_mol") else 0
    base = name[:-4] if kind else name
    if base == "edges":
        return _edges(name, kind)
    if base == "edges_c2":
        return _edges(name, kind, cycles=2)
    if base == "bad":
        return _bad(name, kind)
    stride, cycles, F = RANDOM[base]
    return _random(name, kind, stride, cycles, F, seed=sorted(RANDOM).index(base) + 100 * kind)


@functools.lru_cache(maxsize=None)
def reference(name: str) -> np.ndarray:
    """metrics_ref over the set -> the accumulator's words (read only)."""
    x = make(name)
    w = MR.words(MR.run(x.ss(), unpack(x.seq), x.qual, x.length, x.status, molecular=bool(x.kind), cycles=x.cycles,
                        bad=x.bad))
    w.setflags(write=False)
    return w


def from_oracle(r, molecular: bool, cycles: int = 512) -> Rows:
    """An oracle consensus (oracle.run's result) as the device's arrays: stride padded to a multiple
    of 16, byte rows saturated at 255, and the exact depths / errors of the families that pass a
    byte in wide rows."""
    F, S0 = int(r.status.shape[0]), int(r.cons_seq.shape[2])
    S = max(16, (S0 + 15) // 16 * 16)
    pad = lambda a: np.pad(np.asarray(a), [(0, 0)] * (a.ndim - 1) + [(0, S - a.shape[-1])])  # noqa: E731
    d, e = pad(r.ss["depth"]).astype(np.int64), pad(r.ss["err"]).astype(np.int64)
    need = np.nonzero((d > 255).any(axis=(1, 2)))[0]
    wide = np.full(F, -1, np.int32)
    wide[need] = np.arange(need.shape[0])
    return Rows("oracle", int(molecular), S, cycles, np.asarray(r.status, np.uint8), np.asarray(r.cons_len, np.int32),
                pack(pad(r.cons_seq)), pad(r.cons_qual).astype(np.uint8), np.asarray(r.ss["len"], np.int32),
                pad(r.ss["base"]).astype(np.uint8), pad(r.ss["qual"]).astype(np.uint8),
                np.minimum(d, 255).astype(np.uint8), np.minimum(e, 255).astype(np.uint8), wide,
                np.minimum(d[need], 32767).astype(np.uint16), np.minimum(e[need], 32767).astype(np.uint16))

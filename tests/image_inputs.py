"""Inputs of the family-image gather's tests (bsdc_image_gather / its host twin, csrc/bsdc_image.hip;
tests/test_image_host.py, tests/test_gpu_image.py): record streams planned and materialized twice,
with host images (the reference: hostplan.materialize + split_hbm_bucket) and without them (the
gather's table), the records' SEQ / QUAL bytes packed as a BAM packs them.

Plan cases (CASES): kept lengths 1, 2, 7, 8, 9, 15, 16, 17 and max_len + 2 at 32 and 33; leading
soft clips 0..3 with trailing ones, hard clips dropped; odd and even l_seq; quality bytes 0, 93,
127, 128, 255; families of 1 and of 520 records; a batch split_hbm_bucket cuts (one family left
whole); step-1 ('vote', mi-group) and step-5 ('full') plans.  `lead` / `gap` put the SEQ fields at
every src % 4.  table_case(): a hand-made table beside a plain numpy statement of the images, for
what no plan produces: a kept length of 0, a first slot past 0 (leading empty families), a skip of
either parity against an odd and an even l_seq, two records sharing a dword of the packed image.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

import align_inputs as AL
import edge_inputs as E
from bsseqconsensusreads_amd import _lib, batch as B, hostplan, pipeline, records as R, synth

QUAL_EDGES = np.array([0, 93, 127, 128, 255], np.uint8)


def q_edges(rng, lens):
    return [QUAL_EDGES[rng.integers(0, 5, size=int(n))] for n in lens]


@dataclass
class Case:
    name: str
    raw: R.RawRecords
    ref: Optional[R.Reference]
    mode: str = "full"
    order: str = "template-coordinate"
    molecular: bool = False
    part_cap: Optional[int] = None  # split_hbm_bucket over every large bucket with parts this large
    lead: int = 0
    gap: int = 0


def _clips_case() -> AL.Case:
    """Leading soft clips 0..3 with trailing ones, hard clips (which hold no bases), reads of 29..31
    bases: odd and even l_seq."""
    shapes = ("30M", "1S29M", "2S27M1S", "3S25M2S", "29M2S", "1S28M", "3H2S27M1S", "28M3S2H", "31M", "2S29M")
    fams = []
    for k, c in enumerate(shapes):
        s = AL._start(k)
        fams.append(AL.Fam(c, AL.pair("a", "A", True, (s, c), (s + 12, c)) + AL.pair("b", "B", False, (s, c), (s + 12, c))))
    return AL.build("clips", fams, True, 31)


def _lengths() -> E.EdgeSet:
    fams = E.random_families(60, (1, 4), (1, 2, 7, 8, 9, 15, 16, 17), 41, frag_extra=(0, 6), contig_len=3000)
    return E.build(fams, q_edges, seed=1041, contig_len=3000)


def _sizes() -> E.EdgeSet:
    return E.size_case(False, seed=45, L=30, reps=1, sizes=(1, 2, 3), deep=E.DEEP_FAMILY)


def _cases():
    out = []
    es = _lengths()
    out.append(Case("lengths", es.raw, es.ref, lead=0, gap=0))
    out.append(Case("lengths_vote", es.raw, None, mode="vote", order="mi-group", molecular=True, lead=1, gap=1))
    for st, lead in ((32, 2), (33, 3)):
        es = E.stride_case(st)
        out.append(Case("stride%d" % st, es.raw, es.ref, lead=lead, gap=st & 1))
    c = _clips_case()
    out.append(Case("clips", c.raw, c.ref, lead=1, gap=2))
    out.append(Case("clips_vote", c.raw, None, mode="vote", lead=3, gap=0))
    es = E.quality_case("wild", n_fam=40)
    out.append(Case("wild", es.raw, es.ref, lead=2, gap=3))
    es = _sizes()
    out.append(Case("sizes", es.raw, es.ref, lead=1, gap=0))
    s = synth.generate("C3", 40, seed=5, device="cpu", genome_len=100_000)
    out.append(Case("split", s.raw, s.ref, part_cap=12_000, lead=1, gap=0))  # every family cut, many parts
    out.append(Case("split_mixed", s.raw, s.ref, part_cap=40_000, lead=0, gap=0))  # some cut, some left whole
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = {c.name: c for c in _cases()}
    return _CASES


CASE_NAMES = ("lengths", "lengths_vote", "stride32", "stride33", "clips", "clips_vote", "wild", "sizes", "split",
              "split_mixed")


def _materialize(plan, gather: bool, part_cap):
    cap = B.route_small_cap(plan, 0, plan.n_fam)
    fb = hostplan.materialize(plan, 0, plan.n_fam, cap, gather=gather)
    if part_cap is None:
        return B.split_hbm_bucket(fb)
    old = B.SPLIT_FROM
    B.SPLIT_FROM = 0  # every large bucket (tests/test_batches.py)
    try:
        return B.split_hbm_bucket(fb, part_cap=part_cap)
    finally:
        B.SPLIT_FROM = old


def _materialize_range(plan, a: int, b: int, gather: bool, part_cap: int):
    """Plan families [a, b) with every family in the HBM bucket, cut where it can be into parts of
    at most part_cap LDS bytes (tests/test_gpu_parity.py force_parts)."""
    fb = hostplan.materialize(plan, a, b, 0, gather=gather)
    nb = len(fb.large_buckets)
    fb.large_buckets = [np.zeros((0, 4), np.uint32)] * (nb - 1) + [fb.large_fams]
    fb.large_arenas = [16] * (nb - 1) + [max(max(fb.large_arenas), B.LARGE_LDS_MAX + 16)]
    return B.split_hbm_bucket(fb, part_cap=part_cap)


_BUILT = {}


def built(name: str):
    """-> (case, records without unpacked bases, batch with host images, batch with the gather's
    table), computed once."""
    if name not in _BUILT:
        c = cases()[name]
        raw = pipeline.molecular_records(c.raw) if c.molecular else c.raw
        packed = R.pack_bases(raw, c.lead, c.gap)
        ph = B.plan_families(raw, c.mode, c.ref, family_order=c.order)
        pg = B.plan_families(packed, c.mode, c.ref, family_order=c.order)
        _BUILT[name] = (c, packed, _materialize(ph, False, c.part_cap), _materialize(pg, True, c.part_cap), ph, pg)
    return _BUILT[name][:4]


def plans(name: str):
    built(name)
    return _BUILT[name][4:]


def padded(raw_bases: np.ndarray) -> np.ndarray:
    """The bytes in a 4-byte aligned array of their exact size."""
    a = np.zeros((raw_bases.shape[0] + 3) // 4, np.uint32).view(np.uint8)[:raw_bases.shape[0]]
    a[:] = raw_bases
    return a


def twin(raw_bases: np.ndarray, table: np.ndarray, n_slots: int):
    """bsdc_image_gather_host -> (rc, seq image, qual image, message); the images start as 0xA5."""
    lib = _lib.load()
    rb = padded(raw_bases)
    t = np.ascontiguousarray(table)
    seq = np.full(n_slots // 2 + 4, 0xA5, np.uint8)
    qual = np.full(n_slots + 4, 0xA5, np.uint8)
    rc = lib.bsdc_image_gather_host(None, rb.ctypes.data, rb.shape[0], t.ctypes.data, t.shape[0], n_slots,
                                    seq.ctypes.data, qual.ctypes.data)
    assert (seq[n_slots // 2:] == 0xA5).all() and (qual[n_slots:] == 0xA5).all()  # nothing past the images
    return rc, seq[:n_slots // 2], qual[:n_slots], lib.bsdc_image_last_error().decode()


# ---- a hand-made table and the plain statement of its images -----------------------------------
def table_case(seed: int = 7):
    """-> (raw bytes, table, n_slots): records of l_seq 0..19, 30, 31, 150 and 151 with every skip
    parity, kept lengths from 0 up, the first slot at 32 (leading empty families), slots back to
    back (round4(len + 2): neighbours share dwords of the packed image) with a family gap now and
    then; the SEQ fields at every src % 4."""
    rng = np.random.default_rng(seed)
    rows, chunks, at, slot = [], [], 0, 32
    for i, l_seq in enumerate(list(range(20)) * 2 + [30, 31, 150, 151] * 3):
        pad = int(rng.integers(0, 4))
        chunks.append(rng.integers(0, 256, size=pad).astype(np.uint8))
        at += pad
        nb = (l_seq + 1) // 2
        chunks.append(rng.integers(0, 256, size=nb).astype(np.uint8))
        chunks.append(QUAL_EDGES[rng.integers(0, 5, size=l_seq)] if i % 3 else rng.integers(0, 256, size=l_seq).astype(np.uint8))
        skip = int(rng.integers(0, min(l_seq, 3) + 1))
        ln = 0 if i % 11 == 0 else int(rng.integers(0, l_seq - skip + 1))
        if i % 5 == 0:
            ln = l_seq - skip
        rows.append((at, l_seq, skip, ln, slot))
        at += nb + l_seq
        slot += (ln + 2 + 3) // 4 * 4
        if i % 7 == 6:
            slot = (slot + 31) // 32 * 32
    table = np.array(rows, np.dtype(_lib.IMAGE_REC))
    n_slots = (slot + 31) // 32 * 32 + 64
    return np.concatenate(chunks), table, n_slots


def images_py(raw_bases: np.ndarray, table: np.ndarray, n_slots: int):
    """The images of a table, base by base (include/bsdc.h bsdc_image_gather's definition)."""
    codes = np.zeros(n_slots, np.uint8)
    qual = np.zeros(n_slots, np.uint8)
    for r in table:
        src, l_seq, skip, ln, slot = (int(r[k]) for k in ("src", "l_seq", "skip", "len", "slot"))
        for j in range(ln):
            b = int(raw_bases[src + (skip + j) // 2])
            codes[slot + 1 + j] = (b & 15) if (skip + j) & 1 else (b >> 4)
            qual[slot + 1 + j] = raw_bases[src + (l_seq + 1) // 2 + skip + j]
    return ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8), qual


def bad_tables(raw_bases: np.ndarray, table: np.ndarray, n_slots: int):
    """(what, table) with one entry out of range each, for every check of the launcher."""
    n_raw = int(raw_bases.shape[0])
    out = []

    def one(what, i, **kw):
        t = table.copy()
        for k, v in kw.items():
            t[k][i] = v
        out.append((what, t))
    last = len(table) - 1
    one("src", 3, src=-1)
    one("src", last, src=n_raw - 1)
    one("src", 0, src=n_raw + 1, l_seq=0, skip=0, len=0)
    one("src", 5, l_seq=-1)
    one("src", 5, l_seq=2 ** 31 - 1)
    one("skip + len", 7, skip=-1)
    one("skip + len", 7, len=-1)
    one("skip + len", 8, len=int(table["l_seq"][8]) - int(table["skip"][8]) + 1)
    one("skip + len", 8, skip=2 ** 31 - 1, len=2 ** 31 - 1)
    one("slot is not a multiple of 4", 2, slot=int(table["slot"][2]) + 2)
    one("slot is not a multiple of 4", 2, slot=int(table["slot"][2]) + 1)
    big = int(np.argmax(table["len"]))
    one("slot + 1 + len", big, slot=n_slots - 4)
    one("slot + 1 + len", big, slot=2 ** 32 - 4)
    return out

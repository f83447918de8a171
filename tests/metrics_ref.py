"""The per-run consensus metrics, restated in numpy as a reference for libbsdc's
bsdc_metrics / bsdc_metrics_host: a plain helper module like filter_ref.py.  It shares no code with
the kernel or with the package's metrics module (only filter_ref's row reader and float32 rate, read
only), reads record by record, and asserts its own invariants before it returns.

Inputs are a consensus as oracle.run gives it (or fabricated rows, unpacked): ``ss`` with "len"
[F, 4], "base" / "qual" / "depth" / "err" [F, 4, stride] (depth / err exact, or bytes with the wide
families' exact rows in "wide" / "wdepth" / "werr"), ``cons_seq`` (nt16 codes, unpacked) /
``cons_qual`` [F, 2, stride], ``cons_len`` [F, 2], ``status`` (bit 0 = emitted); the filter counters
from ``filt`` [F] and ``masked`` [F, 2] (filter_ref.apply's outputs) when given.
"""
from __future__ import annotations

import math

import numpy as np

import filter_ref as FR

N_COUNTS, FAMILIES, EMITTED, RECORDS, SKIPPED, KEPT, MINREADS, READERR, NOCALL, MEANQ, MASKED = 16, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9
ACGT = (1, 2, 4, 8)


def rate_bin(x) -> int:
    """min((int)floor((double)x * 1000.0), 100); NaN -> 101 (an infinite rate lands in 100)"""
    x = float(x)
    if math.isnan(x):
        return 101
    t = x * 1000.0
    return 100 if t >= 100.0 else int(math.floor(t))


def empty(cycles: int) -> dict:
    return {"counts": np.zeros(N_COUNTS, np.uint64), "depth_hist": np.zeros((3, 2, 256), np.uint64),
            "rate_hist": np.zeros((3, 2, 102), np.uint64), "qual_hist": np.zeros((2, 95), np.uint64),
            "by_cycle": np.zeros((2, cycles, 6), np.uint64)}


def words(m: dict) -> np.ndarray:
    """The tables as the accumulator's words, in its fixed order."""
    return np.concatenate([m[k].reshape(-1) for k in ("counts", "depth_hist", "rate_hist", "qual_hist", "by_cycle")])


def record(m: dict, ss, f, e, seq, qual, molecular, cycles):
    """One output record (family f, end e; bases seq, qualities qual, cut to its length) into m."""
    L = int(seq.shape[0])
    if molecular:
        rows = [e]
    else:
        rows = [s for s in (e, 3 - e) if int(ss["len"][f, s]) > 0] or [3 - e]
    ab, aq, ad, ae = FR._row(ss, f, rows[0], L)
    two = len(rows) == 2
    if two:
        bb, bq, bd, be = FR._row(ss, f, rows[1], L)
    else:
        bb, bq, bd, be = ab, aq, np.zeros(L, np.int64), np.zeros(L, np.int64)
    aD, aE = int(ad.max(initial=0)), FR._rate32(ae.sum(), ad.sum())
    bD, bE = (int(bd.max(initial=0)), FR._rate32(be.sum(), bd.sum())) if two else (0, np.float32(0.0))
    if two:
        raw = np.where(ab == bb, ab, np.where(aq > bq, ab, np.where(bq > aq, bb, ab)))
        cerr = np.where(ab == raw, ae, ad) + np.where(bb == raw, be, bd)
        cD, cE = int((ad + bd).max(initial=0)), FR._rate32(cerr.sum(), (ad + bd).sum())
    else:
        cD, cE = aD, aE
    for k, (D, E) in enumerate(((cD, cE), (aD, aE), (bD, bE))):
        m["depth_hist"][k, e, min(D, 255)] += 1
        m["rate_hist"][k, e, rate_bin(E)] += 1
    for c in range(L):
        r = min(c, cycles - 1)
        n = int(seq[c]) == 15
        q = int(qual[c])
        m["qual_hist"][e, 94 if n else min(q, 93)] += 1
        row = m["by_cycle"][e, r]
        row[0] += 1
        row[1] += n
        row[2] += q
        row[3] += int(ad[c] + bd[c])
        row[4] += int(ae[c] + be[c])
        row[5] += bool(two and int(ab[c]) in ACGT and int(bb[c]) in ACGT and int(ab[c]) != int(bb[c]))


def run(ss, cons_seq, cons_qual, cons_len, status, molecular=False, cycles=512, filt=None, masked=None, bad=()) -> dict:
    """-> the tables (empty()'s keys).  bad: families the kernel must skip (counted, never read)."""
    m = empty(cycles)
    F = int(np.asarray(status).shape[0])
    n_rec = [0, 0]
    sum_len = [0, 0]
    for f in range(F):
        m["counts"][FAMILIES] += 1
        if not int(status[f]) & 1:
            continue
        m["counts"][EMITTED] += 1
        if f in bad:
            m["counts"][SKIPPED] += 1
            continue
        m["counts"][RECORDS] += 2
        for e in range(2):
            L = int(cons_len[f, e])
            record(m, ss, f, e, np.asarray(cons_seq[f, e, :L]), np.asarray(cons_qual[f, e, :L]), molecular, cycles)
            n_rec[e] += 1
            sum_len[e] += L
    if filt is not None:
        em = (np.asarray(status) & 1) != 0
        fl = np.asarray(filt)
        m["counts"][KEPT] = int((em & (fl == 0)).sum())
        for k, w in enumerate((MINREADS, READERR, NOCALL, MEANQ)):
            m["counts"][w] = int((em & ((fl >> k) & 1 != 0)).sum())
        m["counts"][MASKED] = int(np.asarray(masked, np.int64)[em].sum())
    # invariants
    for e in range(2):
        for k in range(3):
            assert int(m["depth_hist"][k, e].sum()) == n_rec[e] and int(m["rate_hist"][k, e].sum()) == n_rec[e]
        assert int(m["qual_hist"][e].sum()) == sum_len[e] == int(m["by_cycle"][e, :, 0].sum())
        assert (m["by_cycle"][e, :, 5] <= m["by_cycle"][e, :, 0]).all()
        assert (m["by_cycle"][e, :, 1] <= m["by_cycle"][e, :, 0]).all()
    assert int(m["counts"][RECORDS]) == n_rec[0] + n_rec[1]
    return m

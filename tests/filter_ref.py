"""fgbio FilterConsensusReads, restated in numpy, as a reference for libbsdc's
bsdc_filter: a plain helper module like fgbio_vote.py.  It shares no code with the kernel or with
the package's filter module, and reads record by record, one template at a time, as fgbio's loop
does: the per-read values from the single-strand rows (as the tag encoder defines them, so a tool
reading the tagged BAM would see the same numbers), the read-level gate, the per-base mask, the
two checks after masking, and the template verdict.

Inputs are a consensus as oracle.run gives it (or pipeline.Consensus, unpacked): ``ss`` with "len"
[F, 4], "base" / "qual" / "depth" / "err" [F, 4, stride] (depth / err u16, or bytes with the wide
families' exact rows in "wide" / "wdepth" / "werr"), ``cons_seq`` / ``cons_qual`` [F, 2, stride],
``cons_len`` [F, 2], ``status`` (bit 0 = emitted).  Parameters are keyword arguments named after
bsdc_filter_params.
"""
from __future__ import annotations

import numpy as np

MINREADS, READERR, NOCALL, MEANQ = 1, 2, 4, 8
N, NO_CALL_QUAL = 15, 2


def three(v):
    """One value stands for (duplex, AB, BA) alike; two values (v0, v1) for (v0, v1, v1)."""
    v = list(v) if isinstance(v, (tuple, list)) else [v]
    assert 1 <= len(v) <= 3
    return v + [v[-1]] * (3 - len(v))


def _row(ss, f, s, L):
    """Single-strand row (f, s) cut to L columns: bases, quals, depths, errors (exact)."""
    d, e = ss["depth"][f, s, :L], ss["err"][f, s, :L]
    wide = ss.get("wide")
    if wide is not None and ss.get("wdepth") is not None and len(ss["wdepth"]) and int(wide[f]) >= 0:
        d, e = ss["wdepth"][int(wide[f]), s, :L], ss["werr"][int(wide[f]), s, :L]
    return (ss["base"][f, s, :L].astype(np.int64) & 15, ss["qual"][f, s, :L].astype(np.int64),
            d.astype(np.int64), e.astype(np.int64))


def _rate32(err_sum, depth_sum):
    """The tag encoder's E value: a float32 divide of the two sums, NaN with no depth."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(err_sum) / np.float32(depth_sum)


def _rates64(err, depth):
    """Per-column error rates in fp64, 0 where there is no depth."""
    return np.where(depth > 0, err.astype(np.float64) / np.maximum(depth, 1).astype(np.float64), 0.0)


def _nan0(x):
    return np.float32(0.0) if np.isnan(x) else x


def filter_record(ss, f, e, seq, qual, molecular, min_reads, max_read_error_rate, max_base_error_rate,
                  min_base_quality, max_no_call_fraction, min_mean_base_quality, require_single_strand_agreement):
    """One consensus read (family f, end e) with bases `seq` and `qual` (length L, not modified)
    -> (reason bits, masked seq, masked qual, newly masked columns)."""
    L = int(seq.shape[0])
    M, E, B = min_reads, max_read_error_rate, max_base_error_rate
    if molecular:
        rows = [e]
    else:  # strand rows (0, 3) for R1 and (1, 2) for R2: AB first, then BA; those present
        rows = [s for s in (e, 3 - e) if int(ss["len"][f, s]) > 0] or [3 - e]
    ab, aq, ad, ae = _row(ss, f, rows[0], L)
    two = len(rows) == 2
    if two:
        bb, bq, bd, be = _row(ss, f, rows[1], L)
    else:
        bd, be = np.zeros(L, np.int64), np.zeros(L, np.int64)
    # per-read values
    aD, aE = int(ad.max(initial=0)), _rate32(ae.sum(), ad.sum())
    bD, bE = (int(bd.max(initial=0)), _rate32(be.sum(), bd.sum())) if two else (0, np.float32(0.0))
    if two:
        # the duplex call before its N mask: the agreed base, else the strand of the higher quality,
        # AB on a tie; a strand that agrees with it counts its errors, one that does not all its reads
        raw = np.where(ab == bb, ab, np.where(aq > bq, ab, np.where(bq > aq, bb, ab)))
        cerr = np.where(ab == raw, ae, ad) + np.where(bb == raw, be, bd)
        cD, cE = int((ad + bd).max(initial=0)), _rate32(cerr.sum(), (ad + bd).sum())
    else:
        cD, cE = aD, aE
    # read-level gate
    reason = 0
    if cD < M[0]:
        reason |= MINREADS
    if float(cE) > E[0]:  # (NaN: False)
        reason |= READERR
    if not molecular:
        if max(aD, bD) < M[1] or min(aD, bD) < M[2]:
            reason |= MINREADS
        x, y = float(_nan0(aE)), float(_nan0(bE))
        if min(x, y) > E[1] or max(x, y) > E[2]:
            reason |= READERR
    if reason:
        return reason, seq, qual, 0
    # per-base mask, over the columns that hold a base
    q = qual.astype(np.int64)
    m = q < min_base_quality
    if molecular:
        m |= ad < M[0]
        m |= _rates64(ae, ad) > B[0]
    else:
        ra, rb = _rates64(ae, ad), _rates64(be, bd)
        m |= (ad + bd) < M[0]
        m |= _rates64(ae + be, ad + bd) > B[0]
        m |= np.maximum(ad, bd) < M[1]
        m |= np.minimum(ad, bd) < M[2]
        m |= np.minimum(ra, rb) > B[1]
        m |= np.maximum(ra, rb) > B[2]
        if require_single_strand_agreement and two:
            m |= ab != bb
    m &= seq != N
    seq, qual = np.where(m, N, seq).astype(np.uint8), np.where(m, NO_CALL_QUAL, qual).astype(np.uint8)
    # after masking
    n_n = int((seq == N).sum())
    if L > 0 and float(n_n) / float(L) > max_no_call_fraction:
        reason |= NOCALL
    if min_mean_base_quality >= 0 and int(qual.astype(np.int64).sum()) < min_mean_base_quality * L:
        reason |= MEANQ
    return reason, seq, qual, int(m.sum())


def apply(ss, cons_seq, cons_qual, cons_len, status, molecular=False, min_reads=(1,), max_read_error_rate=(0.025,),
          max_base_error_rate=(0.1,), min_base_quality=0, max_no_call_fraction=0.2, min_mean_base_quality=-1,
          require_single_strand_agreement=False):
    """-> (filt u8 [F], masked i32 [F, 2], seq, qual): a family's reason bits over both ends (0:
    kept, or not emitted and not looked at), the newly masked columns per end, and copies of the
    consensus with the mask applied (an end that passed the gate is masked even when the other end
    drops the template)."""
    M = [int(x) for x in three(min_reads)]
    E = [float(x) for x in three(max_read_error_rate)]
    B = [float(x) for x in three(max_base_error_rate)]
    F = int(np.asarray(status).shape[0])
    filt, masked = np.zeros(F, np.uint8), np.zeros((F, 2), np.int32)
    seq, qual = np.array(cons_seq, np.uint8), np.array(cons_qual, np.uint8)
    for f in range(F):
        if not int(status[f]) & 1:
            continue
        for e in range(2):
            L = int(cons_len[f, e])
            r, s, q, n = filter_record(ss, f, e, seq[f, e, :L], qual[f, e, :L], molecular, M, E, B,
                                       int(min_base_quality), float(max_no_call_fraction), int(min_mean_base_quality),
                                       bool(require_single_strand_agreement))
            filt[f] |= r
            masked[f, e] = n
            seq[f, e, :L], qual[f, e, :L] = s, q
    return filt, masked, seq, qual

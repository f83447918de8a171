"""Per-run consensus metrics: the accumulator's layout (include/bsdc.h
bsdc_metrics_words), the host twin's binding, and the JSON file of `--metrics`.  The reduction itself
runs on the device (libbsdc bsdc_metrics, device.Engine.metrics); this module is host-only and loads
no torch.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
from typing import Optional

import numpy as np

from . import _lib

DEFAULT_CYCLES = 512
# the accumulator's words (BSDC_METRICS_*)
FAMILIES, EMITTED, RECORDS, SKIPPED, KEPT, MINREADS, READERR, NOCALL, MEANQ, MASKED = range(10)
DEPTH_HIST = 16
RATE_HIST = DEPTH_HIST + 3 * 2 * 256
QUAL_HIST = RATE_HIST + 3 * 2 * 102
BY_CYCLE = QUAL_HIST + 2 * 95
KINDS = ("c", "a", "b")
ENDS = ("r1", "r2")
CYCLE_COLUMNS = ("records", "no_calls", "qual_sum", "depth_sum", "error_sum", "disagreements")


def words(cycles: int = DEFAULT_CYCLES) -> int:
    """The accumulator's length in u64 words (bsdc_metrics_words); ValueError outside 2..1024 cycles."""
    n = int(_lib.load().bsdc_metrics_words(int(cycles)))
    if n < 0:
        raise ValueError("metrics: cycles outside 2..1024 (%r)" % (cycles,))
    return n


def views(acc: np.ndarray, cycles: int) -> dict:
    """The accumulator's tables as numpy views: counts [16], depth_hist [3, 2, 256], rate_hist
    [3, 2, 102], qual_hist [2, 95], by_cycle [2, cycles, 6]."""
    acc = np.asarray(acc)
    assert acc.shape == (BY_CYCLE + 12 * cycles,), (acc.shape, cycles)
    return {"counts": acc[:DEPTH_HIST], "depth_hist": acc[DEPTH_HIST:RATE_HIST].reshape(3, 2, 256),
            "rate_hist": acc[RATE_HIST:QUAL_HIST].reshape(3, 2, 102), "qual_hist": acc[QUAL_HIST:BY_CYCLE].reshape(2, 95),
            "by_cycle": acc[BY_CYCLE:].reshape(2, cycles, 6)}


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host(acc: np.ndarray, cycles: int, status, length, seq_packed, qual, ss_len, ss_base, ss_qual, ss_depth, ss_err,
         ss_wide=None, ss_wdepth=None, ss_werr=None, molecular: bool = False, stride: Optional[int] = None):
    """The host twin (bsdc_metrics_host) over host arrays laid out as the device's: status u8 [F],
    length [F, 2], seq_packed u8 [F, 2, stride / 2], qual u8 [F, 2, stride], ss_len [F, 4], the rows
    u8 [F, 4, stride], ss_wide i32 [F] with ss_wdepth / ss_werr u16 [W, 4, stride] or None.  Adds
    into acc (uint64, metrics.words(cycles) long).  RuntimeError with the library's message on a
    refusal."""
    lib = _lib.load()
    F = int(np.asarray(status).shape[0])
    stride = int(qual.shape[-1]) if stride is None else int(stride)
    keep = [np.ascontiguousarray(status, np.uint8), np.ascontiguousarray(length).astype(np.uint16),
            np.ascontiguousarray(seq_packed, np.uint8), np.ascontiguousarray(qual, np.uint8),
            np.ascontiguousarray(ss_len).astype(np.uint16)] + \
        [np.ascontiguousarray(x, np.uint8) for x in (ss_base, ss_qual, ss_depth, ss_err)]
    o = _lib.ConsensusC()
    o.stride = stride
    o.status, o.len, o.seq, o.qual, o.ss_len, o.ss_base, o.ss_qual, o.ss_depth, o.ss_err = [x.ctypes.data for x in keep]
    W = 0
    if ss_wide is not None:
        wide = np.ascontiguousarray(ss_wide, np.int32)
        keep.append(wide)
        o.ss_wide = wide.ctypes.data
        if ss_wdepth is not None and len(ss_wdepth):
            wd, we = np.ascontiguousarray(ss_wdepth, np.uint16), np.ascontiguousarray(ss_werr, np.uint16)
            keep += [wd, we]
            o.ss_wdepth, o.ss_werr = wd.ctypes.data, we.ctypes.data
            W = int(wd.shape[0])
    assert acc.dtype == np.uint64 and acc.flags.c_contiguous
    rc = lib.bsdc_metrics_host(None, C.byref(o), F, W, 1 if molecular else 0, int(cycles), _ptr(acc))
    if rc != 0:
        raise RuntimeError("bsdc_metrics_host failed (%d): %s" % (rc, lib.bsdc_metrics_last_error().decode()))


def host_filter(acc: np.ndarray, status, filt, masked):
    """The filter counters' host twin (bsdc_metrics_filter_host): status u8 [F], filt u8 [F], masked [F, 2]."""
    lib = _lib.load()
    st, fl = np.ascontiguousarray(status, np.uint8), np.ascontiguousarray(filt, np.uint8)
    mk = np.ascontiguousarray(masked).astype(np.uint16)
    rc = lib.bsdc_metrics_filter_host(None, _ptr(st), _ptr(fl), _ptr(mk), int(st.shape[0]), _ptr(acc))
    if rc != 0:
        raise RuntimeError("bsdc_metrics_filter_host failed (%d): %s" % (rc, lib.bsdc_metrics_last_error().decode()))


def run_params(consensus_params, molecular: bool, flt=None) -> dict:
    """The parameters a run used, as the JSON carries them: the caller's rates and overlap flag,
    molecular or duplex, and the filter's parameters (filter.FilterParams) if one ran."""
    from .filter import three
    p = {"mode": "molecular" if molecular else "duplex",
         "error_rate_pre_umi": float(consensus_params.error_rate_pre_umi),
         "error_rate_post_umi": float(consensus_params.error_rate_post_umi),
         "consensus_call_overlapping_bases": bool(consensus_params.consensus_call_overlapping_bases),
         "min_consensus_base_quality": int(consensus_params.min_consensus_base_quality),
         "filter": None}
    if flt is not None:
        d = dataclasses.asdict(flt)
        for k in ("min_reads", "max_read_error_rate", "max_base_error_rate"):
            d[k] = list(three(d[k], k))
        p["filter"] = d
    return p


def report(acc: np.ndarray, cycles: int, params: Optional[dict] = None) -> dict:
    """The accumulator as the `--metrics` document: plain ints, keys in a fixed order, the trailing
    all-zero rows of by_cycle cut (the table's last row, when it is kept, is the sum of the columns
    at and past cycles - 1).  The filter's counters are there when params carries a filter."""
    v = views(np.asarray(acc, np.uint64), cycles)
    c = [int(x) for x in v["counts"]]
    doc = {"version": 1, "cycles": int(cycles), "params": params,
           "counts": {"families": c[FAMILIES], "families_emitted": c[EMITTED], "records": c[RECORDS],
                      "families_skipped": c[SKIPPED]}}
    if params is not None and params.get("filter") is not None:
        doc["counts"]["filter"] = {"families_kept": c[KEPT], "min_reads": c[MINREADS], "read_error": c[READERR],
                                   "no_call": c[NOCALL], "mean_quality": c[MEANQ], "masked_bases": c[MASKED]}
    doc["depth_hist"] = {k + "D": {e: v["depth_hist"][i, j].tolist() for j, e in enumerate(ENDS)} for i, k in enumerate(KINDS)}
    doc["rate_hist"] = {"bin_width": 0.001, "nan_bin": 101,
                        **{k + "E": {e: v["rate_hist"][i, j].tolist() for j, e in enumerate(ENDS)}
                           for i, k in enumerate(KINDS)}}
    doc["qual_hist"] = {"no_call_bin": 94, **{e: v["qual_hist"][j].tolist() for j, e in enumerate(ENDS)}}
    bc = v["by_cycle"]
    used = np.nonzero(bc.any(axis=(0, 2)))[0]
    n = int(used[-1]) + 1 if used.shape[0] else 0
    doc["by_cycle"] = {"columns": list(CYCLE_COLUMNS), "overflow_row": int(cycles) - 1,
                       **{e: bc[j, :n].tolist() for j, e in enumerate(ENDS)}}
    return doc


def write(path: str, acc: np.ndarray, cycles: int, params: Optional[dict] = None) -> dict:
    doc = report(acc, cycles, params)
    with open(path, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    return doc

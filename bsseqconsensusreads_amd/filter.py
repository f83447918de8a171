"""fgbio FilterConsensusReads options and bookkeeping.  The filter itself runs on
the device (libbsdc bsdc_filter, device.Engine.filter); this module is host-only and loads no torch.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib

# reason bits of Consensus.filt (bsdc.h BSDC_FILT_*), by their key in the info dict
REASONS = (("min_reads", _lib.FILT_MINREADS), ("read_error", _lib.FILT_READERR), ("no_call", _lib.FILT_NOCALL),
           ("mean_quality", _lib.FILT_MEANQ))


def three(v, what: str) -> tuple:
    """fgbio's one-to-three-valued flags, ordered duplex ("cc"), AB, BA: one value stands for all
    three, two values (v0, v1) for (v0, v1, v1)."""
    v = list(v) if isinstance(v, (tuple, list)) else [v]
    if not 1 <= len(v) <= 3:
        raise ValueError("%s takes one to three values" % what)
    return tuple(v + [v[-1]] * (3 - len(v)))


@dataclass
class FilterParams:
    """fgbio FilterConsensusReads options (bsdc_filter_params).  min_base_quality is fgbio's
    required -N; min_reads (-M, which fgbio requires too) defaults to 1 here, the rates and the
    no-call fraction to fgbio's defaults.  min_mean_base_quality None = off.  The library checks
    the domain (BSDC_EINVAL, the message names the field)."""

    min_base_quality: int
    min_reads: tuple = (1,)
    max_read_error_rate: tuple = (0.025,)
    max_base_error_rate: tuple = (0.1,)
    max_no_call_fraction: float = 0.2
    min_mean_base_quality: Optional[int] = None
    require_single_strand_agreement: bool = False

    def c_struct(self):
        p = _lib.FilterParamsC()
        p.min_reads[:] = [int(x) for x in three(self.min_reads, "min_reads")]
        p.max_read_error_rate[:] = [float(x) for x in three(self.max_read_error_rate, "max_read_error_rate")]
        p.max_base_error_rate[:] = [float(x) for x in three(self.max_base_error_rate, "max_base_error_rate")]
        p.min_base_quality = int(self.min_base_quality)
        p.max_no_call_fraction = float(self.max_no_call_fraction)
        p.min_mean_base_quality = -1 if self.min_mean_base_quality is None else int(self.min_mean_base_quality)
        p.require_single_strand_agreement = int(bool(self.require_single_strand_agreement))
        return p


def kept(cons) -> np.ndarray:
    """bool [F]: the families whose pair goes out -- emitted (status bit 0) and, with a filter,
    carrying no reason."""
    em = (cons.status & 1) != 0
    return em if getattr(cons, "filt", None) is None else em & (cons.filt == 0)


def empty_summary() -> dict:
    return {"templates": 0, "kept": 0, "dropped": {name: 0 for name, _ in REASONS}, "bases_masked": 0}


def summary(cons) -> dict:
    """The info dict's `filter` entry of one Consensus: templates looked at, kept, dropped per
    reason (a template may carry several), and the bases newly masked in the kept ones."""
    em = (cons.status & 1) != 0
    if cons.filt is None:  # (an input without a single family)
        return empty_summary()
    k = em & (cons.filt == 0)
    return {"templates": int(em.sum()), "kept": int(k.sum()),
            "dropped": {name: int((em & ((cons.filt & bit) != 0)).sum()) for name, bit in REASONS},
            "bases_masked": int(cons.masked[k].astype(np.int64).sum())}


def add_summary(total: dict, part: dict) -> dict:
    """Sum of two summaries (a stream's chunks)."""
    return {"templates": total["templates"] + part["templates"], "kept": total["kept"] + part["kept"],
            "dropped": {k: total["dropped"][k] + part["dropped"][k] for k in part["dropped"]},
            "bases_masked": total["bases_masked"] + part["bases_masked"]}

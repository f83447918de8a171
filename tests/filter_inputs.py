"""Inputs and parameter sets of the consensus-filter tests (a plain helper module, like
edge_inputs.py): test_filter_ref.py checks on the CPU, with oracle/ alone, that they reach the
filter's ground; test_gpu_filter.py runs the same ones through bsdc_filter.  Each input is built
once per process, with its oracle consensus, and must not be modified.
"""
from __future__ import annotations

import functools

import numpy as np

import edge_inputs as E
from bsseqconsensusreads_amd import pipeline, synth
from oracle import oracle

# Parameter sets (keyword arguments of filter_ref.apply; FilterParams takes the same names).  Every
# value the kernel compares against appears at both ends of its range in some set: min_reads (1),
# (3, 2, 1), (0); rates 0 and 1; min_base_quality 0 and 93; max_no_call_fraction 0 and 1;
# min_mean_base_quality off and 30; strand agreement on.
LAX = dict(min_reads=(0,), max_read_error_rate=(1.0,), max_base_error_rate=(1.0,), min_base_quality=0,
           max_no_call_fraction=1.0, min_mean_base_quality=-1, require_single_strand_agreement=False)
PARAM_SETS = {
    # the set that meets test_filter_ref's ground conditions on the main C2 input (seed 11): three
    # min_reads, three read rates, every reason bit set by some template, masked bases in kept ones
    # (the synthetic strands disagree far more often than real ones: the rates are set to match)
    "typical": dict(min_reads=(2, 1, 1), max_read_error_rate=(0.3, 0.25, 0.35), max_base_error_rate=(0.5, 0.5, 1.0),
                    min_base_quality=20, max_no_call_fraction=0.5, min_mean_base_quality=30,
                    require_single_strand_agreement=False),
    # the same for the step-1 input (seed 13)
    "molecular_typical": dict(min_reads=(2,), max_read_error_rate=(0.025,), max_base_error_rate=(0.1,),
                              min_base_quality=30, max_no_call_fraction=0.1, min_mean_base_quality=42,
                              require_single_strand_agreement=False),
    # one-strand families pass the gate (BA may show no read), strands must agree
    "single_ok": dict(min_reads=(2, 1, 0), max_read_error_rate=(0.5, 0.4, 0.5), max_base_error_rate=(0.4, 0.3, 0.5),
                      min_base_quality=10, max_no_call_fraction=0.5, min_mean_base_quality=-1,
                      require_single_strand_agreement=True),
    "lax": LAX,                                               # nothing dropped, nothing masked
    "ones": dict(LAX, min_reads=(1,)),
    "three_reads": dict(LAX, min_reads=(3, 2, 1)),
    "fgbio_defaults": dict(min_reads=(1,), max_read_error_rate=(0.025,), max_base_error_rate=(0.1,), min_base_quality=2,
                           max_no_call_fraction=0.2, min_mean_base_quality=-1, require_single_strand_agreement=False),
    "rates0": dict(LAX, min_reads=(1,), max_read_error_rate=(0.0,), max_base_error_rate=(0.0,)),
    "base_rate0": dict(LAX, min_reads=(1,), max_base_error_rate=(0.0,)),
    "two_reads": dict(LAX, min_reads=(2, 1), max_base_error_rate=(1.0, 0.05)),
    "q93": dict(LAX, min_base_quality=93),                    # every base masked, every read kept
    "q93_nocall0": dict(LAX, min_base_quality=93, max_no_call_fraction=0.0),
    "nocall0": dict(LAX, max_no_call_fraction=0.0),           # a read with any N is dropped
    "meanq30": dict(LAX, min_mean_base_quality=30),
    "agree": dict(LAX, min_reads=(1,), require_single_strand_agreement=True),
}


def filter_params(p: dict):
    """The set as the package's FilterParams."""
    from bsseqconsensusreads_amd.filter import FilterParams
    q = p["min_mean_base_quality"]
    return FilterParams(p["min_base_quality"], tuple(p["min_reads"]), tuple(p["max_read_error_rate"]),
                        tuple(p["max_base_error_rate"]), p["max_no_call_fraction"], None if q < 0 else q,
                        p["require_single_strand_agreement"])


class Case:
    """One input: raw records, reference, whether it runs as step 1 (molecular), and its oracle
    consensus (an OracleResult; for molecular, over pipeline.molecular_records(raw))."""

    def __init__(self, raw, ref, molecular=False):
        self.raw, self.ref, self.molecular = raw, ref, molecular
        if molecular:
            self.oracle = oracle.run(pipeline.molecular_records(raw), ref, run_tools=False, family_order="mi-group",
                                     min_consensus_base_quality=0, threads=8)
        else:
            self.oracle = oracle.run(raw, ref, threads=8)

    def reference(self, p: dict):
        """filter_ref over the oracle consensus -> (filt, masked, seq, qual)."""
        import filter_ref
        r = self.oracle
        return filter_ref.apply(r.ss, r.cons_seq, r.cons_qual, r.cons_len, r.status, molecular=self.molecular, **p)


def _round_families():
    """Consensus lengths 511 / 512 / 513 (a lane's round is 512 columns) and 520, 1040 beside them:
    duplex, AB-only and BA-only families of 1-3 templates each."""
    rng = np.random.default_rng(21)
    fams = []
    for L in (511, 512, 513, 520, 1040, 512, 513, 511):
        for na, nb in ((2, 1), (3, 0), (0, 2), (1, 1)):
            fams.append(E.Family(na, nb, [(L, L)] * (na + nb), 0, L + int(rng.integers(0, 8)),
                                 ab_top=bool(rng.random() < 0.5)))
    glen = 4000
    for f, s in zip(fams, E._place(rng, len(fams), [f.frag for f in fams], glen)):
        f.start = s
    return E.build(fams, E.q_bins, seed=22, contig_len=glen, extra_error=0.01)


def _strand_families():
    """AB-only, BA-only and duplex families interleaved with families that emit nothing (a lone
    R1: no R2 set, so no pair)."""
    rng = np.random.default_rng(31)
    fams = []
    for k in range(90):
        kind = k % 5
        L = int(rng.integers(20, 60))
        nt = int(rng.integers(1, 5))
        if kind == 0:
            f = E.Family(nt, 0, [(L, L)] * nt, 0, L + 5)
        elif kind == 1:
            f = E.Family(0, nt, [(L, L)] * nt, 0, L + 5)
        elif kind == 2:
            f = E.Family(0, 0, [], 0, L + 5, unpaired_r1=L)
        else:
            f = E.Family(nt, nt, [(L, L)] * (2 * nt), 0, L + 5, ab_top=kind == 3)
        fams.append(f)
    glen = 3000
    for f, s in zip(fams, E._place(rng, len(fams), [f.frag for f in fams], glen)):
        f.start = s
    return E.build(fams, E.q_full_range, seed=32, contig_len=glen, extra_error=0.02)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    if name == "c2":  # ~2,000 messy C2 families: k_small
        s = synth.generate("C2", 2000, seed=11, device="cpu", genome_len=400_000)
        return Case(synth.messify(s.raw, frac=0.1, seed=2), s.ref)
    if name == "c3":  # ~60 C3 families (40-200 records each): most through k_large
        s = synth.generate("C3", 60, seed=29, device="cpu", genome_len=200_000)
        return Case(synth.messify(s.raw, frac=0.1, seed=3), s.ref)
    if name == "molecular":  # step-1 records: every MI run a family, one strand per end
        s = synth.generate("C2", 500, seed=13, device="cpu", genome_len=200_000)
        return Case(synth.messify(s.raw, frac=0.1, seed=4), s.ref, molecular=True)
    if name == "tiny":  # reads of 1-9 bases
        es = E.length_case("tiny")
    elif name.startswith("stride"):  # max_len + 2 on and beside a multiple of 16
        es = E.stride_case(int(name[6:]))
    elif name == "rounds":
        es = _round_families()
    elif name == "strands":
        es = _strand_families()
    elif name == "wide":  # one AB-only family of 520 records (set depths 260, past a byte) among small ones
        es = E.size_case(True, sizes=(2, 3, 64, 65), reps=2)
    else:
        raise KeyError(name)
    return Case(es.raw, es.ref)


EDGE_CASES = ("tiny", "stride47", "stride48", "stride49", "rounds", "strands", "wide")

"""The HIP vote against the independent fp64 restatement of fgbio (tests/fgbio_vote.py), through
the C-ABI: single-strand reads (BSDC_MODE_TAGS) and duplex consensus on C0-C4 and on adversarial
near-tie columns, in both kernels (k_small, and k_large with every family forced into it).

Bar (north_star): consensus bases bit-exact and quals within +-1 of fgbio's double-precision
log-space arithmetic, on every column: exact ties (the same multiset of qualities on two bases)
included, where fgbio's pick is the rounding of its read-order double sums and the kernels' near-tie
path (fp64_pick) reproduces it.  Counts are printed (run with -s) and asserted.
"""
import numpy as np
import pytest

from bsseqconsensusreads_amd import batch, pipeline, synth
from helpers import gpu_vs_fp64, near_tie_votes
from test_fgbio_vote import CASES, low_quality_votes

pytestmark = pytest.mark.gpu


def _gpu_vs_fp64(engine, raw, ref, run_tools, what, molecular=False):
    """helpers.gpu_vs_fp64 (shared with tests/test_gpu_edges.py) at the default flags."""
    return gpu_vs_fp64(engine, raw, ref, run_tools, what, molecular=molecular)[0]


@pytest.mark.parametrize("cfg,n,qlo", CASES)
def test_gpu_vote_vs_fgbio_fp64(engine, cfg, n, qlo):
    s = synth.generate(cfg, n, seed=11, device="cpu", genome_len=400_000)
    raw = s.raw if qlo is None else near_tie_votes(s.raw, qlo=qlo, seed=5)
    _gpu_vs_fp64(engine, raw, s.ref, qlo is None, "%s n=%d q>=%s" % (cfg, n, qlo))


@pytest.mark.parametrize("qlo", [84, 88])
def test_gpu_large_kernel_near_ties_vs_fgbio_fp64(engine, qlo, monkeypatch):
    """Every family through k_large (its near-tie path in `resolve` and the tag pass)."""
    s = synth.generate("C1", 800, seed=13, device="cpu", genome_len=200_000)
    raw = near_tie_votes(s.raw, qlo=qlo, seed=7)
    real = batch.materialize
    monkeypatch.setattr(pipeline, "materialize",
                        lambda plan, f0, f1, small_cap=0, images=None: real(plan, f0, f1, small_cap=0, images=images))
    _gpu_vs_fp64(engine, raw, s.ref, False, "k_large q>=%d" % qlo)


def _force_large(monkeypatch):
    real = batch.materialize
    monkeypatch.setattr(pipeline, "materialize",
                        lambda plan, f0, f1, small_cap=0, images=None: real(plan, f0, f1, small_cap=0, images=images))


@pytest.mark.parametrize("kernel", ["small", "large"])
@pytest.mark.parametrize("caller", ["duplex", "molecular"])
def test_gpu_min_consensus_base_quality(engine, kernel, caller, monkeypatch):
    """Q0-Q3 disagreement columns (Q1 calls, all-N columns) in both kernels and both callers:
    step 5's duplex caller masks single-strand Q < 2 to (N, 2), step 1 (main.snake.py:54,
    --min-consensus-base-quality=0) keeps the call at Q1; GPU == oracle/ bit for bit, and both
    within the fp64 bar of fgbio's arithmetic.  The engine's own flags are restored afterwards."""
    from bsseqconsensusreads_amd import records as R
    s = synth.generate("C1", 600, seed=17, device="cpu", genome_len=200_000)
    raw = low_quality_votes(s.raw, seed=9)
    if caller == "molecular":
        raw = R.take(raw, np.lexsort((raw.mi_strand, raw.mi_id)))
    if kernel == "large":
        _force_large(monkeypatch)
    cons = _gpu_vs_fp64(engine, raw, s.ref, False, "low-quality %s %s" % (caller, kernel),
                        molecular=caller == "molecular")
    w = cons.ss["qual"].shape[2]
    em = (cons.status & 1) != 0
    live = (np.arange(w)[None, None, :] < cons.ss["len"][:, :, None]) & em[:, None, None]
    q1 = int((live & (cons.ss["qual"] == 1)).sum())
    assert (q1 > 50) if caller == "molecular" else (q1 == 0)
    assert engine.params.min_consensus_base_quality == 2

"""The stream's shared stages (bsseqconsensusreads_amd/stream.py: FrontEnd, BackEnd, Chunk) on the
CPU with the oracle stand-in of tests/test_stream_pipeline.py: whichever stage fails on its second
chunk, the caller gets that error, every stage thread has ended and no spill or second-pass file is
left -- through bam.step5_stream and, for a front-end and a back-end stage, through
fleet.step5_stream_multi, which runs the same two ends; and a chunk's pooled buffers are given back
exactly once."""
import os
import threading

import pytest

from bsseqconsensusreads_amd import bam, fleet, pipeline
from test_gpu_stream import _inputs
from test_stream_pipeline import standin  # noqa: F401 -- (the fixture)

CHUNK = dict(chunk_bytes=25_000, slack=2000)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return _inputs(tmp_path_factory.mktemp("stages"), "C2", 400, 0.0, 31)


def _fail_on_second(monkeypatch, owner, name, before=None):
    """owner.name raises on its second call (after `before`, e.g. giving a chunk back)."""
    orig, calls = getattr(owner, name), {"n": 0}

    def failing(*a, **k):
        calls["n"] += 1
        if calls["n"] == 2:
            if before is not None:
                before(*a, **k)
            raise RuntimeError("%s failed on purpose" % name)
        return orig(*a, **k)
    monkeypatch.setattr(owner, name, failing)
    return calls


STAGES = {
    "reader": (bam.StreamChunk, "decode", lambda self, *a, **k: self.discard()),
    "planner": (pipeline, "plan_families", None),
    "gpu": (pipeline, "run_batches", None),
    "builder": (bam, "duplex_records", None),
    "writer": (bam.BamWriter, "add", None),
}


def _leftovers(d):
    return sorted(x for x in os.listdir(d) if ".spill" in x or ".p2" in x or x.endswith(".asm"))


@pytest.mark.parametrize("stage", list(STAGES))
def test_a_failing_stage_surfaces_and_every_thread_ends(standin, inputs, tmp_path, monkeypatch, stage):  # noqa: F811
    inp, fa = inputs
    owner, name, before = STAGES[stage]
    calls = _fail_on_second(monkeypatch, owner, name, before)
    n0 = threading.active_count()
    with pytest.raises(RuntimeError, match="%s failed on purpose" % name):
        bam.step5_stream(inp, fa, str(tmp_path / "x.bam"), engine=standin, threads=2, level=1,
                         fastq=(str(tmp_path / "x1.fq.gz"), str(tmp_path / "x2.fq.gz")), **CHUNK)
    assert calls["n"] >= 2
    assert threading.active_count() == n0
    assert _leftovers(tmp_path) == []


@pytest.mark.parametrize("stage", ["planner", "writer"])
def test_a_failing_stage_surfaces_through_the_fleet(inputs, tmp_path, monkeypatch, stage):
    """The same front end and back end under fleet.step5_stream_multi (two stand-in workers): the
    error reaches the caller, the stage threads and the collector have ended (the segment pool's
    prefill thread and the queues' feeders are the fleet's own), the workers are gone."""
    inp, fa = inputs
    owner, name, before = STAGES[stage]
    _fail_on_second(monkeypatch, owner, name, before)
    fl = fleet.Fleet([0, 0], "fleet_standin:OracleRunner", 2)
    try:
        with pytest.raises(RuntimeError, match="%s failed on purpose" % name):
            fleet.step5_stream_multi(inp, fa, str(tmp_path / "f.bam"), [0, 0], threads=2, level=1,
                                     batch_bases=40_000, fleet=fl, **CHUNK)
        assert [t.name for t in threading.enumerate() if t.name.startswith("stream_")] == []
    finally:
        fl.close()
    assert all(not p.is_alive() for p in fl.procs)
    assert _leftovers(tmp_path) == []


@pytest.mark.parametrize("tags", [True, False])
def test_a_chunks_pooled_buffers_are_given_back_once(standin, inputs, tmp_path, monkeypatch, tags):  # noqa: F811
    """Per chunk one buffer of records (bam.StreamChunk.decode) and, with tags, one of tag bytes
    (bam.consensus_tags): each taken from the pool and given back when the chunk is written."""
    inp, fa = inputs
    taken, given = [], []
    take, give = bam.BufferPool.take, bam.BufferPool.give

    def counted_take(self, nbytes):
        buf = take(self, nbytes)
        taken.append(id(buf))
        return buf

    def counted_give(self, buf):
        if buf is not None:
            given.append(id(buf))
        return give(self, buf)
    monkeypatch.setattr(bam.BufferPool, "take", counted_take)
    monkeypatch.setattr(bam.BufferPool, "give", counted_give)
    info = bam.step5_stream(inp, fa, str(tmp_path / "p.bam"), engine=standin, threads=2, level=1, tags=tags, **CHUNK)
    assert info["chunks"] > 4
    assert len(given) == (2 if tags else 1) * info["chunks"]
    assert sorted(given) == sorted(taken)  # every buffer taken went back, none twice

"""The family images gathered on the GPU (bsdc_image_gather, csrc/bsdc_image.hip; --gpu-image): the
kernel against its host twin on every case of tests/image_inputs.py, the launcher's refusals, whole
batches with device images against host images and oracle/, and the command line's output files
with the option against those without, byte for byte."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import image_inputs as I
from bsseqconsensusreads_amd import _lib, batch, pipeline, records as R, synth
from oracle import oracle
from test_gpu_parity import assert_consensus_equal, assert_ss_equal

pytestmark = pytest.mark.gpu


def _kernel(engine, raw_bases, table, n_slots):
    """bsdc_image_gather -> (rc, seq image, qual image, message); the images start as 0xA5 and the
    tensors hold 64 bytes more, which must stay 0xA5."""
    import torch
    dev = engine.device
    rb = torch.from_numpy(I.padded(raw_bases).copy() if raw_bases.shape[0] else np.zeros(4, np.uint8)).to(dev)
    t = np.ascontiguousarray(table)
    td = torch.from_numpy(t.view(np.uint8).copy() if t.shape[0] else np.zeros(8, np.uint8)).to(dev)
    seq = torch.full((n_slots // 2 + 64,), 0xA5, dtype=torch.uint8, device=dev)
    qual = torch.full((n_slots + 64,), 0xA5, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    rc = engine.lib.bsdc_image_gather(engine.ctx, C.c_void_p(rb.data_ptr()), int(raw_bases.shape[0]),
                                      C.c_void_p(td.data_ptr()), C.c_void_p(t.ctypes.data), t.shape[0], n_slots,
                                      C.c_void_p(seq.data_ptr()), C.c_void_p(qual.data_ptr()), C.c_void_p(s.cuda_stream))
    s.synchronize()
    sq, ql = seq.cpu().numpy(), qual.cpu().numpy()
    assert (sq[n_slots // 2:] == 0xA5).all() and (ql[n_slots:] == 0xA5).all()
    return rc, sq[:n_slots // 2], ql[:n_slots], engine.lib.bsdc_last_error(engine.ctx).decode()


@pytest.mark.parametrize("name", I.CASE_NAMES)
def test_kernel_equals_twin(engine, name):
    _, packed, fh, fg = I.built(name)
    rc, seq, qual, msg = _kernel(engine, packed.raw_bases, fg.gather, fg.n_slots)
    assert rc == 0, msg
    rc, ts, tq, msg = I.twin(packed.raw_bases, fg.gather, fg.n_slots)
    assert rc == 0, msg
    assert np.array_equal(qual, tq) and np.array_equal(seq, ts)
    assert np.array_equal(qual, fh.qual[:fh.n_slots]) and np.array_equal(seq, fh.seq[:fh.n_slots // 2])


def test_kernel_equals_twin_on_the_table_case(engine):
    rb, table, n_slots = I.table_case()
    rc, seq, qual, msg = _kernel(engine, rb, table, n_slots)
    assert rc == 0, msg
    _, ts, tq, _ = I.twin(rb, table, n_slots)
    assert np.array_equal(qual, tq) and np.array_equal(seq, ts)
    rc, seq, qual, msg = _kernel(engine, rb, table[:0], 64)  # an empty table: zeroed images
    assert rc == 0 and not seq.any() and not qual.any()


def test_launcher_refuses_bad_tables(engine):
    """BSDC_EINVAL from the launcher's checks, the field named, nothing launched: the images keep
    their fill."""
    rb, table, n_slots = I.table_case()
    for what, t in I.bad_tables(rb, table, n_slots):
        rc, seq, qual, msg = _kernel(engine, rb, t, n_slots)
        assert rc == -22 and what in msg, (what, rc, msg)
        assert (seq == 0xA5).all() and (qual == 0xA5).all()
    rc, seq, qual, msg = _kernel(engine, rb, table, n_slots + 4)
    assert rc == -22 and "n_slots" in msg and (qual == 0xA5).all()


def _both(engine, raw, ref, mode, plan_mode, order, molecular=False, part_cap=None):
    """run_batches over the same families with host images and with device images -> both."""
    out = []
    for gather in (False, True):
        r = R.pack_bases(raw, 1, 0) if gather else raw
        plan = batch.plan_families(r, plan_mode, ref, family_order=order)
        assert not plan.split_ext
        fbs = []
        for a, b in pipeline.plan_ranges(plan, 4_000_000):
            if part_cap is None:
                fbs.append(batch.materialize(plan, a, b, gather=gather))
            else:
                fbs.append(I._materialize_range(plan, a, b, gather, part_cap))
        assert all((fb.gather is not None) == gather for fb in fbs)
        cons = pipeline.concat_consensus(pipeline.run_batches(engine, fbs, mode, True, molecular=molecular,
                                                              raw_bases=r.raw_bases if gather else None))
        out.append((cons, fbs))
    return out


FULL = pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE


@pytest.mark.parametrize("cfg,n_fam,part_cap", [("C2", 2000, None), ("C3", 60, None), ("C4", 250, 30_000)])
def test_batches_with_device_images(engine, cfg, n_fam, part_cap):
    s = synth.generate(cfg, n_fam, seed=23, device="cpu", genome_len=300_000)
    engine.load_reference(s.ref)
    (h, fh), (g, fg) = _both(engine, s.raw, s.ref, FULL, "full", "template-coordinate", part_cap=part_cap)
    if part_cap is not None:
        assert sum(fb.split_fams.shape[0] for fb in fg) > 0  # cut families: their images re-laid by the gather
    for k in ("status", "length", "seq", "qual"):
        assert np.array_equal(getattr(h, k), getattr(g, k)), k
    for k in ("len", "base", "qual", "depth", "err"):
        assert np.array_equal(h.ss[k], g.ss[k]), "ss " + k
    ref = oracle.run(s.raw, s.ref)
    for cons, what in ((h, "host images"), (g, "device images")):
        assert_consensus_equal(cons, ref, what + " " + cfg)
        assert_ss_equal(cons, ref, what + " " + cfg)


def test_molecular_batches_with_device_images(engine):
    s = synth.generate("C2", 600, seed=29, device="cpu", genome_len=200_000)
    rm = pipeline.molecular_records(s.raw)
    with engine.flags(min_consensus_base_quality=0):
        (h, _), (g, _) = _both(engine, rm, None, pipeline.MODE_VOTE, "vote", "mi-group", molecular=True)
    for k in ("status", "length", "seq", "qual"):
        assert np.array_equal(getattr(h, k), getattr(g, k)), k
    ref = oracle.run(rm, s.ref, run_tools=False, family_order="mi-group", min_consensus_base_quality=0)
    assert_consensus_equal(g, ref, "molecular device images")


# ---- the command line
from test_gpu_bam_device import _cli, _step5, COUNTERS, long_bam  # noqa: E402,F401


@pytest.mark.parametrize("more", [(), ("--gpu-inflate", "true"), ("--gpu-fastq", "true", "--gpu-bam", "true"),
                                  ("--gpu-bam", "true", "--filter-min-base-quality", "20", "--filter-min-reads", "2", "1", "1"),
                                  ("--output-per-base-tags", "false")],
                         ids=["alone", "inflate", "fastq_bam", "bam_filtered", "notags"])
def test_cli_step5(capsys, long_bam, more):
    """far templates, the deferral's cuts and its second pass: the BAM and the FASTQ pair with
    --gpu-image true are those without it, byte for byte"""
    t = "%d%s" % (len(more), more[0][6:9] if more else "")
    base, b0, fq0 = _step5(capsys, long_bam, "i0" + t, True, *more)
    info, b1, fq1 = _step5(capsys, long_bam, "i1" + t, True, "--gpu-image", "true", *more)
    assert info["spliced_families"] > 0 and info["spilled_bytes"] > 0 and info.get("deferred_records", 0) > 0
    assert b1 == b0 and fq1 == fq0
    for k in COUNTERS:
        assert info[k] == base[k], k


def test_cli_molecular(capsys, tmp_path):
    from test_molecular_stream import grouped_bam
    _, p = grouped_bam(tmp_path, n_fam=1500)
    runs = {}
    for tag, more in (("d", ()), ("g", ("--gpu-image", "true")), ("db", ("--gpu-bam", "true")),
                      ("gb", ("--gpu-bam", "true", "--gpu-image", "true"))):
        out = str(tmp_path / (tag + ".bam"))
        fq = [str(tmp_path / ("%s_%d.fq.gz" % (tag, d))) for d in (1, 2)]
        info = _cli(capsys, ["molecular", p, out, "--threads", "4", "--chunk-mb", "1", "--fastq1", fq[0], "--fastq2", fq[1]] +
                    list(more))
        runs[tag] = (info, open(out, "rb").read(), [open(x, "rb").read() for x in fq])
    assert runs["g"][1] == runs["d"][1] and runs["g"][2] == runs["d"][2]
    assert runs["gb"][1] == runs["db"][1] and runs["gb"][2] == runs["db"][2]
    assert runs["g"][0]["records_out"] == runs["d"][0]["records_out"] > 0

"""bsdc_filter (csrc/bsdc_filter.hip) on resident C2 families: the kernel alone,
timed with HIP events after a warm-up, against a device-to-device copy that moves the same number
of bytes in the same process, and (--e2e) the wall time of `cli step5` -> filtered FASTQ against
`cli step5` -> tagged BAM (the file a user must write today before FilterConsensusReads can run)
on one input file.

Bytes of the kernel, from the layout (not from counters): per emitted family and end of length L,
the single-strand rows present (1 or 2) x 4 arrays x L, the packed seq (L / 2) and qual (L) read,
the same two written back where the end holds a masked column, and per family status, both len,
four ss_len, filt and both masked (18 B).  The copy is of half that many bytes, so that its reads
plus writes equal the kernel's.  Two parameter sets: "typical" (tests/filter_inputs.py's, part of
the reads fail the gate and skip the second sweep) and "all_masked" (every read passes the gate and
every base is rewritten: the most traffic the kernel can have).
Usage (GPU box): python profiles/filter_bench.py [--families 1000000] [--reps 20] [--e2e DIR]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, the MI355X's specified peak


def kernel_leg(a):
    import torch

    from bsseqconsensusreads_amd import batch as B
    from bsseqconsensusreads_amd import pipeline, synth
    from bsseqconsensusreads_amd.device import Engine
    from bsseqconsensusreads_amd.filter import FilterParams
    sets = {"typical": FilterParams(20, (2, 1, 1), (0.3, 0.25, 0.35), (0.5, 0.5, 1.0), 0.5, 30, False),
            "all_masked": FilterParams(93, (0,), (1.0,), (1.0,), 1.0, None, False)}
    eng = Engine(0)
    s = synth.generate("C2", a.families, seed=42, device="cuda")
    eng.load_reference(s.ref)
    fb = B.build_family_batch(s.raw, "full", s.ref)
    db = eng.upload(fb, tags=True, filt=True)
    eng.run(db, pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE | pipeline.MODE_TAGS)
    seq0, qual0 = db.seq.clone(), db.qual.clone()
    status, length = db.fetch_lengths()
    ss_len = db.ss_len[:4 * db.n_fam].cpu().numpy().view(np.uint16).reshape(-1, 4)
    em = (status & 1) != 0
    rows = np.stack([(ss_len[:, 0] > 0).astype(np.int64) + (ss_len[:, 3] > 0), (ss_len[:, 1] > 0).astype(np.int64) + (ss_len[:, 2] > 0)], 1)
    L = length.astype(np.int64)
    st = torch.cuda.current_stream()
    out = {"families": int(db.n_fam), "emitted": int(em.sum()), "stride": int(db.stride)}
    for name, fp in sets.items():
        ms = []
        for i in range(a.warmup + a.reps):
            db.seq.copy_(seq0)
            db.qual.copy_(qual0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            eng.filter(db, fp)
            e1.record(st)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        o = db.fetch(ss=False)
        wrote = o["masked"] > 0
        nbytes = int((rows[em] * 4 * L[em]).sum() + (L[em] * 3 // 2).sum() + (L * 3 // 2)[em[:, None] & wrote].sum()) + 18 * db.n_fam
        half = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(half)
        cs = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            dst.copy_(half)
            e1.record(st)
            torch.cuda.synchronize()
            if i >= a.warmup:
                cs.append(e0.elapsed_time(e1))
        k, c = float(np.median(ms)), float(np.median(cs))
        out[name] = {"kernel_ms": round(k, 4), "kernel_ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                     "copy_ms": round(c, 4), "bytes": nbytes, "kernel_over_copy": round(k / c, 3),
                     "kernel_GBps": round(nbytes / k / 1e6, 1), "copy_GBps": round(nbytes / c / 1e6, 1),
                     "kernel_fraction_of_hbm_peak": round(nbytes / (k / 1e3) / HBM_PEAK, 4),
                     "kept": int((em & (o["filt"] == 0)).sum()), "bases_masked": int(o["masked"].sum())}
    eng.close()
    return out, s


def e2e_leg(a, s):
    """One coordinate-sorted BAM of the kernel leg's families; `cli step5` twice on it."""
    from bsseqconsensusreads_amd import bam, cli
    from bsseqconsensusreads_amd import records as R
    os.makedirs(a.e2e, exist_ok=True)
    raw = R.take(s.raw, np.lexsort((s.raw.pos, s.raw.tid)))
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in
                                                    zip(s.ref.names, s.ref.lengths)) + "@RG\tID:A\tSM:s\tLB:L\n"
    inp, fa = os.path.join(a.e2e, "in.bam"), os.path.join(a.e2e, "g.fa")
    bam.write_bam(inp, bam.BamHeader(text, list(s.ref.names), np.asarray(s.ref.lengths, np.int64)),
                  bam.records_to_bam(raw), level=1, threads=16)
    codes = R.unpack_nibbles(s.ref.packed, s.ref.n_nibbles)
    with open(fa, "wb") as fh:
        fh.write((">%s\n" % s.ref.names[0]).encode() + R.NT16_TO_ASCII[codes].tobytes() + b"\n")
    out = {"input_MB": round(os.path.getsize(inp) / 1e6, 1)}
    flt = ["--filter-min-base-quality", "20", "--filter-min-reads", "2", "1", "1", "--filter-max-read-error-rate", "0.3",
           "0.25", "0.35", "--filter-max-base-error-rate", "0.5", "0.5", "1.0", "--filter-max-no-call-fraction", "0.5",
           "--filter-min-mean-base-quality", "30"]
    legs = {"filtered_fastq_s": ["-", "--fastq1", os.path.join(a.e2e, "f1.fq.gz"), "--fastq2", os.path.join(a.e2e, "f2.fq.gz")] + flt,
            "tagged_bam_s": [os.path.join(a.e2e, "tagged.bam")]}
    for rep in range(2):  # (the second pass is the one reported: the first warms the page cache)
        for k, tail in legs.items():
            t0 = time.perf_counter()
            rc = cli.main(["step5", "--reference", fa, inp] + tail + ["--threads", "16"])
            out[k] = round(time.perf_counter() - t0, 2)
            assert rc == 0, k
    out["tagged_bam_MB"] = round(os.path.getsize(os.path.join(a.e2e, "tagged.bam")) / 1e6, 1)
    out["filtered_fastq_MB"] = round(sum(os.path.getsize(os.path.join(a.e2e, n)) for n in ("f1.fq.gz", "f2.fq.gz")) / 1e6, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e", metavar="DIR", default=None, help="also time cli step5 on a BAM of the families, written here")
    a = ap.parse_args()
    out, s = kernel_leg(a)
    print(json.dumps(out), flush=True)
    if a.e2e:
        print(json.dumps({"e2e": e2e_leg(a, s)}), flush=True)


if __name__ == "__main__":
    main()

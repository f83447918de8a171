"""The device FASTQ kernels alone (csrc/bsdc_fastq.hip): bsdc_fastq_format on a voted
C2 batch (Engine.fastq's launch) and bsdc_bgzf_crc32 over the whole blocks of its text, two warm-up
runs and seven timed ones each (HIP events) -> min / median / max ms and GB/s of text, written to
profiles/fastq_bench.json.  Usage: python profiles/fastq_bench.py [--families 200000]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warm=2, runs=7):
    import torch
    ms = []
    for k in range(warm + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_bench.json"))
    a = ap.parse_args()
    import torch

    from bsseqconsensusreads_amd import bam, pipeline, synth
    from bsseqconsensusreads_amd.device import Engine
    s = synth.generate("C2", a.families, seed=42, device="cuda", genome_len=50_000_000)
    eng = Engine(0)
    eng.load_reference(s.ref)
    fb = pipeline.build_family_batch(s.raw, "full", eng.ref)
    db = eng.upload(fb)
    eng.run(db, pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE)
    names = bam.family_names(fb.fam_mi, s.raw.mi_names, "bench")
    fq = eng.fastq(db, names)
    small = db.fetch(seqqual=False)
    total = small["fastq_total"]
    # the same launch again on the same buffers (Engine.fastq's arguments, without its allocations)
    lib = eng.lib
    dev = eng.device
    off_h = fq.name_off
    d_off = torch.from_numpy(off_h).to(dev)
    d_buf = torch.from_numpy(np.ascontiguousarray(names.buf)).to(dev)
    tmp = torch.empty(int(lib.bsdc_fastq_tmp_bytes(db.n_fam)), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fmt():
        rc = lib.bsdc_fastq_format(C.byref(db._o), None, db.n_fam, d_off.data_ptr(), d_buf.data_ptr(),
                                   off_h.ctypes.data, fq.off[0].data_ptr(), fq.off[1].data_ptr(), fq.text[0].data_ptr(),
                                   fq.text[1].data_ptr(), fq.cap[0], fq.cap[1], tmp.data_ptr(), st)
        assert rc == 0, rc
    nblk = total[0] // 65280
    crc = torch.empty(max(nblk, 1), dtype=torch.int32, device=dev)

    def crc32():
        assert lib.bsdc_bgzf_crc32(fq.text[0].data_ptr(), 0, nblk, crc.data_ptr(), st) == 0
    res = {"families": a.families, "families_emitted": int((small["status"] & 1).sum()), "stride": db.stride,
           "text_bytes": [int(total[0]), int(total[1])], "crc_blocks": int(nblk), "device": torch.cuda.get_device_name(0)}
    for name, fn, nbytes in (("fastq_format", fmt, total[0] + total[1]), ("bgzf_crc32", crc32, nblk * 65280)):
        ms = sorted(timed(fn))
        med = ms[len(ms) // 2]
        res[name] = {"ms_min": round(ms[0], 4), "ms_median": round(med, 4), "ms_max": round(ms[-1], 4),
                     "bytes": int(nbytes), "GBps_at_median": round(nbytes / med / 1e6, 2)}
    eng.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

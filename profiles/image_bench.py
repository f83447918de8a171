"""The family-image gather alone (bsdc_image_gather) on the records of one C2 batch,
beside the host's image fill (hostplan.materialize with images, --threads host threads) over the
same batch: two warm-ups and seven timed runs each, min / median / max.  The kernel's time is the
two memsets plus k_image_gather between two events on one stream; the host figure is the whole of
materialize (the image fill is not timed apart from the other arrays; materialize without images,
which the gather path still runs, is reported beside it).  The images are compared byte for byte.
  python profiles/image_bench.py [--families 200000] [--threads 16] [--out profiles/image_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mmm(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=200_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    from bsseqconsensusreads_amd import batch as B, hostplan, records as R, synth
    from bsseqconsensusreads_amd.device import Engine
    s = synth.generate("C2", a.families, seed=42, device="cuda", genome_len=20_000_000)
    eng = Engine(0)
    packed = R.pack_bases(s.raw)
    ph = B.plan_families(s.raw, "full", s.ref)
    pg = B.plan_families(packed, "full", s.ref)
    cap = B.route_small_cap(ph, 0, ph.n_fam)
    host, table = [], []
    for k in range(9):
        t0 = time.perf_counter()
        fh = hostplan.materialize(ph, 0, ph.n_fam, cap, n_threads=a.threads)
        t1 = time.perf_counter()
        fg = hostplan.materialize(pg, 0, pg.n_fam, cap, n_threads=a.threads, gather=True)
        t2 = time.perf_counter()
        if k >= 2:
            host.append((t1 - t0) * 1e3)
            table.append((t2 - t1) * 1e3)
    dev = eng.device
    raw_dev = eng.upload_raw(packed.raw_bases)
    tab = np.ascontiguousarray(fg.gather)
    tab_dev = torch.from_numpy(tab.view(np.uint8)).to(dev)
    seq = torch.empty(fg.n_slots // 2 + 64, dtype=torch.uint8, device=dev)
    qual = torch.empty(fg.n_slots + 64, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)
    ms = []
    for k in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        rc = eng.lib.bsdc_image_gather(eng.ctx, C.c_void_p(raw_dev.data_ptr()), int(raw_dev.numel()),
                                       C.c_void_p(tab_dev.data_ptr()), C.c_void_p(tab.ctypes.data), tab.shape[0],
                                       fg.n_slots, C.c_void_p(seq.data_ptr()), C.c_void_p(qual.data_ptr()),
                                       C.c_void_p(st.cuda_stream))
        assert rc == 0, eng.lib.bsdc_last_error(eng.ctx)
        e1.record(st)
        e1.synchronize()
        if k >= 2:
            ms.append(e0.elapsed_time(e1))
    same = bool(np.array_equal(seq[:fg.n_slots // 2].cpu().numpy(), fh.seq[:fg.n_slots // 2]) and
                np.array_equal(qual[:fg.n_slots].cpu().numpy(), fh.qual[:fg.n_slots]))
    res = {"families": a.families, "records": int(fg.n_rec), "n_slots": int(fg.n_slots), "bases": int(fg.n_bases),
           "raw_bytes": int(packed.raw_bases.shape[0]), "table_bytes": int(tab.nbytes), "host_threads": a.threads,
           "kernel_ms": mmm(ms), "host_materialize_with_images_ms": mmm(host),
           "host_materialize_table_only_ms": mmm(table), "images_identical": same,
           "kernel_GBps_written": round(1.5 * fg.n_slots / (statistics.median(ms) * 1e-3) / 1e9, 1)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh_:
            json.dump(res, fh_, indent=1)
            fh_.write("\n")
    eng.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

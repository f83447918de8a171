"""k_metrics alone on a 200k-family C2 batch's rows, beside the tagged vote step of the same batch
(DESIGN.md 8.10): two warm-ups, seven timed runs each, torch events on the stream that runs them.
The tagged vote is the one bench.py --full's tag leg times (bsdc_run with BSDC_MODE_TAGS on the
resident batch); this change leaves its kernels as they were.  Row bytes = what the kernel must read
once: for every emitted end its length in consensus qual bytes, half that in packed seq, and 2
(depth, err) rows a strand plus base and qual rows where both strands are present (molecular: 2).

    python profiles/metrics_bench.py [--families 200000] [--out profiles/metrics_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsseqconsensusreads_amd import batch as B, pipeline, synth  # noqa: E402
from bsseqconsensusreads_amd.device import Engine  # noqa: E402


def timed(fn, warm=2, runs=7):
    out = []
    for i in range(warm + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            out.append(e0.elapsed_time(e1))
    return {"min_ms": round(min(out), 4), "median_ms": round(float(np.median(out)), 4), "max_ms": round(max(out), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = synth.generate("C2", a.families, seed=7, device="cpu")
    eng = Engine(0)
    eng.load_reference(s.ref)
    fb = B.build_family_batch(s.raw, "full", s.ref)
    db = eng.upload(fb, tags=True)
    mode = pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE | pipeline.MODE_TAGS
    vote = timed(lambda: eng.run(db, mode))
    eng.metrics_begin(512)
    met = timed(lambda: eng.metrics(db))
    o = db.fetch()
    em = (o["status"] & 1) != 0
    L = o["len"][em].astype(np.int64)                       # [emitted, 2]
    sl = o["ss_len"][em]
    two = np.stack([(sl[:, 0] > 0) & (sl[:, 3] > 0), (sl[:, 1] > 0) & (sl[:, 2] > 0)], axis=1)
    row_bytes = int((L * (1 + 0.5 + 2 + two * 6)).sum())
    res = {"families": int(fb.n_fam), "emitted": int(em.sum()), "stride": int(db.stride), "row_bytes": row_bytes,
           "k_metrics": met, "tagged_vote": vote,
           "k_metrics_row_GBps_median": round(row_bytes / (met["median_ms"] / 1e3) / 1e9, 1),
           "k_metrics_over_tagged_vote_median": round(met["median_ms"] / vote["median_ms"], 4)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()

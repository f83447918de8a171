"""bsdc_toolrec_format alone on a 200k-family C2 batch, beside the tagged vote step of the same batch
(DESIGN.md 8.11): two warm-ups, three timed runs each, all reported, torch events on the stream that
runs them.  The tagged vote is bsdc_run with BSDC_MODE_TAGS | BSDC_MODE_DUMP on the resident batch;
the format call is timed as Engine.toolrec makes it (five launches, with the allocation of its
buffers and the upload of the batch's tables), as the bare call with the buffers kept (which still
holds the launcher's host pass over the table), and as its five kernels alone (kernels()).
Bytes = the records written (off[n_rec]).

    python profiles/toolrec_bench.py [--families 200000] [--out profiles/toolrec_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsseqconsensusreads_amd import batch as B, pipeline, synth, toolrec  # noqa: E402
from bsseqconsensusreads_amd.device import Engine  # noqa: E402


def timed(fn, warm=2, runs=3):
    out = []
    for i in range(warm + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            out.append(round(e0.elapsed_time(e1), 4))
    return {"runs_ms": out, "median_ms": round(float(np.median(out)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = synth.generate("C2", a.families, seed=7, device="cpu")
    eng = Engine(0)
    eng.load_reference(s.ref)
    fb = B.build_family_batch(s.raw, "full", s.ref)
    db = eng.upload(fb, tags=True, dump=True)
    mode = pipeline.MODE_CONVERT | pipeline.MODE_EXTEND | pipeline.MODE_VOTE | pipeline.MODE_TAGS | pipeline.MODE_DUMP
    vote = timed(lambda: eng.run(db, mode))
    t = toolrec.batch_tables(s.raw, fb)
    whole = timed(lambda: eng.toolrec(db, t))
    total = int(db.toolrec.foff[-1].item())
    # the launches alone: the tables and the buffers stay
    n, n_dump = db.n_rec, int(db.dump_seq.numel()) // 4 * 4
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8)).to(eng.device)  # noqa: E731
    d_tab, d_names, d_cig, d_aux = up(t.tab), up(t.names), up(t.cigar), up(t.aux)
    cap = t.bound(n_dump)
    rec = torch.empty(cap, dtype=torch.uint8, device=eng.device)
    off = torch.empty(n + 1, dtype=torch.int64, device=eng.device)
    tmp = torch.empty(int(eng.lib.bsdc_toolrec_tmp_bytes(n)), dtype=torch.uint8, device=eng.device)
    tab_h = np.ascontiguousarray(t.tab)

    def launches():
        st = torch.cuda.current_stream(eng.device)
        rc = eng.lib.bsdc_toolrec_format(C.byref(db._o), db.t["rec"].data_ptr(), n, n_dump, d_tab.data_ptr(),
                                         tab_h.ctypes.data, d_names.data_ptr(), t.names.shape[0], d_cig.data_ptr(),
                                         t.cigar.shape[0], d_aux.data_ptr(), t.aux.shape[0], off.data_ptr(), rec.data_ptr(),
                                         cap, tmp.data_ptr(), C.c_void_p(st.cuda_stream))
        assert rc == 0, eng.lib.bsdc_toolrec_last_error().decode()
    alone = timed(launches)
    assert int(off[-1].item()) == total

    # the five kernels without the launcher's host pass over the table: the stream is kept busy by
    # `ahead` vote launches while the host checks, the first event lies behind them and the second
    # behind the format's launches, so the interval holds the kernels alone -- as long as the host
    # is done enqueuing before the votes are (host_ms, taken with the clock, against ahead_ms)
    import time

    def kernels(ahead=40):
        out = []
        for i in range(5):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ea = torch.cuda.Event(enable_timing=True)
            ea.record()
            for _ in range(ahead):
                eng.run(db, mode)
            e0.record()
            t0 = time.perf_counter()
            launches()
            host_ms = (time.perf_counter() - t0) * 1e3
            e1.record()
            e1.synchronize()
            if i >= 2:
                out.append({"kernels_ms": round(e0.elapsed_time(e1), 4), "host_call_ms": round(host_ms, 4),
                            "ahead_ms": round(ea.elapsed_time(e0), 4)})
        return out
    kern = kernels()
    kmed = float(np.median([x["kernels_ms"] for x in kern]))
    res = {"families": int(fb.n_fam), "records": int(n), "record_bytes": total, "bound_bytes": int(cap),
           "toolrec_launches": alone, "toolrec_with_tables": whole, "tagged_vote_with_dump": vote,
           "toolrec_kernels": {"runs": kern, "median_ms": round(kmed, 4),
                               "host_hidden": all(x["host_call_ms"] < x["ahead_ms"] for x in kern)},
           "toolrec_call_GBps_median": round(total / (alone["median_ms"] / 1e3) / 1e9, 1),
           "toolrec_kernels_GBps_median": round(total / (kmed / 1e3) / 1e9, 1),
           "toolrec_kernels_over_tagged_vote_median": round(kmed / vote["median_ms"], 4),
           "toolrec_call_over_tagged_vote_median": round(alone["median_ms"] / vote["median_ms"], 4)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    eng.close()


if __name__ == "__main__":
    main()

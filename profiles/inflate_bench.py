"""GPU BGZF inflate throughput (libbsdc bsdc_bgzf_inflate, csrc/bsdc_inflate.hip) on the BGZF blocks
of a C2 step-5 input BAM: the kernel alone on device-resident blocks (HIP events; the whole file in
one launch, and in launches of one 8 MiB fill's blocks), and the host's libdeflate on the same
blocks at --threads threads.  With a library built with -DBSDC_INFLATE_PHASES at BSDC_LIB_PATH,
also lane 0's clock per phase (header + tables, symbol decode, copies).  Writes
profiles/inflate_bench.json.
Usage (GPU box): python profiles/inflate_bench.py [--families 1000000] [--threads 16]"""
import argparse
import concurrent.futures as cf
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=1_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=int, default=5)
    a = ap.parse_args()
    import torch

    from bsseqconsensusreads_amd import _lib as L
    from bsseqconsensusreads_amd import bam, synth
    from bsseqconsensusreads_amd import records as R
    from test_stream import _header
    s = synth.generate("C2", a.families, seed=5, device="cpu", genome_len=max(400_000, 40 * a.families))
    raw = R.take(s.raw, np.lexsort((s.raw.pos, s.raw.tid)))
    p = os.path.join(tempfile.mkdtemp(prefix="bsdc_inflb_"), "in.bam")
    bam.write_bam(p, _header(s.ref), bam.records_to_bam(raw), level=a.level, threads=a.threads)
    data = np.fromfile(p, np.uint8)
    blocks, o, dst = [], 0, 0
    while o < data.shape[0]:
        xlen = int(data[o + 10]) | int(data[o + 11]) << 8
        bsize = (int(data[o + 16]) | int(data[o + 17]) << 8) + 1
        isize = int.from_bytes(data[o + bsize - 4:o + bsize].tobytes(), "little")
        if isize:
            blocks.append((o + 12 + xlen, bsize - 12 - xlen - 8, isize, dst))
            dst += isize
        o += bsize
    nblk, n_out = len(blocks), dst
    d = (L.InflateBlockC * nblk)()
    for i, t in enumerate(blocks):
        d[i].src, d[i].clen, d[i].isize, d[i].dst = t
    lib = L.load()
    comp = torch.from_numpy(data).cuda()
    blk = torch.from_numpy(np.frombuffer(bytes(d), np.uint8).copy()).cuda()
    out = torch.empty(n_out, dtype=torch.uint8, device="cuda")
    status = torch.empty(nblk, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def launch(b0, nb):
        assert lib.bsdc_bgzf_inflate(comp.data_ptr(), data.shape[0], blk.data_ptr() + 24 * b0, nb, out.data_ptr(), n_out,
                                     status.data_ptr() + 4 * b0, st) == 0

    def timed(fn):
        ms = []
        for k in range(a.reps + 2):  # two warm-up runs
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= 2:
                ms.append(e0.elapsed_time(e1))
        return ms

    whole = timed(lambda: launch(0, nblk))
    assert int(status.abs().sum()) == 0
    # one 8 MiB fill's blocks per launch, as the streaming reader calls it
    per_fill = max(1, int(nblk * (8 << 20) / data.shape[0]))
    fills = timed(lambda: [launch(b0, min(per_fill, nblk - b0)) for b0 in range(0, nblk, per_fill)])
    got = out.cpu().numpy()
    # the host: libdeflate, one decompressor per thread, the same blocks
    ld = C.CDLL("libdeflate.so.0")
    ld.libdeflate_alloc_decompressor.restype = C.c_void_p
    ld.libdeflate_deflate_decompress.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    host = np.empty(n_out, np.uint8)
    parts = [blocks[k::a.threads] for k in range(a.threads)]
    decs = [ld.libdeflate_alloc_decompressor() for _ in parts]

    def work(k):
        for src, clen, isize, to in parts[k]:
            assert ld.libdeflate_deflate_decompress(decs[k], data.ctypes.data + src, clen, host.ctypes.data + to, isize,
                                                    None) == 0
    hs = []
    with cf.ThreadPoolExecutor(a.threads) as ex:
        for k in range(a.reps + 2):
            t0 = time.perf_counter()
            list(ex.map(work, range(a.threads)))
            if k >= 2:
                hs.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(host, got), "the kernel's bytes differ from libdeflate's"
    gbs = lambda ms: round(n_out / ms / 1e6, 2)  # noqa: E731
    res = {"families": a.families, "blocks": nblk, "bytes_in": int(data.shape[0]), "bytes_out": n_out,
           "blocks_in_flight": min(nblk, 2 * torch.cuda.get_device_properties(0).multi_processor_count),
           "kernel_ms": spread(whole), "kernel_GBps_out": gbs(statistics.median(whole)),
           "blocks_per_fill": per_fill, "per_fill_launches_ms": spread(fills),
           "per_fill_GBps_out": gbs(statistics.median(fills)),
           "host_threads": a.threads, "host_ms": spread(hs), "host_GBps_out": gbs(statistics.median(hs)),
           "kernel_over_host": round(statistics.median(hs) / statistics.median(whole), 3)}
    if hasattr(lib, "bsdc_inflate_phases"):  # a -DBSDC_INFLATE_PHASES build: lane 0's 100 MHz clock per block
        launch(0, min(nblk, 8192))
        torch.cuda.synchronize()
        ph = np.zeros(4 * min(nblk, 8192), np.uint64)
        assert lib.bsdc_inflate_phases(C.c_void_p(ph.ctypes.data), C.c_int64(ph.shape[0])) == 0
        ph = ph.reshape(-1, 4)[:, :3].astype(np.float64).sum(0)
        res["phase_share"] = dict(zip(("header_tables", "decode", "copies"), [round(float(x / ph.sum()), 3) for x in ph]))
    print(json.dumps(res, indent=1))
    with open(os.path.join(ROOT, "profiles", "inflate_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

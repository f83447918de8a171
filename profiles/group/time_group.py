"""Times of cli group's pieces: run from the repository root on one MI355X,
    python profiles/group/time_group.py > profiles/group/time_group.log
Wall times around each call with the device synchronised: 3 warm-up runs, 10 timed, median (min .. max).
bsdc_group_assign reads three counts back, so its time includes those round trips."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import group_inputs as GI  # noqa: E402
from bsseqconsensusreads_amd import bam, bgzf, group, zipper  # noqa: E402


def timed(fn, warm=3, runs=10):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return "%.2f ms (%.2f .. %.2f)" % (float(np.median(t)), min(t), max(t))


def fabricated(n, seed=3):
    """n templates: position groups of Poisson(4) + 1 templates, molecules of about 3, 1% UMI errors"""
    rng = np.random.default_rng(seed)
    g = np.repeat(np.arange(n // 4 + 1), rng.poisson(4, n // 4 + 1) + 1)[:n]
    k0 = (rng.integers(1, 1 << 28, g.max() + 1, dtype=np.uint64)[g] << np.uint64(1))
    k1 = k0 + np.uint64(400)
    m = np.arange(n) // 3
    base = rng.integers(0, 1 << 24, m.max() + 1, dtype=np.uint64)[m]
    umi = (base >> np.uint64(12)) << np.uint64(32) | (base & np.uint64(0xfff))
    flip = rng.random(n) < 0.12  # (12 bases at 1%)
    umi = umi ^ np.where(flip, np.uint64(1) << (rng.integers(0, 6, n).astype(np.uint64) * np.uint64(2)), np.uint64(0))
    p = rng.permutation(n)
    return k0[p], k1[p], umi[p], rng.integers(0, 2, n).astype(np.uint8)


def main():
    torch.set_num_threads(16)
    print("device:", torch.cuda.get_device_name(0))
    recs = GI.sweep()
    data = b"".join(recs)
    buf = zipper._aligned_copy(data)
    a = zipper.Records(None, buf, len(data), zipper.scan(buf, len(data)))
    t0 = time.perf_counter()
    t = group.templates(a)
    print("sweep: %d records, %d templates; host join, filters, keys: %.1f ms" % (a.n, t.n, (time.perf_counter() - t0) * 1e3))
    tab = group.rec_table(a, t)
    dev = {}

    def assign():
        dev["r"] = group.assign_device(0, t.k0, t.k1, t.umi, t.strand, 1, t.kmax)
    print("sweep bsdc_group_assign (with upload):", timed(assign))
    print("sweep bsdc_group_format (with upload):", timed(lambda: group.format_device(dev["r"][2], dev["r"][0], dev["r"][1], tab, a.buf)))
    host = {}

    def assign_h():
        host["r"] = group.assign_host(t.k0, t.k1, t.umi, t.strand, 1, t.kmax)
    print("sweep bsdc_group_assign_host:", timed(assign_h))
    print("sweep bsdc_group_format_host:", timed(lambda: group.format_host(host["r"][2], host["r"][0], host["r"][1], tab, a.buf)))
    with tempfile.TemporaryDirectory() as d:
        h = bam.BamHeader(GI.HEADER, [x for x, _ in GI.REFS], np.asarray([x for _, x in GI.REFS], np.int64))
        w = bgzf.BamWriter(os.path.join(d, "in.bam"), h, 1)
        w.add_raw(data, 16)
        w.close(16)
        print("sweep group() whole call, device:", timed(lambda: group.group(os.path.join(d, "in.bam"), os.path.join(d, "o.bam"), threads=16), 1, 5))
        print("sweep group() whole call, host twins (16 threads):",
              timed(lambda: group.group(os.path.join(d, "in.bam"), os.path.join(d, "h.bam"), threads=16, host=True), 1, 5))
    k0, k1, umi, strand = fabricated(1_000_000)
    stats = group.assign_device(0, k0, k1, umi, strand)[3]
    print("1M fabricated templates: %s groups, %s nodes, %s molecules, most nodes %s" % tuple(stats.tolist()))
    print("1M bsdc_group_assign (with upload):", timed(lambda: group.assign_device(0, k0, k1, umi, strand), 2, 5))
    print("1M bsdc_group_assign_host:", timed(lambda: group.assign_host(k0, k1, umi, strand), 1, 3))


if __name__ == "__main__":
    main()

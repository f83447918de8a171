"""bench.py --dump-outputs on the GPU: dump_outputs reads the device buffers a step left, checked
against DeviceBatch.fetch() of the same batch -- a small C4 batch (skewed sizes: small and large
families), every family, valid positions only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from bsseqconsensusreads_amd.bam import unpack_nibbles  # noqa: E402


@pytest.mark.gpu
def test_dump_outputs_equals_fetch(engine, tmp_path):
    args = bench.parse(["--config", "C4", "--families", "5000"])
    res, _ = bench.build(args, 0, engine.device, engine)
    assert len(res) == 1 and res[0].n_large > 0 and res[0].small.size > 0
    for _ in range(2):  # the buffers hold the last step's consensus
        engine.run(res[0].db, bench.FULL_MODE)
    torch.cuda.synchronize()
    shapes = bench.dump_outputs(res, str(tmp_path), args.seed)
    A = {k: np.load(str(tmp_path / (k + ".npy"))) for k in shapes}
    o = res[0].db.fetch()
    F, s = res[0].n_fam, o["stride"]
    fa, fs = A["family"].astype(np.int64), A["sample_family"].astype(np.int64)
    assert np.array_equal(fa, np.arange(F)) and np.array_equal(fs, np.arange(F))  # all of them fit the budget
    emitted = (o["status"] & 1) != 0
    assert emitted.any()
    seq = unpack_nibbles(o["seq"]).astype(np.int64)
    qual = o["qual"].astype(np.int64)
    ok = (np.arange(s)[None, None, :] < o["len"][:, :, None]) & emitted[:, None, None]
    assert np.array_equal(A["status"], o["status"].astype(np.float32))
    assert np.array_equal(A["length"], o["len"].astype(np.float32))
    assert np.array_equal(A["seq"], (seq * ok).astype(np.float32))
    assert np.array_equal(A["qual"], (qual * ok).astype(np.float32))
    assert np.array_equal(A["checksum"], ((qual + 256 * seq) * (np.arange(s) + 1) * ok).sum(-1).astype(np.float64))
    assert A["checksum"].max() > 0

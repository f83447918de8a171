"""bench.py --dump-outputs on the CPU: dump_outputs over stand-in resident batches (host tensors in
the device layout) against a per-family numpy statement -- valid positions only, float32 / float64,
inside the byte budget, the family sample seeded (the same from call to call).  And bench.run's
order of work with the device taken out: a plain run launches its warm-up and timed steps and
nothing else; --dump-outputs writes after the last timed step and before the --full legs."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _batch(rng, F, s):
    db = types.SimpleNamespace(stride=s)
    db.status = torch.from_numpy(rng.integers(0, 8, F, dtype=np.uint8))
    db.len = torch.from_numpy(rng.integers(0, s + 1, 2 * F).astype(np.uint16).view(np.int16))
    db.seq = torch.from_numpy(rng.integers(0, 256, F * s, dtype=np.uint8))       # junk past the lengths too
    db.qual = torch.from_numpy(rng.integers(0, 94, 2 * F * s, dtype=np.uint8))
    return types.SimpleNamespace(db=db, n_fam=F)


def _family(res, g):
    """-> (status, length [2], base [2, s], qual [2, s], checksum [2]) of family g, invalid positions 0."""
    k = 0
    while g >= res[k].n_fam:
        g -= res[k].n_fam
        k += 1
    db, F, s = res[k].db, res[k].n_fam, res[k].db.stride
    st = int(db.status[g])
    ln = db.len.numpy().view(np.uint16).reshape(F, 2)[g].astype(np.int64)
    p = db.seq.numpy().reshape(F, 2, s // 2)[g]
    b = np.stack((p >> 4, p & 15), -1).reshape(2, s).astype(np.int64)  # high nibble first
    q = db.qual.numpy().reshape(F, 2, s)[g].astype(np.int64)
    ok = (np.arange(s)[None, :] < ln[:, None]) & bool(st & 1)
    return st, ln, b * ok, q * ok, ((q + 256 * b) * (np.arange(s) + 1) * ok).sum(-1)


def test_dump_outputs_matches_numpy_statement(tmp_path, monkeypatch):
    rng = np.random.default_rng(5)
    res = [_batch(rng, 700, 160), _batch(rng, 333, 176)]  # two batches, the second one wider
    total, S = 1033, 176
    whole = bench.DUMP_BUDGET
    for budget in (whole, 200_000, 30_000):  # everything; sampled bases; both sampled
        monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
        d = str(tmp_path / str(budget))
        shapes = bench.dump_outputs(res, d, 42)
        A = {k: np.load(os.path.join(d, k + ".npy")) for k in shapes}
        assert sorted(A) == ["checksum", "family", "length", "qual", "sample_family", "seq", "status"]
        assert sum(a.nbytes for a in A.values()) <= budget
        assert all(A[k].dtype == (np.float64 if k in ("family", "sample_family", "checksum") else np.float32) for k in A)
        fa, fs = A["family"].astype(np.int64), A["sample_family"].astype(np.int64)
        assert (fa.size == total) == (budget >= 200_000) and (fs.size == total) == (budget == whole)
        for f in (fa, fs):
            assert 0 < f.size <= total and (np.diff(f) > 0).all() and f[0] >= 0 and f[-1] < total
        assert A["seq"].shape == A["qual"].shape == (fs.size, 2, S)
        for i, g in enumerate(fa):
            st, ln, _, _, cs = _family(res, g)
            assert A["status"][i] == st and (A["length"][i] == ln).all() and (A["checksum"][i] == cs).all(), g
        for i, g in enumerate(fs):
            _, _, b, q, _ = _family(res, g)
            s = b.shape[1]
            assert (A["seq"][i, :, :s] == b).all() and (A["qual"][i, :, :s] == q).all(), g
            assert not A["seq"][i, :, s:].any() and not A["qual"][i, :, s:].any()
        again = bench.dump_outputs(res, str(tmp_path / "again"), 42)
        assert again == shapes
        for k in A:
            assert np.array_equal(A[k], np.load(str(tmp_path / "again" / (k + ".npy")))), k


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def _run_on_stand_ins(monkeypatch, capsys, argv):
    """bench.run with the device taken out: stand-in batches and engine, host tensors, no-op stream
    and events -> (the ordered log of engine runs / the dump / the --full legs, the result line)."""
    import json

    from bsseqconsensusreads_amd import device, shard

    log = []
    rng = np.random.default_rng(9)
    res = []
    for F in (40, 25):
        r = _batch(rng, F, 160)
        r.db.fetch_lengths = lambda db=r.db, F=F: (db.status.numpy(), db.len.numpy().view(np.uint16).astype(np.int32).reshape(F, 2))
        r.molecules, r.n_rec, r.n_bases, r.small, r.n_large = F, 3 * F, 450 * F, np.arange(F), 0
        res.append(r)

    class Engine:
        def __init__(self, index):
            pass

        def run(self, db, mode, stream):
            log.append(("run", mode))

        def close(self):
            pass

    class Event:
        def __init__(self, enable_timing=False):
            pass

        def record(self, stream):
            pass

        def elapsed_time(self, other):
            return 1.0

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(device, "Engine", Engine)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: None)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    reduce0 = shard.reduce_step
    monkeypatch.setattr(shard, "reduce_step", lambda dist, t, c, dev: reduce0(dist, t, c, torch.device("cpu")))
    monkeypatch.setattr(bench, "build", lambda args, rank, dev, eng: (res, None))
    dump0 = bench.dump_outputs
    monkeypatch.setattr(bench, "dump_outputs", lambda *a: (log.append(("dump",)), dump0(*a))[1])
    legs = {"roofline": {"kernel": "k_small"}, "cpu_baseline": None, "tags_ms_per_step": 1.0, "tags_roofline": None,
            "tags_families_per_s": None}
    monkeypatch.setattr(bench, "full_legs", lambda *a: (log.append(("full",)), legs)[1])
    bench.run(bench.parse(argv))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return log, json.loads(lines[0])


def test_plain_run_times_its_steps_and_nothing_else(monkeypatch, capsys):
    log, d = _run_on_stand_ins(monkeypatch, capsys, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert log == [("run", bench.FULL_MODE)] * ((7 + 2) * 2)  # every step runs both batches; no dump, no --full leg
    assert d["steps"] == 7 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["full"] is False
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 65) <= 65 * 1e-2  # families a step / its time (rounded)
    assert d["unit"] == "families/s" and d["higher_is_better"] is True and d["metric"] == bench.METRIC
    assert d["dumped"] is None
    for k in ("roofline", "cpu_baseline", "tags_ms_per_step", "tags_roofline", "tags_families_per_s"):
        assert d[k] is None, k


def test_full_run_dumps_the_last_timed_step_before_its_legs(monkeypatch, capsys, tmp_path):
    out = str(tmp_path / "dump")
    log, d = _run_on_stand_ins(monkeypatch, capsys, ["--steps", "3", "--warmup", "1", "--full", "--dump-outputs", out])
    assert log == [("run", bench.FULL_MODE)] * ((3 + 1) * 2) + [("dump",), ("full",)]
    assert d["full"] is True and d["roofline"] == {"kernel": "k_small"} and d["tags_ms_per_step"] == 1.0
    assert sorted(d["dumped"]) == ["checksum", "family", "length", "qual", "sample_family", "seq", "status"]
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in d["dumped"])
    assert np.load(os.path.join(out, "status.npy")).shape == (65,)

"""The host side of the device BAM record path, no GPU: the fabricated inputs hold their edges, the
size helpers and argument checks of libbsdc's bsdc_bam_format (which touch no device), the CLI's and
the stream's refusals, and bam.family_aux against the aux bytes of duplex_records' records."""
import ctypes as C

import numpy as np
import pytest

from bsseqconsensusreads_amd import _lib, bam
import bamrec_inputs as BI


@pytest.mark.parametrize("stride", [16, 32, 528])
def test_inputs_hold_their_edges(stride):
    x = BI.make(stride, 300, seed=stride)
    keep = x.kept(True)
    L = x.length[keep].reshape(-1)
    assert set(BI.SPECIAL_LEN(stride)) <= set(L.tolist()) and (L % 2 == 1).any() and int(L.max()) == stride - 2
    assert set(np.diff(x.names.off).tolist()) >= set(range(1, 254)) and int(np.diff(x.names.off).max()) == 253
    al = np.diff(x.aux.off)
    assert al.min() == 0 and any(b"RXZ" in x.aux[int(f)] for f in np.nonzero(keep)[0])
    assert any(b"RXZ" not in x.aux[int(f)] and len(x.aux[int(f)]) for f in np.nonzero(keep)[0])
    codes, quals = set(), set()
    for f in np.nonzero(keep)[0]:
        for d in range(2):
            n = int(x.length[f, d])
            row = np.stack([x.seq[f, d] >> 4, x.seq[f, d] & 15], -1).reshape(-1)[:n]
            codes |= set(row.tolist())
            quals |= set(x.qual[f, d, :n].tolist())
    assert codes == set(range(16)) and quals == set(range(256))
    sl = x.ss_len[keep] > 0
    assert (sl[:, 0] & ~sl[:, 3]).any() and (~sl[:, 0] & sl[:, 3]).any() and (sl[:, 0] & sl[:, 3]).any()
    n = x.notes
    assert {"no_depth", "d255", "d255_min", "d256_m255", "d256_m256", "one_strand_255", "one_strand_256", "wide_max",
            "disagree"} <= set(n) and all(keep[f] for f in n.values())
    d = x.depth16()
    Lf = int(x.length[n["no_depth"], 0])
    assert d[n["no_depth"]].max() == 0 and Lf > 0
    assert (d[n["d255"], :2, :Lf] == 255).all() and (d[n["d255"], 0, :Lf] + d[n["d255"], 3, :Lf] == 256).all()
    f = n["d255_min"]
    assert (d[f, 0, :Lf] + d[f, 3, :Lf]).max() == 255 and (d[f, 0, :Lf] + d[f, 3, :Lf]).min() < 255
    assert d[n["d256_m255"], 0, :Lf].max() == 256 and d[n["d256_m255"], 0, :Lf].min() == 255
    assert d[n["d256_m256"], :, :Lf].min() == 256 == d[n["d256_m256"], :, :Lf].max()
    assert d[n["one_strand_255"], 0, :Lf].max() == 255 and not x.ss_len[n["one_strand_255"], 2:].any()
    assert d[n["one_strand_256"], 2, :Lf].max() == 256 and d[n["one_strand_256"], 2, :Lf].min() == 255
    assert not x.ss_len[n["one_strand_256"], :2].any()
    f = n["wide_max"]
    assert x.ss_wide[f] >= 0 and (d[f, 0, :Lf] + d[f, 3, :Lf]).max() == 65534
    f = n["disagree"]
    a, b = x.ss_base[f, 0, :Lf] & 15, x.ss_base[f, 3, :Lf] & 15
    eq = x.ss_qual[f, 0, :Lf] == x.ss_qual[f, 3, :Lf]
    assert (a != b).all() and eq.any() and (~eq).any()
    # garbage past the lengths; unwritten families in front, at the end and in runs; a filtered-out one
    assert (x.ss_depth[keep][:, :, -1] != 0).any() and (x.seq[keep][:, :, -1] != 0).any()
    assert not keep[0] and not keep[-1] and not keep[40:57].any() and ((x.status & 1 != 0) & (x.filt != 0)).any()


@pytest.mark.parametrize("stride", [16, 32, 528])
def test_bytes_bound_and_scratch_size(stride, tmp_path):
    lib = _lib.load()
    x = BI.make(stride, 120, seed=stride)
    for molecular in (False, True):
        for tags in (False, True):
            data, off = BI.expected(x, molecular, tags, False, str(tmp_path))
            bound = lib.bsdc_bam_bytes_bound(x.n_fam, int(x.names.off[-1]), int(x.aux.off[-1]), stride, int(molecular),
                                             int(tags))
            assert len(data) == int(off[-1]) <= bound
    assert lib.bsdc_bam_bytes_bound(-1, 0, 0, 16, 0, 1) < 0 and lib.bsdc_bam_bytes_bound(1, -1, 0, 16, 0, 1) < 0
    assert lib.bsdc_bam_bytes_bound(1, 0, -1, 16, 0, 1) < 0 and lib.bsdc_bam_bytes_bound(1, 0, 0, -16, 0, 1) < 0
    assert lib.bsdc_bam_bytes_bound(1, 0, 0, 16, 2, 1) < 0 and lib.bsdc_bam_bytes_bound(1, 0, 0, 16, -1, 0) < 0
    assert lib.bsdc_bam_bytes_bound(0, 0, 0, 16, 0, 1) == 0
    # the scan's sums (a workgroup per 1024 families) and 12 dwords a record
    for n in (0, 1, 1025, 1_700_000):
        assert lib.bsdc_bam_tmp_bytes(n) >= 8 * ((n + 1023) // 1024 + 1) + 2 * n * 40
    assert lib.bsdc_bam_tmp_bytes(-1) < 0


def test_abi_and_refusals_without_a_device():
    """every refusal returns -22 before any device is touched (this test runs without one)"""
    lib = _lib.load()
    assert lib.bsdc_abi_version() == 19
    F = 3
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)  # (never dereferenced: the checks come first)
    no = np.asarray([0, 3, 6, 9], np.int64)
    hp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def out(**kw):
        o = _lib.ConsensusC()
        o.stride = 16
        for k in ("status", "len", "seq", "qual", "ss_len", "ss_base", "ss_qual", "ss_depth", "ss_err"):
            setattr(o, k, buf.ctypes.data)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(o=None, kind=0, tags=1, n=F, noff=no, aoff=no, cap=100, skip=None):
        a = [C.byref(o if o is not None else out()), None, kind, tags, n, p, p, hp(noff), p, p, hp(aoff), p, p, cap, p,
             None]
        if skip is not None:
            a[skip] = None
        return lib.bsdc_bam_format(*a)

    assert lib.bsdc_bam_format(None, None, 0, 0, 0, None, None, None, None, None, None, None, None, 0, None, None) == -22
    for skip in (0, 5, 6, 7, 8, 9, 10, 11, 12, 14):  # a NULL pointer (filt apart)
        assert call(skip=skip) == -22, skip
    for k in ("status", "len", "seq", "qual"):
        assert call(out(**{k: None}), tags=0) == -22, k
    for k in ("ss_len", "ss_base", "ss_qual", "ss_depth", "ss_err"):  # with_tags with out->ss_* NULL
        assert call(out(**{k: None})) == -22, k
    assert call(n=-1) == -22 and call(cap=-1) == -22  # a negative count or cap
    assert call(kind=2) == -22 and call(kind=-1) == -22
    assert call(noff=np.asarray([0, 3, 2, 9], np.int64)) == -22  # offsets that go backwards
    assert call(aoff=np.asarray([0, 3, 2, 9], np.int64)) == -22
    assert call(noff=np.asarray([0, 254, 255, 256], np.int64)) == -22  # a name over 253 bytes
    assert call(out(stride=0)) == -22 and call(out(stride=24)) == -22


STEP5 = ["step5", "-r", "g.fa", "in.bam"]


@pytest.mark.parametrize("argv,word", [
    (STEP5 + ["-", "--fastq1", "a", "--fastq2", "b", "--gpu-bam", "true"], "'-'"),
    (STEP5 + ["out.bam", "--gpu-bam", "true", "--gpus", "2"], "--gpus 2"),
    (STEP5 + ["out.bam", "--gpu-bam", "true", "--stream", "false"], "--stream false"),
    (["molecular", "in.bam", "out.bam", "--gpu-bam", "true", "--stream", "false"], "--stream false"),
    (["molecular", "in.bam", "-", "--fastq1", "a", "--fastq2", "b", "--gpu-bam", "true"], "'-'"),
])
def test_cli_refuses_gpu_bam(capsys, argv, word):
    from bsseqconsensusreads_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--gpu-bam" in err and word in err, err


def test_cli_accepts_gpu_bam():
    from bsseqconsensusreads_amd import cli
    a = cli.parse(STEP5 + ["out.bam", "--gpu-bam", "true", "--filter-min-base-quality", "20", "--filter-min-reads", "2",
                           "1", "1", "--output-per-base-tags", "false", "--gpu-inflate", "true"])
    assert a.gpu_bam == "true" and cli.filter_params(a).min_reads == (2, 1, 1)
    a = cli.parse(STEP5 + ["out.bam", "--fastq1", "a", "--fastq2", "b", "--gpu-bam", "true", "--gpu-fastq", "true"])
    assert a.gpu_bam == "true" and a.gpu_fastq == "true"
    assert cli.parse(["molecular", "in.bam", "o.bam", "--gpu-bam", "true"]).gpu_bam == "true"
    assert cli.parse(STEP5 + ["out.bam"]).gpu_bam == "false"


def test_cli_refuses_an_unsorted_input_that_would_be_read_whole(tmp_path, monkeypatch, capsys):
    """step5 --gpu-bam true on an input without SO:coordinate: a ValueError by name, exit 1, before any work"""
    from bsseqconsensusreads_amd import cli, device

    class NoEngine:
        def __init__(self, *a):
            pass

        def close(self):
            pass
    monkeypatch.setattr(device, "Engine", NoEngine)
    monkeypatch.setattr(cli, "_coordinate_sorted", lambda bam_, path: False)
    assert cli.main(STEP5 + [str(tmp_path / "o.bam"), "--gpu-bam", "true"]) == 1
    err = capsys.readouterr().err
    assert "ValueError" in err and "--gpu-bam" in err and "read whole" in err


def test_stream_refuses_gpu_bam_without_its_needs(tmp_path):
    """the Python surface: no output BAM, and a runner stream"""
    from bsseqconsensusreads_amd import stream
    job = stream.StreamJob("in.bam", "g.fa", None, ("a", "b"), gpu_bam=True)
    with pytest.raises(ValueError, match="gpu_bam"):
        stream.run(job, engine=object())
    job = stream.StreamJob("in.bam", "g.fa", str(tmp_path / "o.bam"), gpu_bam=True)
    with pytest.raises(ValueError, match="gpu_bam"):
        stream.run(job, runner=object())
    assert stream.StreamJob("a", "b", "c").gpu_bam is False


def test_family_aux_equals_the_records_aux():
    """bam.family_aux for every family == the aux bytes of duplex_records' records, on a small C2
    input with RX tags (the oracle's consensus stands in for the vote: no GPU)."""
    from bsseqconsensusreads_amd import pipeline, synth
    from bsseqconsensusreads_amd.batch import plan_families, materialize
    s = synth.generate("C2", 200, seed=11, device="cpu", genome_len=100_000)
    raw = s.raw
    rng = np.random.default_rng(4)
    umis = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 6)]) for _ in range(int(raw.mi_id.max()) + 1)]
    aux = []
    for k in range(raw.n):
        u = umis[int(raw.mi_id[k])] if raw.mi_id[k] >= 0 else b"NNNNNN"
        pair = u + b"-" + u[::-1] if raw.mi_strand[k] == 0 else u[::-1] + b"-" + u
        aux.append(b"RXZ" + pair + b"\0" if k % 11 else b"")
    raw.aux = aux
    plan = plan_families(raw, "full", s.ref)
    fb = materialize(plan, 0, plan.n_fam)
    F = fb.n_fam
    status = np.ones(F, np.uint8)
    status[::5] = 0
    cons = pipeline.Consensus(fb.fam_mi.copy(), status, np.full((F, 2), 3, np.int32), np.ones((F, 2, 16), np.uint8),
                              np.ones((F, 2, 16), np.uint8), fb.fam_off.astype(np.int64), fb.src.astype(np.int64))
    recs = bam.duplex_records(cons, raw, "p")
    table = bam.family_aux(fb.fam_off, fb.src, fb.fam_mi, raw)
    assert len(table) == F
    em = np.nonzero(status & 1)[0]
    assert recs.n == 2 * em.shape[0] and any(b"RXZ" in recs.aux[2 * k] for k in range(em.shape[0]))
    for k, f in enumerate(em):
        assert recs.aux[2 * k] == recs.aux[2 * k + 1] == table[int(f)], f
        assert table[int(f)].startswith(b"RGZA\0MIZ")

"""The family-image gather on the host (no GPU): bsdc_image_gather_host, the twin that shares the
kernel's per-dword function (csrc/bsdc_image.hip), against hostplan.materialize + split_hbm_bucket
byte for byte over all n_slots; the decode without unpacked bases; the plan on either record form;
the option's parsing and refusals; the twin under the sanitizers as a stand-alone program."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import image_inputs as I
from bsseqconsensusreads_amd import _lib, bam, batch as B, cli, records as R, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", I.CASE_NAMES)
def test_twin_equals_host_images(name):
    c, packed, fh, fg = I.built(name)
    assert fg.seq is None and fg.qual is None and fg.gather is not None and fh.gather is None
    assert fg.n_slots == fh.n_slots and fg.n_rec == fh.n_rec > 0
    for k in ("fam_off", "rec_off", "rec_pos", "rec_lenflag", "rec_link", "rec_win", "cig_off", "cig_info", "cigar", "rt",
              "fam_entry", "src", "split_parts", "split_part_recs", "split_fams"):
        assert np.array_equal(getattr(fg, k), getattr(fh, k)), k
    assert np.array_equal(fg.gather["slot"], fh.rec_off)  # (taken after the cut)
    assert set(np.unique(fg.gather["src"] % 4)) == {0, 1, 2, 3}
    if c.part_cap is not None:
        cut = set(int(x) for x in fh.split_fams[:, 0])
        assert cut and (name != "split_mixed" or len(cut) < fh.n_fam)  # mixed: one family cut, one left whole
    rc, seq, qual, msg = I.twin(packed.raw_bases, fg.gather, fg.n_slots)
    assert rc == 0, msg
    assert np.array_equal(qual, fh.qual[:fh.n_slots])
    assert np.array_equal(seq, fh.seq[:fh.n_slots // 2])
    assert "seq" not in fg.device_arrays() and "qual" not in fg.device_arrays()


def test_cases_hold_their_edges():
    L = {int(x) for n in I.CASE_NAMES for x in (I.built(n)[2].rec_lenflag & 0xFFFF)}
    assert {1, 2, 7, 8, 9, 15, 16, 17, 30, 31}.issubset(L)
    for st in (32, 33):
        assert I.built("stride%d" % st)[2].max_len + 2 == st
    sizes = np.diff(I.built("sizes")[2].fam_off.astype(np.int64))
    assert 1 in sizes and 520 in sizes
    _, packed, _, fg = I.built("clips")
    assert {0, 1, 2, 3}.issubset(set(int(x) for x in fg.gather["skip"]))
    assert ((fg.gather["skip"] + fg.gather["len"]) < fg.gather["l_seq"]).any()  # trailing clips
    assert {0, 1} == set(int(x) & 1 for x in fg.gather["l_seq"])
    q = set()
    for n in ("lengths", "wild"):
        q |= set(int(x) for x in np.unique(I.built(n)[2].qual))
    assert {0, 93, 127, 128, 255}.issubset(q)


def test_twin_equals_plain_statement():
    """What no plan produces: a kept length of 0, a first slot past 0, every skip parity."""
    rb, table, n_slots = I.table_case()
    assert (table["len"] == 0).any() and table["slot"][0] > 0
    assert {(int(s) & 1, int(l) & 1) for s, l in zip(table["skip"], table["l_seq"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert (table["slot"] % 8 == 4).any()  # records that share a dword of the packed image with a neighbour
    rc, seq, qual, msg = I.twin(rb, table, n_slots)
    assert rc == 0, msg
    es, eq = I.images_py(rb, table, n_slots)
    assert np.array_equal(seq, es) and np.array_equal(qual, eq)


def test_twin_refuses_bad_tables():
    rb, table, n_slots = I.table_case()
    for what, t in I.bad_tables(rb, table, n_slots):
        rc, seq, qual, msg = I.twin(rb, t, n_slots)
        assert rc == -22 and what in msg, (what, rc, msg)
        assert (seq == 0xA5).all() and (qual == 0xA5).all()  # refused before anything is written
    rc, _, _, msg = I.twin(rb, table, n_slots + 4)
    assert rc == -22 and "n_slots" in msg


def test_exports_and_abi():
    lib = _lib.load()
    assert lib.bsdc_abi_version() == 19
    for k in ("bsdc_image_gather", "bsdc_image_gather_host"):
        assert k in _lib.EXPORTS and hasattr(lib, k)
    assert np.dtype(_lib.IMAGE_REC).itemsize == 24


@pytest.fixture(scope="module")
def bam_file(tmp_path_factory):
    s = synth.generate("C2", 300, seed=11, device="cpu", genome_len=100_000)
    raw = synth.messify(s.raw, frac=0.1, seed=3)
    raw = R.take(raw, np.lexsort((raw.pos, raw.tid)))  # coordinate-sorted, as the step-5 input is
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in
                                                    zip(s.ref.names, s.ref.lengths)) + "@RG\tID:rg1\tSM:s1\tLB:libA\n"
    p = str(tmp_path_factory.mktemp("img") / "in.bam")
    bam.write_bam(p, bam.BamHeader(text, list(s.ref.names), np.asarray(s.ref.lengths, np.int64)),
                  bam.records_to_bam(raw), level=1, threads=2)
    return p, s.ref


def _stream_decode(path, packed):
    out = []
    for ch in bam.stream_chunks(path, 2, 40_000, 2000):
        out.append(ch.decode(2, packed=packed)[1])
    return out


def test_decode_without_unpacked_bases(bam_file):
    path, _ = bam_file
    a, b = _stream_decode(path, False), _stream_decode(path, True)
    assert len(a) == len(b) > 1
    for x, y in zip(a, b):
        assert y.seq is None and y.qual is None
        for k in ("flag", "tid", "pos", "mapq", "l_seq", "seq_off", "cig_off", "n_cig", "cigar", "next_tid", "next_pos",
                  "tlen", "name_id", "mi_id", "mi_strand", "mc_off", "mc_n", "mc_cigar", "la_tag", "rd_tag"):
            assert np.array_equal(getattr(x, k), getattr(y, k)), k
        assert np.array_equal(x.names.buf, y.names.buf) and np.array_equal(x.aux.buf, y.aux.buf)
        u = R.unpack_bases(y)
        assert np.array_equal(u.seq, x.seq) and np.array_equal(u.qual, x.qual)
        for k in (0, x.n // 2, x.n - 1):
            assert np.array_equal(y.record_seq(k), x.record_seq(k)) and np.array_equal(y.record_qual(k), x.record_qual(k))
        l = x.l_seq.astype(np.int64)
        assert np.array_equal(np.diff(y.seq_src), (l + 1) // 2 + l) and y.raw_bases.shape[0] == y.seq_src[-1]


@pytest.mark.parametrize("native", [True, False])
def test_plan_identical_on_either_form(native, monkeypatch):
    """predict_rd reads one base a converted record: from seq, or from the packed SEQ field."""
    s = synth.generate("C2", 400, seed=19, device="cpu", genome_len=60_000)
    raw = synth.messify(s.raw, frac=0.2, seed=5)
    monkeypatch.setenv("BSDC_HOST_PLAN", "native" if native else "numpy")
    pa = B.plan_families(raw, "full", s.ref)
    pb = B.plan_families(R.pack_bases(raw, 1, 1), "full", s.ref)
    assert pa.conv.any() and (raw.flag[pa.conv] & 16).any()  # converted reverse reads
    for k in ("order", "fam_off", "fam_mi", "t2_rank", "conv", "ext_right", "ext_left", "partner_raw", "rd_in", "sL", "L",
              "kfirst", "kn", "fam_split"):
        assert np.array_equal(getattr(pa, k), getattr(pb, k)), k
    sel = np.nonzero(pa.conv)[0]
    rd = B.predict_rd(raw, s.ref, sel, pa.sL, pa.L)
    assert rd.any() and np.array_equal(rd, B.predict_rd(R.pack_bases(raw, 3, 0), s.ref, sel, pa.sL, pa.L))


def test_cli_parses_and_refuses(capsys):
    s5 = ["step5", "in.bam", "out.bam", "--reference", "ref.fa"]
    a = cli.parse(s5 + ["--gpu-image", "true"])
    assert a.gpu_image == "true"
    assert cli.parse(s5).gpu_image == "false"
    assert cli.parse(["molecular", "in.bam", "out.bam", "--gpu-image", "true"]).gpu_image == "true"
    for argv, word in ((s5 + ["--gpu-image", "true", "--gpus", "2"], "--gpus 2"),
                       (s5 + ["--gpu-image", "true", "--stream", "false"], "--stream false"),
                       (["molecular", "in.bam", "out.bam", "--gpu-image", "true", "--stream", "false"], "--stream false")):
        with pytest.raises(SystemExit):
            cli.parse(argv)
        err = capsys.readouterr().err
        assert "--gpu-image" in err and word in err


def test_stream_job_field_and_runner_refusal():
    import dataclasses
    from bsseqconsensusreads_amd import stream
    names = [f.name for f in dataclasses.fields(stream.StreamJob)]
    assert names[-2:] == ["gpu_image", "gpu_inflate"]
    assert stream.StreamJob("a", "b", "c").gpu_image is False
    with pytest.raises(ValueError, match="gpu_image"):
        stream.run(stream.StreamJob("a.bam", "r.fa", "o.bam", gpu_image=True), runner=object())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_twin_under_sanitizers(tmp_path):
    """tests/sanitize/image_twin_main.cpp: the twin on heap buffers of their exact sizes under
    -fsanitize=address,undefined, every out-of-range entry refused (host code, its own main)."""
    exe = str(tmp_path / "image_twin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-x", "c++", os.path.join(ROOT, "tests", "sanitize", "image_twin_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "image twin ok" in r.stdout

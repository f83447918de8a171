"""cli group's host twins (csrc/bsdc_group.hip): bsdc_group_assign_host,
bsdc_group_format_host and group(host=True) against tests/group_ref.py on every case of
group_inputs.py -- ids, strands, order, the output records' bytes, the info dict -- and the refusals."""
import json

import numpy as np
import pytest

import group_inputs as GI
import group_ref as GR
from bsseqconsensusreads_amd import _lib, bam, bgzf, group, zipper


def write_input(path, recs):
    h = bam.BamHeader(GI.HEADER, [n for n, _ in GI.REFS], np.asarray([ln for _, ln in GI.REFS], np.int64))
    w = bgzf.BamWriter(str(path), h, 1)
    w.add_raw(b"".join(recs), 2)
    w.close(2)
    return str(path)


def split(buf: bytes):
    out, p = [], 0
    while p < len(buf):
        n = 4 + int.from_bytes(buf[p:p + 4], "little")
        out.append(buf[p:p + n])
        p += n
    return out


def records_of(path):
    r = zipper.read_records(path)
    return r.header, split(r.buf[:r.n_bytes].tobytes())


@pytest.fixture(scope="module")
def sweep_ref():
    recs = GI.sweep()
    return recs, GR.run(recs)


def check(tmp_path, recs, ref, **kw):
    inp = write_input(tmp_path / "in.bam", recs)
    info = group.group(inp, str(tmp_path / "out.bam"), host=True, info=str(tmp_path / "info.json"), threads=2, **kw)
    hdr, got = records_of(str(tmp_path / "out.bam"))
    assert got == ref.records
    for k, v in ref.info.items():
        assert info[k] == v, k
    assert info["raw_bytes"] == sum(map(len, ref.records)) and info["compressed_bytes"] > 0
    assert json.load(open(tmp_path / "info.json")) == info
    return hdr, info


@pytest.mark.parametrize("name", GI.NAMES)
def test_cases(tmp_path, name):
    for kw in GI.params(name):
        hdr, _ = check(tmp_path, GI.case(name), GR.run(GI.case(name), **kw), **kw)
    lines = hdr.text.splitlines()
    assert lines[0] == "@HD\tVN:1.5\tSO:unsorted\tGO:query\tSS:unsorted:template-coordinate"
    assert lines[1:] == GI.HEADER.splitlines()[1:] and list(hdr.ref_names) == [n for n, _ in GI.REFS]


@pytest.mark.parametrize("extra", [0, 1])
def test_lds_boundary(tmp_path, extra):
    """a group of exactly bsdc_group_lds_nodes() nodes, and of one more"""
    n = int(_lib.load().bsdc_group_lds_nodes())
    assert n == 7710
    recs = GI.past_lds(n) if extra else GI.at_lds(n)
    _, info = check(tmp_path, recs, GR.run(recs, edits=GI.LDS_EDITS), edits=GI.LDS_EDITS)
    assert info["max_nodes_in_group"] == n + extra and info["molecules"] == 1


def test_sweep(tmp_path, sweep_ref):
    _, info = check(tmp_path, *sweep_ref)
    assert info["templates_out"] >= 20000 and info["molecules"] > 1000


def test_options(tmp_path):
    recs = GI.case("drops")
    check(tmp_path, recs, GR.run(recs, min_map_q=0, include_non_pf=True), min_map_q=0, include_non_pf_reads=True)
    recs = [r.replace(b"RXZ", b"ZUZ") for r in GI.case("shuffled")]
    check(tmp_path, recs, GR.run(recs, raw_tag=b"ZU", assign_tag=b"NM"), raw_tag="ZU", assign_tag="NM")


def test_assign_words():
    """bsdc_group_assign_host on fabricated keys: ids, strands, order and stats"""
    k0 = np.asarray([5, 5, 5, 2, 5, 5], np.uint64)
    k1 = np.asarray([9, 9, 9, 9, 9, 8], np.uint64)
    umi = np.asarray([0x10, 0x11, 0x10, 0x10, 0x10, 0x10], np.uint64)
    strand = np.asarray([1, 0, 0, 0, 1, 0], np.uint8)
    mol, ab, order, stats = group.assign_host(k0, k1, umi, strand, 1)
    assert mol.tolist() == [2, 2, 2, 0, 2, 1] and ab.tolist() == [0, 1, 1, 0, 0, 0]
    assert order.tolist() == [3, 5, 0, 4, 1, 2] and stats.tolist() == [3, 4, 3, 2]
    mol, _, _, stats = group.assign_host(k0, k1, umi, strand, 0)
    assert mol.tolist() == [2, 3, 2, 0, 2, 1] and stats.tolist() == [3, 4, 4, 2]
    assert group.assign_host(k0[:0], k1[:0], umi[:0], strand[:0])[3].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("name", GI.ERRORS)
def test_errors(tmp_path, name):
    recs, word = GI.error_case(name)
    with pytest.raises(ValueError, match=word):
        group.group(write_input(tmp_path / "in.bam", recs), str(tmp_path / "out.bam"), host=True)


def test_refusals(tmp_path):
    lib = _lib.load()
    assert lib.bsdc_abi_version() == 19
    inp = write_input(tmp_path / "in.bam", GI.case("tie"))
    with pytest.raises(ValueError, match="adjacency"):
        group.group(inp, str(tmp_path / "o.bam"), strategy="adjacency", host=True)
    with pytest.raises(ValueError, match="edits"):
        group.group(inp, str(tmp_path / "o.bam"), edits=4, host=True)
    z = np.zeros(2, np.uint64)
    with pytest.raises(ValueError, match="edits"):
        group.assign_host(z, z, z, np.zeros(2, np.uint8), 7)
    bad = [GI.tpl("trunc", "AAAA-CCCC", aux2=b"XYZab")[0], GI.tpl("trunc", "AAAA-CCCC", aux2=b"XYZab")[1]]
    with pytest.raises(ValueError, match="trunc"):
        group.group(write_input(tmp_path / "bad.bam", bad), str(tmp_path / "o.bam"), host=True)
    from bsseqconsensusreads_amd import cli
    with pytest.raises(SystemExit):
        cli.parse(["group", "a.bam", "b.bam", "--strategy", "identity"])
    assert cli.parse(["group", "a.bam", "b.bam"]).edits == 1

"""cli group on the GPU (csrc/bsdc_group.hip): bsdc_group_assign (the device
sort, k_group_small, k_group_large with its LDS and scratch arenas) and bsdc_group_format
(k_group_write) against the host twins on every case of group_inputs.py, word for word and byte for
byte; cli group on the sweep against group(host=True); cli molecular on its output."""
import json

import numpy as np
import pytest
import torch

import group_inputs as GI
from bsseqconsensusreads_amd import _lib, bam, cli, group
from test_group_host import records_of, write_input
from test_zipper_host import records_of as recs_of_bytes

pytestmark = pytest.mark.gpu


def both(recs, arena=0, **kw):
    """assign + format of the records on the host and on the device -> the two results"""
    a = recs_of_bytes(recs)
    t = group.templates(a)
    tab = group.rec_table(a, t)
    mol, ab, order, stats = group.assign_host(t.k0, t.k1, t.umi, t.strand, kmax=t.kmax, **kw)
    off, buf = group.format_host(order, mol, ab, tab, a.buf)
    d_mol, d_ab, d_order, d_stats = group.assign_device(0, t.k0, t.k1, t.umi, t.strand, kmax=t.kmax, arena=arena, **kw)
    dst, total, _ = group.format_device(d_order, d_mol, d_ab, tab, a.buf)
    torch.cuda.synchronize()
    n = t.n
    host = (mol, ab, order, stats.tolist(), buf[:int(off[-1])].tobytes())
    dev = (d_mol.cpu().numpy().view(np.uint32)[:n], d_ab.cpu().numpy()[:n], d_order.cpu().numpy().view(np.uint32)[:n],
           d_stats.tolist(), dst[:total].cpu().numpy().tobytes())
    return host, dev


def same(host, dev):
    for h, d in zip(host[:3], dev[:3]):
        assert np.array_equal(h, d)
    assert host[3] == dev[3]
    assert host[4] == dev[4]


@pytest.mark.parametrize("name", GI.NAMES)
def test_cases(name):
    for kw in GI.params(name):
        same(*both(GI.case(name), **kw))


@pytest.mark.parametrize("name", ["nodes_65", "chain3000"])
def test_scratch_arena(name):
    same(*both(GI.case(name), arena=1))


@pytest.mark.parametrize("extra", [0, 1])
def test_lds_boundary(extra):
    """exactly bsdc_group_lds_nodes() nodes: the last group walked in LDS, its arrays ending at the
    arena's last byte; one more: the scratch arena under the full LDS launch"""
    n = int(_lib.load().bsdc_group_lds_nodes())
    host, dev = both(GI.past_lds(n) if extra else GI.at_lds(n), edits=GI.LDS_EDITS)
    assert host[3][2] == 1  # (one molecule: every node had its round)
    assert host[3][3] == n + extra
    same(host, dev)


@pytest.fixture(scope="module")
def sweep_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("sweep")
    inp = write_input(d / "in.bam", GI.sweep())
    want = group.group(inp, str(d / "host.bam"), host=True, threads=4)
    return d, inp, want


def test_cli_sweep(sweep_files):
    d, inp, want = sweep_files
    assert cli.main(["group", inp, str(d / "out.bam"), "--info", str(d / "info.json"), "--threads", "4"]) == 0
    got = json.load(open(d / "info.json"))
    assert records_of(str(d / "out.bam"))[1] == records_of(str(d / "host.bam"))[1]
    assert {k: v for k, v in got.items() if k != "compressed_bytes"} == {k: v for k, v in want.items() if k != "compressed_bytes"}
    assert cli.main(["group", inp, str(d / "again.bam"), "--threads", "4"]) == 0
    assert open(d / "again.bam", "rb").read() == open(d / "out.bam", "rb").read()


def mi_runs(path):
    """the runs of equal MI:Z values over a BAM's records, in file order"""
    _, recs = records_of(path)
    mi = [r[r.rindex(b"MIZ") + 3:r.index(b"\0", r.rindex(b"MIZ"))] for r in recs]
    return [x for k, x in enumerate(mi) if k == 0 or x != mi[k - 1]]


def test_cli_molecular_on_the_output(sweep_files, capfd):
    """cli molecular takes cli group's file as it stands: one family per <id>/<strand>, as many as
    the info's histogram counts, each emitted under its own MI"""
    d, inp, want = sweep_files
    assert cli.main(["group", inp, str(d / "grouped.bam"), "--info", str(d / "g.json"), "--threads", "4"]) == 0
    got = json.load(open(d / "g.json"))
    families = sum(got["family_size_histogram"].values())
    capfd.readouterr()
    assert cli.main(["molecular", str(d / "grouped.bam"), str(d / "cons.bam"), "--threads", "4"]) == 0
    info = json.loads(capfd.readouterr().err.strip().splitlines()[-1])
    runs_in, runs_out = mi_runs(str(d / "grouped.bam")), mi_runs(str(d / "cons.bam"))
    print("histogram families %d, molecular: %r, MI runs in %d, out %d" % (families, info, len(runs_in), len(runs_out)))
    assert len(runs_in) == families and len(set(runs_in)) == families
    assert info["records_in"] == 2 * got["templates_out"]
    assert info["families"] == families
    assert info["families_emitted"] == families and info["records_out"] == 2 * families
    assert len(runs_out) == families and sorted(runs_out) == sorted(runs_in)

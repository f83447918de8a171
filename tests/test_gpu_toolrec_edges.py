"""The tool-stage record writer's kernels (csrc/bsdc_toolrec.hip) and its instance of the offset scan
(csrc/bsdc_devtext.h) at the edges the fabricated sets of test_gpu_toolrec.py do not reach by
themselves: a destination at every byte phase, a dump that ends with the last base, the clamp at
`cap` when the records outgrow bsdc_toolrec_bytes_bound (table entries that share their bytes), a
dump slot that leaves n_dump, more workgroup sums than one tile of k_scan_scan, and offsets past
2^31 and 2^32.  The references: the host twin (itself held to the restatement toolrec_ref.py in
test_toolrec_host.py), the restatement, and numpy's cumulative sum of the layout rule's sizes."""
import numpy as np
import pytest
import torch

import toolrec_inputs as TI
import toolrec_ref as TR
from test_gpu_toolrec import device_format
from test_toolrec_host import GUARD, twin, twin_call

pytestmark = pytest.mark.gpu
_twins = {}


def _err(engine):
    return engine.lib.bsdc_toolrec_last_error().decode()


def _named(name):
    """(case, the twin's offsets, the twin's bytes) of a named set, made once"""
    if name not in _twins:
        c = TI.build_named(name)
        off, buf = twin(c)
        _twins[name] = (c, off, buf[:int(off[-1])].copy())
    return _twins[name]


def _assert_bytes(got, want, off, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: byte %d (record %d): %d vs %d" % (
        what, bad[0], int(np.searchsorted(off, bad[0], "right")) - 1, got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("name", ["phases", "place", "lens"])
def test_destination_at_every_byte_phase(engine, name, shift):
    """dst = an aligned address + shift: a record's start in its dword comes from the address, not
    from its offset alone; the bytes in front of dst and behind the total stay"""
    c, want_off, want = _named(name)
    rc, off, buf = device_format(engine, c, dst_shift=shift)
    assert rc == 0, _err(engine)
    assert np.array_equal(off, want_off)
    total = int(off[-1])
    _assert_bytes(buf[shift:shift + total], want, off, "%s at +%d" % (name, shift))
    assert (buf[:shift] == GUARD).all() and (buf[shift + total:] == GUARD).all()


@pytest.mark.parametrize("L", TI.TIGHT)
def test_dump_that_ends_with_the_last_base(engine, L):
    """n_dump = the last record's last base exactly (any value is in the contract, a multiple of 4
    or not): no aligned dword of the dump holds that record's last bases whole, so its QUAL and SEQ
    dwords go byte by byte (tr_can4), at every destination phase"""
    c = TI.build_named("tight_%d" % L)
    want_off, want = TR.stream(c.recs)
    n_dump = int(c.rec_off[-1]) + L
    rc, hoff, hbuf = twin_call(c, n_dump=n_dump)
    assert rc == 0 and np.array_equal(hoff, want_off) and hbuf[:int(want_off[-1])].tobytes() == want
    want = np.frombuffer(want, np.uint8)
    for shift in range(4):
        rc, off, buf = device_format(engine, c, n_dump=n_dump, dst_shift=shift)
        assert rc == 0, _err(engine)
        assert np.array_equal(off, want_off)
        _assert_bytes(buf[shift:shift + want.shape[0]], want, off, "L %d at +%d" % (L, shift))
        assert (buf[:shift] == GUARD).all() and (buf[shift + want.shape[0]:] == GUARD).all()


@pytest.mark.parametrize("shift", [0, 1])
def test_cap_clamp_with_shared_table_entries(engine, shift):
    """200 records on one name, one cigar and one aux block: their total is far beyond the bound,
    which is the cap.  The offsets are whole, the bytes below cap are the restatement's and every
    byte from cap on is untouched.  cap lies inside a record at 2 mod 4 (3 mod 4 of the aligned
    address with shift 1): the last dword leaves as single bytes, those before it whole"""
    c = TI.shared_case()
    want_off, want = TR.stream([TI.record_of(c, r) for r in range(c.n)])
    cap = c.tables().bound(c.dump_seq.shape[0])
    total = int(want_off[-1])
    k = int(np.searchsorted(want_off, cap, "right")) - 1
    assert cap < total and cap % 4 == 2 and want_off[k] + 4 <= cap <= want_off[k + 1] - 4
    rc, off, buf = device_format(engine, c, cap=cap, dst_shift=shift, alloc=total + 64)
    assert rc == 0, _err(engine)
    assert np.array_equal(off, want_off)
    _assert_bytes(buf[shift:shift + cap], np.frombuffer(want, np.uint8)[:cap], off, "below cap")
    assert (buf[:shift] == GUARD).all() and (buf[shift + cap:] == GUARD).all()


def test_dump_slot_that_leaves_n_dump(engine):
    """the call is told a dump that ends inside the third record from the end (the buffers keep
    their size): those three are written with l_seq 0 and read nothing, the others do not change"""
    c, _, _ = _named("counts_65")
    n = c.n
    n_dump = int(c.rec_off[n - 3]) + int(c.dump_len[n - 3]) - 1
    assert int(c.rec_off[n - 4]) + int(c.dump_len[n - 4]) <= n_dump and (c.dump_len[n - 3:] > 0).all()
    empty = np.zeros(0, np.uint8)
    recs = [dict(r, seq=empty, qual=empty) if k >= n - 3 else r for k, r in enumerate(c.recs)]
    want_off, want = TR.stream(recs)
    full_off = TR.stream(c.recs)[0]
    assert np.array_equal(want_off[:n - 2], full_off[:n - 2]) and want_off[-1] < full_off[-1]
    cap = c.tables().bound(c.dump_seq.shape[0] // 4 * 4) + 64
    rc, off, buf = device_format(engine, c, cap=cap, n_dump=n_dump)
    assert rc == 0, _err(engine)
    assert np.array_equal(off, want_off)
    total = int(off[-1])
    _assert_bytes(buf[:total], np.frombuffer(want, np.uint8), off, "slots past n_dump")
    assert (buf[total:] == GUARD).all()
    rc, _, _ = twin_call(c, n_dump=n_dump, cap=cap)  # (the twin reads the dump's table and refuses)
    assert rc == -22


@pytest.mark.parametrize("n_rec", TI.CARRY_COUNTS)
def test_scan_carries_over_its_tile(engine, n_rec):
    """256, 257 and 258 workgroup sums: k_scan_scan's second round starts from the first one's
    carry.  The offsets against numpy's cumulative sum of the layout rule's sizes, the bytes
    against the twin"""
    assert TI.scan_groups(n_rec) == 256 + TI.CARRY_COUNTS.index(n_rec)
    c = TI.carry_case(n_rec)
    want_off = np.concatenate([[0], np.cumsum(TI.layout_sizes(c))])
    rc, off, buf = device_format(engine, c)
    assert rc == 0, _err(engine)
    bad = np.nonzero(off != want_off)[0]
    assert bad.size == 0, "off[%d] (workgroup %d): %d vs %d" % (bad[0], bad[0] // TI.SCAN_GROUP, off[bad[0]], want_off[bad[0]])
    hoff, hbuf = twin(c)
    total = int(off[-1])
    assert np.array_equal(hoff, want_off)
    _assert_bytes(buf[:total], hbuf[:total], off, "%d records" % n_rec)
    assert (buf[total:] == GUARD).all()


def test_offsets_past_4_gib(engine):
    """270 records on one 16 MiB aux block: the stream is 4.2 GiB long, and a record lies across
    2^31 and another across 2^32.  Checked on the device: every record's aux bytes against the
    block, its bytes in front of them and its RD / LA tags against the restatement, the offsets
    against numpy's int64 sum, the bytes behind the total"""
    dev = engine.device
    free = torch.cuda.mem_get_info(dev)[0]
    if free < 6 << 30:
        pytest.skip("%.1f GiB free on the device, the 4.2 GiB stream needs 6" % (free / 2 ** 30))
    A = 1 << 24
    c = TI.far_case(270, A)
    sizes = TI.layout_sizes(c)
    want_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(want_off[-1])
    for edge in (1 << 31, 1 << 32):
        r = int(np.searchsorted(want_off, edge, "right")) - 1
        assert want_off[r] + 36 < edge < want_off[r + 1] - 8, edge  # (a record's aux bytes lie across it)
    assert total > (1 << 32) + 13 * A
    rc, off, buf = device_format(engine, c, cap=total + 64, alloc=total + 128, fetch=False)
    assert rc == 0, _err(engine)
    assert np.array_equal(off.cpu().numpy(), want_off)
    assert bool((buf[total:] == GUARD).all())
    aux = torch.from_numpy(c.tables().aux[:A].copy()).to(dev)
    conv = 8 * c.conv.astype(np.int64)
    o_aux = sizes - A - conv
    idx, want = [], []
    for r in range(c.n):
        a = int(want_off[r] + o_aux[r])
        assert torch.equal(buf[a:a + A], aux), "record %d: its aux bytes" % r
        # the restatement of the record with no aux bytes, its block_size raised by them
        w = TR.record_bytes(TI.record_of(c, r, aux=b""))
        w = (len(w) - 4 + A).to_bytes(4, "little") + w[4:]
        assert len(w) + A == sizes[r]
        idx += [np.arange(want_off[r], a), np.arange(a + A, want_off[r + 1])]
        want.append(w)
    got = buf[torch.from_numpy(np.concatenate(idx)).to(dev)].cpu().numpy()
    assert got.tobytes() == b"".join(want)

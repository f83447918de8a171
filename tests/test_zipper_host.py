"""cli zipper's host twins (bsdc_zip_format_host, bsdc_zip_sort_host; zipper.py's join, tables and
header) against the pure-Python restatement (tests/zipper_ref.py): the edge records byte for byte,
the errors, the sort against np.lexsort, and a step-5 input split into its aligned and unmapped
halves and zipped back."""
import numpy as np
import pytest

import zipper_inputs as ZI
import zipper_ref as ZR
from bsseqconsensusreads_amd import _lib, bam, synth, zipper

GUARD = 0xA5


def records_of(recs, text="") -> zipper.Records:
    data = b"".join(recs)
    buf = zipper._aligned_copy(data)
    return zipper.Records(bam.BamHeader(text, [], np.zeros(0, np.int64)), buf, len(data), zipper.scan(buf, len(data)))


def prepare(a_recs, u_recs, setting):
    """-> (aligned Records, zipper.Tables, the tag lists' struct)"""
    s = ZI.SETTINGS[setting]
    a, u = records_of(a_recs), records_of(u_recs)
    partner, lonely = zipper.join(a, u)
    t = zipper.tables(a, u, partner)
    tags = zipper.tags_struct(zipper.tag_list(s["reverse"], zipper.CONSENSUS_REVERSE),
                              zipper.tag_list(s["revcomp"], zipper.CONSENSUS_REVCOMP), zipper.tag_list(s["remove"], ()))
    return a, t, tags, lonely


def twin(a_recs, u_recs, setting, cap=None, fill=GUARD):
    """-> (off, the buffer, the templates without an aligned record) of the host twins"""
    a, t, tags, lonely = prepare(a_recs, u_recs, setting)
    _, idx = zipper.sort_host(t.keys, t.idx, t.max_ref, t.max_pos)
    off, buf = zipper.format_host(idx, t.tab, a.buf, t.part, tags, cap=cap, fill=fill)
    return off, buf, lonely


def reference(a_recs, u_recs, setting):
    s = ZI.SETTINGS[setting]
    out, counts = ZR.zip_records(ZR.parse_records(b"".join(a_recs)), ZR.parse_records(b"".join(u_recs)), **s)
    return [ZR.encode(r) for r in out], counts


@pytest.mark.parametrize("setting", sorted(ZI.SETTINGS))
@pytest.mark.parametrize("name", ZI.NAMES)
def test_twin_equals_the_restatement(name, setting):
    a, u = ZI.case(name)
    want, counts = reference(a, u, setting)
    off, buf, lonely = twin(a, u, setting)
    assert off.shape[0] == len(want) + 1 and lonely == counts["templates_without_aligned"]
    for k, w in enumerate(want):
        got = buf[int(off[k]):int(off[k + 1])].tobytes()
        assert got == w, "%s / %s: record %d (%r)" % (name, setting, k, ZR.parse_records(w)[0]["name"][:20])
    assert (buf[int(off[-1]):] == GUARD).all()


def test_cap_is_respected_exactly():
    a, u = ZI.case("all")
    ar, t, tags, _ = prepare(a, u, "consensus")
    assert zipper.bound(t.tab) == int(t.tab["rec_len"].sum() + t.tab["part_len"].sum())
    with pytest.raises(ValueError, match="below bsdc_zip_bytes_bound"):
        zipper.format_host(t.idx, t.tab, ar.buf, t.part, tags, cap=zipper.bound(t.tab) - 1)


@pytest.mark.parametrize("name", ZI.ERRORS)
def test_errors_name_the_read(name):
    a, u, word = ZI.error_case(name)
    with pytest.raises(ValueError) as ref:
        reference(a, u, "none")
    with pytest.raises(ValueError) as got:
        twin(a, u, "none")
    assert repr(word) in str(got.value) or "(read %s)" % word in str(got.value), str(got.value)
    for what in ("no partner", "twice", "unknown type", "runs past"):
        assert (what in str(ref.value)) == (what in str(got.value)), (str(ref.value), str(got.value))


def test_scan_refuses_truncated_records():
    data = ZI.rec("r", 99, 0, 1)
    for cut in (data[:-1], data[:20], data + b"\1\0"):
        buf = zipper._aligned_copy(cut)
        with pytest.raises(ValueError, match="truncated"):
            zipper.scan(buf, len(cut))


@pytest.mark.parametrize("name", ZI.SORTS)
def test_sort_twin_equals_lexsort(name):
    assert _lib.load().bsdc_zip_sort_tile() == 2048  # (what the tile-sized inputs are made for)
    ref, pos, flag = ZI.sort_case(name)
    n = ref.shape[0]
    keys = zipper.sort_keys(ref, pos, flag)
    want = np.lexsort((np.arange(n), (flag & 16) != 0, pos, ref))
    k, v = zipper.sort_host(keys, np.arange(n, dtype=np.uint32), int(ref.max()) if n else 0, int(pos.max()) if n else 0)
    assert np.array_equal(v, want.astype(np.uint32)) and np.array_equal(k, keys[want])
    # a payload of its own travels with its key; bounds larger than the keys need change nothing
    pay = (np.arange(n, dtype=np.uint32) * 7 + 3)
    k2, v2 = zipper.sort_host(keys, pay, 1 << 20, (1 << 31) - 2)
    assert np.array_equal(v2, pay[want]) and np.array_equal(k2, k)


def test_sort_refusals():
    lib = _lib.load()
    k, v = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    assert lib.bsdc_zip_sort_host(k.ctypes.data, v.ctypes.data, -1, 0, 0) == -22
    assert lib.bsdc_zip_sort_host(None, v.ctypes.data, 4, 0, 0) == -22
    assert lib.bsdc_zip_sort_host(k.ctypes.data, v.ctypes.data, 4, -1, 0) == -22
    assert b"max_ref" in lib.bsdc_zip_last_error()


def test_header_equals_the_restatement():
    h = zipper.header(bam.BamHeader(ZI.HEADER_A, [n for n, _ in ZI.REFS], np.asarray([l for _, l in ZI.REFS])),
                      bam.BamHeader(ZI.HEADER_U, [], np.zeros(0, np.int64)))
    assert h.text == ZR.header_text(ZI.HEADER_A, ZI.HEADER_U) and h.ref_names == ["chr1", "chr2", "chr3"]
    assert list(h.ref_lens) == [l for _, l in ZI.REFS]


# ---- split and zip back ----

def split_input(tmp, cfg, n_fam=200, seed=5):
    """A small step-5 input of synth (messify on) whose records carry their other tags, then MI, RX
    and RG -> (header text, refs, the original's parsed records shuffled; ALIGNED's records: those
    without MI / RX / RG; UNMAPPED's: a 77 / 141 pair per template carrying them)."""
    s = synth.generate(cfg, n_fam, seed=seed, device="cpu", genome_len=100_000)
    raw = synth.messify(s.raw, frac=0.1, seed=2)
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n@RG\tID:A\tLB:L\n" % (s.ref.names[0], int(s.ref.lengths[0]))
    p = str(tmp / ("synth_%s.bam" % cfg))
    bam.write_bam(p, bam.BamHeader(text, [s.ref.names[0]], np.asarray([int(s.ref.lengths[0])], np.int64)),
                  bam.records_to_bam(raw), level=1, threads=2)
    _, refs, data, _ = ZR.read_bam(p)
    recs = ZR.parse_records(data)
    moved = (b"MI", b"RX", b"RG")
    for r in recs:
        tg = ZR.walk(r["aux"])
        mi = [b for nm, _, b in tg if nm == b"MI"]
        assert len(mi) == 1
        r["aux"] = b"".join(b for nm, _, b in tg if nm not in moved) + mi[0] + ZI.tag("RX", "Z", "ACG-TTA") + ZI.tag("RG", "Z", "A")
    order = np.random.default_rng(seed).permutation(len(recs))
    recs = [recs[int(k)] for k in order]
    aligned, unmapped, seen = [], [], set()
    for r in recs:
        tg = ZR.walk(r["aux"])
        aligned.append(ZR.encode(dict(r, aux=b"".join(b for nm, _, b in tg if nm not in moved))))
        k = (r["name"], r["flag"] & 0xC0)
        assert k not in seen and r["flag"] & 0xC0 in (0x40, 0x80)
        seen.add(k)
        unmapped.append(ZI.rec(r["name"], 77 if r["flag"] & 0x40 else 141, aux=b"".join(b for nm, _, b in tg if nm in moved)))
    return text, refs, recs, aligned, unmapped


def rule6(recs):
    return [recs[k] for k in sorted(range(len(recs)), key=lambda k: (recs[k]["ref"], recs[k]["pos"], recs[k]["flag"] & 16 != 0, k))]


@pytest.mark.parametrize("cfg", ["C0", "C2"])
def test_split_and_zip_back(tmp_path, cfg):
    text, refs, recs, aligned, unmapped = split_input(tmp_path, cfg)
    assert len(recs) > 400 and any(r["flag"] & 16 for r in recs)
    pa, pu, po = (str(tmp_path / x) for x in ("a.bam", "u.bam", "o.bam"))
    ZR.write_bam(pa, text.replace("SO:coordinate", "SO:unsorted"), refs, b"".join(aligned))
    ZR.write_bam(pu, "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:A\tLB:L\n", [], b"".join(unmapped[::-1]))
    info = zipper.zipper(pa, pu, po, threads=2, level=1, host=True, info=str(tmp_path / "i.json"))
    otext, orefs, data, _ = ZR.read_bam(po)
    assert otext.split("\n")[0] == "@HD\tVN:1.6\tSO:coordinate" and orefs == refs and "@RG\tID:A\tLB:L" in otext
    got, want = ZR.parse_records(data), rule6(recs)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g["name"], w["name"])
    assert data == b"".join(ZR.encode(r) for r in want)
    assert info["records_in"] == info["records_out"] == len(recs) and info["unmapped_dropped"] == 0
    assert info["templates_without_aligned"] == 0 and info["raw_bytes"] == len(data)
    import json
    assert json.load(open(str(tmp_path / "i.json"))) == info
    # what the package's own reader sees: the original's MI values, in order
    _, back = bam.read_bam(po, threads=2)
    assert back.n == len(want) and np.array_equal(back.pos, [r["pos"] for r in want])
    mi = lambda r: dict((nm, b) for nm, _, b in ZR.walk(r["aux"]))[b"MI"][3:-1].decode()  # noqa: E731
    assert [back.mi_names[int(k)] + "/" + "AB"[int(s)] for k, s in zip(back.mi_id, back.mi_strand)] == [mi(r) for r in want]

"""tests/group_ref.py (cli group's rules) against ids, strands and order derived by
hand on the small named cases, and that each case of group_inputs.py reaches its stated path."""
import pytest

import group_inputs as GI
import group_ref as GR


def tags(name, **kw):
    return {k.decode(): v.decode() for k, v in GR.run(GI.case(name), **kw).tags.items()}


def by_prefix(t):
    out = {}
    for k, v in t.items():
        out.setdefault(k.split("_")[0], set()).add(v)
    return out


def test_chain():
    assert set(tags("chain").values()) == {"0/A"}


def test_fence():
    assert by_prefix(tags("fence")) == {"p": {"0/A"}, "j": {"0/A"}, "r": {"1/A"}, "q": {"2/A"}, "s": {"2/A"}}


def test_tie():
    assert by_prefix(tags("tie")) == {"y": {"0/A"}, "x": {"1/A"}}


def test_two_roots():
    assert by_prefix(tags("two_roots")) == {"r1": {"0/A"}, "ch": {"0/A"}, "r2": {"1/A"}}


def test_duplex_and_order():
    r = GR.run(GI.case("duplex"))
    assert {k.decode(): v.decode() for k, v in r.tags.items()} == {"d1": "0/A", "d4": "0/A", "d2": "0/B", "d3": "0/B"}
    assert [GR.Rec(b).name.decode() for b in r.records] == ["d1", "d1", "d4", "d4", "d2", "d2", "d3", "d3"]
    assert [GR.Rec(b).flag & 0xC0 for b in r.records] == [0x40, 0x80] * 4
    assert r.records[0].endswith(b"MIZ0/A\0")


def test_bottom_only():
    assert tags("bottom_only") == {"b1": "0/A", "b2": "0/A", "t9": "1/A"}


def test_edits():
    got = {e: by_prefix(tags("edits", edits=e)) for e in (0, 1, 2, 3)}
    assert [len({min(v) for v in got[e].values()}) for e in (0, 1, 2, 3)] == [6, 2, 2, 2]
    assert got[1]["e4"] == {"0/A"} and got[1]["sw"] == {"1/A"}  # (the chain carries e4 in at one edit a step)
    assert got[0]["e1"] != got[0]["e0"]


def test_paths():
    info = {n: GR.run(GI.case(n)).info for n in GI.NAMES if n != "edits"}
    for n in (1, 2, 63, 64, 65):
        assert info["nodes_%d" % n]["max_nodes_in_group"] == n and info["nodes_%d" % n]["position_groups"] == 1
    assert info["chain3000"]["max_nodes_in_group"] == 3000 and info["chain3000"]["molecules"] == 1
    assert info["near_groups"]["position_groups"] == 3 and info["near_groups"]["templates_out"] == 4
    assert info["clipped"]["position_groups"] == 1 and info["clipped"]["molecules"] == 1
    assert info["halves"]["position_groups"] == 3 and info["halves"]["molecules"] == 3
    d = info["drops"]
    assert all(d[k] >= 1 for k in GR.DROPS) and d["templates_out"] == 1 and d["templates_in"] == 9
    assert info["chain"]["family_size_histogram"] == {"17": 1}
    assert info["duplex"]["family_size_histogram"] == {"2": 2}


def test_existing_tag_removed_by_type():
    r = GR.run(GI.case("shuffled"))
    m1 = [b for b in r.records if GR.Rec(b).name == b"m1"]
    m2 = [b for b in r.records if GR.Rec(b).name == b"m2"]
    assert b"77/B" not in m1[0] and b"MIi" not in m1[1] and m1[0].count(b"MIZ") == 1
    assert bytes(b"MIZ9/A\0MIZ") in m2[0] and b"zyZMIZ\0" in m2[1]  # (payloads that spell the tag stay)


@pytest.mark.parametrize("name", [e for e in GI.ERRORS if not e.startswith("r1_")])  # (the rules' errors; r1_*: malformed bytes)
def test_errors(name):
    recs, word = GI.error_case(name)
    with pytest.raises(ValueError, match=word):
        GR.run(recs)

"""CPU side of the fence tests: the helper's own logic on CPU tensors, the coverage the case table claims, and the oracle alone on
every case -- no field of any case may fall into the reference's undefined over-read (the cap on left-out fields is zero)."""
import numpy as np
import pytest

import crtref as R
import fence as F
import fence_cases as FC


def _fenced(n=3, payload=27, stride=40, base_off=3, pitch=9):
    f = F.Fenced(n, payload, stride, base_off, pitch, device="cpu", name="probe")
    pre = f.prefill(1234)
    return f, pre


def test_guards_are_a_condition_not_a_measurement():
    assert F.guard_bytes(0) == 4096 and F.guard_bytes(9) == 4096
    assert F.guard_bytes(1921 * 4) >= 2 * 1921 * 4 and F.guard_bytes(5000) % F.ALIGN == 0
    f, _ = _fenced()
    assert f.start == f.guard + 3 and f.total == f.start + 3 * 40 + f.guard
    assert f.total - f.end >= f.guard and f.start >= f.guard


def test_fill_is_never_a_constant_and_depends_on_the_seed():
    f, pre = _fenced()
    assert len(np.unique(pre[:f.start])) > 64 and len(np.unique(pre[f.end:])) > 64
    assert np.count_nonzero(f.prefill(99) != pre) > f.total // 2
    np.testing.assert_array_equal(f.host(), f.prefill(99))


def test_payload_view_and_prefill_contents():
    f = F.Fenced(3, 27, 40, 3, 9, device="cpu")
    contents = np.arange(81, dtype=np.uint8).reshape(3, 27)
    pre = f.prefill(7, contents)
    v = f.view((3, 9))
    assert tuple(v.shape) == (3, 3, 9) and v.stride(0) == 40 and v[0].is_contiguous()
    np.testing.assert_array_equal(v.numpy().reshape(3, 27), contents)
    np.testing.assert_array_equal(f.payloads(pre), contents)
    assert f.ptr() == f.raw.data_ptr() + f.start
    import torch
    g = F.Fenced(2, 16, 24, 4, device="cpu")
    assert tuple(g.view((4,), torch.int32).shape) == (2, 4)
    with pytest.raises(ValueError):
        F.Fenced(2, 16, 24, 3, device="cpu").view((4,), torch.int32)


@pytest.mark.parametrize("where", ["last front guard byte", "first gap byte behind slot 1", "first back guard byte", "first byte of all", "last byte of all"])
def test_one_changed_byte_is_reported_with_its_location(where):
    f, pre = _fenced()
    off, region, slot, dist = {
        "last front guard byte": (f.start - 1, "front guard", 0, -1),
        "first gap byte behind slot 1": (f.start + 40 + 27, "gap", 1, 1),
        "first back guard byte": (f.start + 3 * 40, "back guard", 2, 14),
        "first byte of all": (0, "front guard", 0, -f.start),
        "last byte of all": (f.total - 1, "back guard", 2, f.total - f.end),
    }[where]
    f.raw[off] = int(pre[off]) ^ 0x40
    ch = f.first_change(pre)
    assert ch[:4] == (off, region, slot, dist) and ch[4] == int(pre[off]) and ch[5] == int(pre[off]) ^ 0x40 and ch[6] == 1
    with pytest.raises(AssertionError) as e:
        f.assert_fence_intact(pre)
    msg = str(e.value)
    assert "offset %d" % off in msg and region in msg and "slot %d" % slot in msg and "%+d bytes" % dist in msg


def test_gap_byte_nearer_to_the_next_slot_names_that_slot():
    f, pre = _fenced()
    off = f.start + 40 + 39                                    # the byte right in front of slot 2
    f.raw[off] ^= 1
    assert f.first_change(pre)[:4] == (off, "gap", 2, -1)


def test_a_change_inside_a_payload_is_not_reported_by_the_fence():
    f, pre = _fenced()
    for k in range(3):
        f.raw[f.start + 40 * k] ^= 0xff
        f.raw[f.start + 40 * k + 26] ^= 0xff
    assert f.first_change(pre) is None
    f.assert_fence_intact(pre)
    with pytest.raises(AssertionError):
        f.assert_unchanged(pre)                                # ... but by the check of a read-only buffer


# ---- the case table holds what it claims ----------------------------------------------------------------------------------------
def test_case_table_row_bytes_cover_the_branches():
    pic = {FC.picture_row_bytes(c) for c in FC.CASES}
    assert any(b < 16 for b in pic) and any(b >= 16 and b % 16 == 0 for b in pic) and any(b > 16 and b % 16 for b in pic)
    img = {FC.image_row_bytes(c) for c in FC.CASES if not FC.is_nes(c)}
    assert any(b < 16 for b in img) and 16 in img and any(17 <= b <= 31 for b in img) and any(b > 128 for b in img)
    assert {303, 132} <= pic and any(c["outh"] == 2049 for c in FC.CASES)


def test_case_table_strides_and_bases():
    four = [c for c in FC.CASES if FC.in_bpp(c) == 4]
    three = [c for c in FC.CASES if FC.in_bpp(c) == 3]
    assert {c["img"][1] for c in four} >= {0, 4, 8, 12} and {c["img"][1] for c in three} >= {1, 2, 3}
    assert {c["img"][0] for c in four} >= {"tight", "row", 4, 4100} and {c["img"][0] for c in three} >= {"tight", "row", 3, 4100}
    o4 = [c for c in FC.CASES if R.bpp4fmt(c["ofmt"]) == 4]
    o3 = [c for c in FC.CASES if R.bpp4fmt(c["ofmt"]) == 3]
    assert {c["out"] for c in o4} >= set(FC.OUT4) and {c["out"] for c in o3} >= set(FC.OUT3)
    lane = [c for c in FC.CASES if c["id"].startswith("lane-")]
    assert {c["img"] for c in lane} == set(FC.IMG4) | set(FC.IMG3) and {c["out"] for c in lane} == set(FC.OUT4) | set(FC.OUT3)
    for c in FC.CASES:
        assert c["noise"] <= 24 and (c["n"] in (2, 3) or c["set_first"] or c["overlap"]), c["id"]
        payload, stride, base, spare = FC.image_layout(c)
        assert stride >= payload and base < F.ALIGN
        assert all(t[0] <= 24 for t in c["triples"] or [])
    nes = [c for c in FC.CASES if FC.is_nes(c)]
    assert nes and all(FC.image_layout(c)[1] % 2 == 0 and c["img"][1] % 2 == 0 for c in nes)
    for c in FC.CASES:
        if c["set_first"]:
            assert c["n"] == 5 and len(c["set_first"]) == 4 and len({b - a for a, b in FC.sets_of(c)}) > 1


@pytest.mark.parametrize("id", FC.CASE_IDS)
def test_the_oracle_excludes_no_field(id):
    c = FC.case(id)
    want = FC.expected(c)
    assert want["excluded"] == [], "%s: the reference reads past inp[] for fields %r (undefined): pick other inputs" % (id, want["excluded"])
    assert want["out"].shape == (c["n"], FC.picture_layout(c)[0])

"""CPU checks of the hue knob (crthip_knobs_prepare8, include/crt_hip.h; the GPU side is tests/test_gpu_hues.py): the hue records
against crthip_params_finalize per field, the other records and both envs against crthip_knobs_prepare7's, the refusals, the
(n, 8) plumbing of crtlib without a device, a model of the margin patch, and the yardstick of the GPU tests -- the oracle with eight
knobs per field, the serial loop of sequence mode -- against the compiled reference."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import hues_cases as HU
import knobs_cases as KC

SYSTEMS = ("ntsc", "ntscp0", "vhs", "vhslcg", "snes", "temp", "nesrgb", "ntscbloom")
ALL_HUES = HU.HUES_A + HU.HUES_B + HU.STRADDLE + HU.DCO_HUES


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    R.build_oracle()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_knobs_prepare8"), "no crthip_knobs_prepare8 in this build"
    return crtlib


def _base(lib, name="ntsc", **kw):
    return lib.make_params(name, w=64, h=48, outw=160, outh=120, format=lib.FMT_BGRA, out_format=lib.FMT_BGRA, **kw)


def _tables(p):
    return np.concatenate([np.array(p.burst).reshape(-1), np.array(p.modI).reshape(-1), np.array(p.modQ).reshape(-1)])


def test_structs_and_abi(lib):
    assert (C.sizeof(lib.Knobs8), C.sizeof(lib.HueRec), C.sizeof(lib.HuesEnv)) == (32, 640, 32)
    assert lib.HUE_REC_INTS == 160 and C.sizeof(lib.HueRec) % 128 == 0
    assert lib.load_library().crthip_abi_version() == 6


@pytest.mark.parametrize("as_color", [1, 0])
@pytest.mark.parametrize("name", SYSTEMS)
def test_hue_records_equal_finalize_per_field(lib, name, as_color):
    """hues[k] = the three tables crthip_params_finalize derives for a copy of p whose hue is field k's: every 4-sample system, both
    chroma patterns (ntsc / ntscp0), as_color 0 (all zeros, except NES-RGB, which has no such switch)"""
    rows = [HU.D7 + (h,) for h in ALL_HUES]
    p = _base(lib, name, as_color=as_color)
    recs, levs, hues, env, lenv, henv = lib.knobs_prepare8(p, np.array(rows))
    assert hues.shape == (len(rows), 160) and (henv.n, henv.magic != 0, any(henv.reserved)) == (len(rows), True, False)
    assert henv.magic not in (env.magic, lenv.magic)
    for k, r in enumerate(rows):
        q = _base(lib, name, as_color=as_color, hue=r[7])
        np.testing.assert_array_equal(hues[k, :150], _tables(q), err_msg="%s hue %d" % (name, r[7]))
        assert not hues[k, 150:].any()
    if not as_color and name != "nesrgb":
        assert not hues.any()
    else:
        assert len({bytes(h) for h in hues}) >= 10, "the hues really give different tables"
    if name == "nesrgb":                                   # rotates only its burst (hue_in_mod == 0)
        assert (hues[:, lib.HUE_MODI:] == hues[0, lib.HUE_MODI:]).all() and len({bytes(h[:50]) for h in hues}) >= 10


def test_whole_turns_follow_the_reference_s_integer_division(lib):
    """360 and -360 against 0: whatever crthip_params_finalize says (angle * 8192 / 180 truncates); negative angles truncate as C's"""
    p = _base(lib)
    _, _, hues, _, _, _ = lib.knobs_prepare8(p, np.array([HU.D7 + (h,) for h in (0, 360, -360, -1, 359)]))
    for k, h in enumerate((0, 360, -360, -1, 359)):
        np.testing.assert_array_equal(hues[k, :150], _tables(_base(lib, hue=h)))


@pytest.mark.parametrize("name", ("ntsc", "snes", "vhs"))
def test_other_records_and_envs_are_prepare7_s(lib, name):
    p = _base(lib, name)
    for cid, rows in HU.BATCHES.items():
        rows = np.array(rows)
        r7, l7, e7, le7 = lib.knobs_prepare7(p, rows[:, :7])
        r8, l8, _, e8, le8, _ = lib.knobs_prepare8(p, rows)
        np.testing.assert_array_equal(r7, r8)
        np.testing.assert_array_equal(l7, l8)
        assert bytes(e7) == bytes(e8) and bytes(le7) == bytes(le8), cid


def test_blob_s_own_hue_is_ignored(lib):
    rows = np.array(HU.BATCHES["straddle"])
    a = lib.knobs_prepare8(_base(lib), rows)
    b = lib.knobs_prepare8(_base(lib, hue=77), rows)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else bytes(x) == bytes(y)


def test_refusals(lib):
    L = lib.load_library()
    p = _base(lib)
    kin = (lib.Knobs8 * 2)()
    for k in range(2):
        kin[k].noise, kin[k].saturation, kin[k].contrast, kin[k].white_point, kin[k].hue = 24, 10, 180, 100, 33 - 100 * k
    recs, levs, hues = (lib.KnobRec * 2)(), (lib.LevelRec * 2)(), (lib.HueRec * 2)()
    env, lenv, henv = lib.KnobsEnv(), lib.LevelsEnv(), lib.HuesEnv()
    good = [C.byref(p), 2, kin, recs, levs, hues, C.byref(env), C.byref(lenv), C.byref(henv)]
    call = L.crthip_knobs_prepare8
    assert call(*good) == 0
    for i in (0, 2, 3, 4, 5, 6, 7, 8):                     # every pointer NULL in turn: hues and henv among them
        bad = list(good)
        bad[i] = None
        assert call(*bad) == -1, i
    for n in (0, -3):
        bad = list(good)
        bad[1] = n
        assert call(*bad) == -1
    raw = lib.Params()
    L.crthip_params_default(C.byref(raw), 0, 1)
    assert call(C.byref(raw), *good[1:]) == -1             # not finalized
    pb = _base(lib, "ntscbloom")
    kin[1].noise = -1
    assert call(C.byref(pb), *good[1:]) == -1              # bloom: negative noise, as prepare7
    kin[1].noise = 24
    pn = lib.make_params("nes", w=256, h=240, outw=320, outh=240, out_format=lib.FMT_BGRA)
    assert call(C.byref(pn), *good[1:]) == -1              # the PPU encoder has no per-field instantiation
    kin[1].hue = 1 << 20                                   # (angle * 8192 must stay an int)
    assert call(*good) == -1
    kin[1].hue = -(1 << 20)
    assert call(*good) == -1
    kin[1].hue = -67
    assert call(*good) == 0
    for bad in (np.zeros((2, 7), dtype=np.int64), np.zeros((2, 9), dtype=np.int64), np.zeros((2, 8)), np.zeros((8,), dtype=np.int64)):
        with pytest.raises(ValueError):
            lib.knobs_prepare8(p, bad)


def test_carriers_stay_inside_the_fast_path_bound_for_every_hue(lib):
    """sn >> 10 of a sine scaled to 2^15: |carrier| <= 32, far inside encoder_fast_ok's 2048 -- prepare8 checks it all the same"""
    for name in ("ntsc", "snes", "nesrgb"):
        _, _, hues, _, _, _ = lib.knobs_prepare8(_base(lib, name), np.array([HU.D7 + (h,) for h in range(-400, 401, 7)]))
        assert int(np.abs(hues).max()) <= 32


def test_straddle_geometry_and_distinct_hues(lib):
    p = _base(lib)
    assert p.desth % 64 != 0 and p.desth > 64, "a wavefront of 64 rows holds rows of two fields"
    _, _, hues, _, _, _ = lib.knobs_prepare8(p, np.array(HU.BATCHES["straddle"]))
    assert len({bytes(h) for h in hues}) == len(hues) >= 3


@pytest.mark.parametrize("parity", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("name", ("ntsc", "vhslcg", "snes", "temp", "nesrgb"))
def test_margin_patch_model(lib, name, parity):
    """the set of (line, t) the HU margin kernels rewrite (HU.burst_positions: skeleton()'s burst predicate restated) equals the set
    where the oracle's clean signal differs between hues, outside the active rectangle: nothing but burst moves with the hue there,
    and every burst sample does for some pair of hues"""
    p = _base(lib, name)
    orc = R.Oracle(name)
    sd = orc.sys
    hues = (0, 180, 90, 45)
    rows = [HU.D7[:0] + (0,) + HU.D7[1:] + (h,) for h in hues]
    dco = [2 * parity[0] + parity[1] + 1] * len(hues)
    img = KC.image(HU.SMALL, 0)
    sig = []
    for r in rows:
        c = orc.new_crt(160, 120, R.FMT_BGRA)
        c.settings(np.concatenate([img, img[-1:]], axis=0), format=R.FMT_BGRA, w=64, h=48, as_color=1)
        c.sset("hue", r[7])
        if orc.system not in R.PROGRESSIVE_SYSTEMS:
            c.sset("field", parity[0])
            c.sset("frame", parity[1])
        if orc.system in R.DOT_CRAWL_SYSTEMS:
            c.sset("dot_crawl_offset", dco[0])
        c.analog[:] = 0
        c.modulate()
        sig.append(np.array(c.analog)[:sd.vres * sd.hres].reshape(sd.vres, sd.hres).copy())
    moved = np.zeros_like(sig[0], dtype=bool)
    for s in sig[1:]:
        moved |= s != sig[0]
    moved[p.yo:p.yo + p.desth, p.xo:p.xo + p.destw] = False
    got = {(int(n), int(t)) for n, t in zip(*np.nonzero(moved))}
    assert got == HU.burst_positions(name, p.yo), (name, parity, sorted(got ^ HU.burst_positions(name, p.yo))[:8])


def _all_batches():
    return dict(HU.BATCHES)


@pytest.mark.parametrize("cid", sorted(_all_batches()))
def test_oracle_against_the_compiled_reference_and_clear_of_its_over_read(cid):
    """the yardstick itself: the oracle per field with its eight knobs == the compiled reference, and no field of a GPU case sits in
    the reference's undefined over-read (the GPU tests exclude nothing)"""
    rows = _all_batches()[cid]
    want = HU.expected(("ntsc", cid, 2), lambda: HU.oracle_fields8("ntsc", HU.SMALL, rows, steps=2))
    assert not any(w["undefined"] for per in want for w in per)
    if not R.have_ref("ntsc"):
        pytest.skip("oracle/_ref not built")
    ref = R.RefLib("ntsc")
    for k, (noise, mon_hue, sat, brightness, contrast, black_point, white_point, hue) in enumerate(rows):
        c = ref.new_crt(HU.SMALL["outw"], HU.SMALL["outh"], R.FMT_BGRA)
        c.set("scanlines", 1)
        for a, v in (("hue", mon_hue), ("saturation", sat), ("brightness", brightness), ("contrast", contrast),
                     ("black_point", black_point), ("white_point", white_point)):
            c.set(a, v)
        img = KC.image(HU.SMALL, k)
        field, frame = KC.parity(k)
        c.settings(np.concatenate([img, img[-1:]], axis=0), format=R.FMT_BGRA, w=HU.SMALL["w"], h=HU.SMALL["h"], as_color=1,
                   field=field, frame=frame)
        c.sset("hue", hue)
        c.modulate()
        c.demodulate(noise)
        w = want[k][0]
        assert (c.get("hsync"), c.get("vsync"), c.get("rn")) == (w["hsync"], w["vsync"], w["rn"]), (cid, k)
        np.testing.assert_array_equal(c.inp[:w["inp"].shape[0]], w["inp"], err_msg="%s field %d inp" % (cid, k))
        np.testing.assert_array_equal(c.out, w["out"], err_msg="%s field %d" % (cid, k))


@pytest.mark.parametrize("name,n", [("vhs", 5), ("vhslcg", 6), ("snes", 6), ("temp", 6), ("nesrgb", 6), ("ntscp0", 4), ("ntscbloom", 6), ("ntscfir7", 4)])
def test_per_system_cases_are_clear_of_the_over_read(name, n):
    rows = HU.per_system(name, n)
    seeds = [3 + 11 * k for k in range(n)] if name == "vhs" else None
    want = HU.expected((name, "system", 2), lambda: HU.oracle_fields8(name, HU.SMALL, rows, steps=2, seeds=seeds))
    assert not any(w["undefined"] for per in want for w in per)
    if name in ("snes", "temp", "nesrgb"):
        assert sorted(HU.dot_crawl(name, k) for k in range(n)) == [0, 1, 2, 3, 4, 5] and min(r[7] for r in rows) < 0


@pytest.mark.parametrize("cid", sorted(HU.SEQ_CASES))
def test_sequence_loop_against_the_compiled_reference(cid):
    """the serial-loop construction of sequence mode: all eight knobs turned between the fields of ONE struct CRT"""
    case = HU.SEQ_CASES[cid]
    orc = HU.seq_expected(case)
    assert not any(w["undefined"] for w in orc)
    assert len({r[7] for r in case["rows"]}) >= 4          # the hue really changes mid-video
    if not R.have_ref(case["name"]):
        pytest.skip("oracle/_ref not built")
    ref = HU.seq_expected(case, R.RefLib(case["name"]))
    for k, (a, b) in enumerate(zip(ref, orc)):
        assert (a["hsync"], a["vsync"], a["rn"]) == (b["hsync"], b["vsync"], b["rn"]), (cid, k)
        np.testing.assert_array_equal(a["out"], b["out"], err_msg="%s field %d" % (cid, k))

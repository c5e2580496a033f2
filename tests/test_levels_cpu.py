"""CPU checks of the level knobs (crthip_knobs_prepare7, include/crt_hip.h; the GPU side is tests/test_gpu_levels.py): the two record
arrays against crthip_params_finalize per field, the env against crthip_knobs_prepare5's, the bounds of crthip_levels_env, the
refusals, the (n, 7) plumbing of crtlib without a device, a model of the encoder's dispatch bound, and the yardstick of the GPU
tests -- the oracle with seven knobs per field, the serial loop of sequence mode -- against the compiled reference."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import encoder_cases as EC
import knobs_cases as KC
import levels_cases as LV
import picknobs_cases as PK

SYSTEMS = ("ntsc", "ntscp0", "vhs", "vhslcg", "snes", "temp", "nesrgb", "ntscbloom")


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    R.build_oracle()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_knobs_prepare7"), "no crthip_knobs_prepare7 in this build"
    return crtlib


def _base(lib, name="ntsc", **kw):
    return lib.make_params(name, w=64, h=48, outw=160, outh=120, format=lib.FMT_BGRA, out_format=lib.FMT_BGRA, **kw)


def _all_batches(name="ntsc"):
    out = dict(LV.BATCHES)
    out.update({"bound-" + k: v for k, v in LV.bound_batches(name).items()})
    out["corners"] = LV.corner_rows(name)
    return out


def test_structs_and_abi(lib):
    assert (C.sizeof(lib.Knobs7), C.sizeof(lib.LevelRec), C.sizeof(lib.LevelsEnv)) == (32, 16, 32)
    assert lib.load_library().crthip_abi_version() == 6


@pytest.mark.parametrize("name", SYSTEMS)
def test_records_equal_finalize_per_field(lib, name):
    """white / ire_base / bright of every field = what crthip_params_finalize derives for a blob with that field's black and white
    point; the tier floor = the library's shared definition on that bright; the first five words = crthip_knobs_prepare's"""
    L = lib.load_library()
    rows = LV.per_system(name, 6) + LV.bound_batches(name)["white-"] + LV.EDGES
    if R.is_bloom(name):
        rows = [r for r in rows if r[0] >= 0]
    p = _base(lib, name)
    recs, levs, env, lenv = lib.knobs_prepare7(p, np.array(rows, dtype=np.int64))
    recs3, _ = lib.knobs_prepare(p, np.array([r[:3] for r in rows]))
    np.testing.assert_array_equal(recs[:, :5], recs3[:, :5])
    floors, brights = [], []
    for k, r in enumerate(rows):
        q = _base(lib, name, brightness=r[3], contrast=r[4], black_point=r[5], white_point=r[6])
        assert (levs[k, lib.LEV_WHITE], levs[k, lib.LEV_IRE_BASE]) == (q.white, q.ire_base) == LV.levels_of(name, r), (name, k, r)
        assert not levs[k, 2:].any()
        assert recs[k, lib.REC_BRIGHT] == q.bright == r[3] - q.ire_base and recs[k, lib.REC_CONTRAST] == r[4]
        fl = L.crt_setup_decoder_floor(C.byref(q), q.bright, q.contrast)
        assert recs[k, lib.REC_TIER_FLOOR] == fl
        floors.append(fl)
        brights.append(q.bright)
    assert env.pic == 1 and (env.tier_floor_min, env.tier_floor_max) == (min(floors), max(floors))
    assert env.bright_abs_lo == max([abs(b) for b, f in zip(brights, floors) if f < 2] or [0])
    assert (lenv.n, lenv.white_abs_max, lenv.ire_base_abs_max) == (len(rows), int(np.abs(levs[:, 0]).max()), int(np.abs(levs[:, 1]).max()))
    assert not any(lenv.reserved) and lenv.magic != env.magic and lenv.magic != 0


def test_edge_rows_cross_the_tier_bound_one_field_each(lib):
    """the black point alone moves ONE field over +-2600 | +-2601; its neighbours stay in tier 0"""
    p = _base(lib)
    for cid in ("edges", "edges-neg"):
        recs, _, env, _ = lib.knobs_prepare7(p, np.array(LV.BATCHES[cid]))
        assert recs[:, lib.REC_TIER_FLOOR].tolist() == LV.EDGE_FLOORS[cid]
        assert [PK.floor_of(r[3] - 7 - r[5], r[4]) for r in LV.BATCHES[cid]] == LV.EDGE_FLOORS[cid]
    recs, _, _, _ = lib.knobs_prepare7(p, np.array(LV.EDGES))
    assert recs[4:, lib.REC_BRIGHT].tolist() == [2600, 2601]
    recs, _, _, _ = lib.knobs_prepare7(p, np.array(LV.EDGES_NEG))
    assert recs[1:3, lib.REC_BRIGHT].tolist() == [-2600, -2601]


@pytest.mark.parametrize("name", ("ntsc", "snes", "vhs"))
def test_env_equals_prepare5_s_when_all_levels_are_the_blob_s(lib, name):
    p = _base(lib, name, black_point=-4, white_point=93, brightness=11, contrast=170)
    rows5 = [t + pc for t, pc in zip(KC.SMALL_TRIPLES, [(0, 180), (2608, 120), (-40, 240), (0, 1 << 23), (33, 90), (0, -200)])]
    r5, e5 = lib.knobs_prepare(p, np.array(rows5))
    r7, l7, e7, lenv = lib.knobs_prepare7(p, np.array([r + (-4, 93) for r in rows5]))
    np.testing.assert_array_equal(r5, r7)
    assert bytes(e5) == bytes(e7)
    assert (l7[:, 0] == p.white).all() and (l7[:, 1] == p.ire_base).all()
    assert (lenv.white_abs_max, lenv.ire_base_abs_max) == (abs(p.white), abs(p.ire_base))
    # ... and through the one door of crtlib: the (n, 7) array gives the same records, with the level arrays on the env
    r7b, e7b = lib.knobs_prepare(p, np.array([r + (-4, 93) for r in rows5]))
    np.testing.assert_array_equal(r7b, r7)
    np.testing.assert_array_equal(e7b.levs, l7)
    assert bytes(e7b) == bytes(e7) and bytes(e7b.lenv) == bytes(lenv) and not hasattr(e5, "levs")


def test_blob_s_own_levels_are_ignored(lib):
    rows = np.array(LV.STRADDLE)
    a = lib.knobs_prepare7(_base(lib), rows)
    b = lib.knobs_prepare7(_base(lib, black_point=55, white_point=-3), rows)
    for x, y in zip(a, b):
        assert bytes(x) == bytes(y) if not isinstance(x, np.ndarray) else np.array_equal(x, y)


def test_loskip_bound_is_the_widest_range_over_the_fields(lib):
    """RGB encoders clamp the level to 0 .. 110 whatever the pair: the bound is prepare5's at the same noises.  The PPU encoder's
    range depends on the pair: the bound over the fields is the smallest of the single fields' (host-only: such a call is refused
    on the device, the bound is still what the contract says)"""
    p = _base(lib)
    _, e5 = lib.knobs_prepare(p, np.array([r[:5] for r in LV.COMBINED]))
    _, _, e7, _ = lib.knobs_prepare7(p, np.array(LV.COMBINED))
    assert e7.loskip_wave_max == e5.loskip_wave_max
    pn = lib.make_params("nes", w=256, h=240, outw=320, outh=240, out_format=lib.FMT_BGRA)
    rows = [(10, 0, 10, 0, 180, 0, 100), (10, 0, 10, 0, 180, 0, 400), (10, 0, 10, 0, 180, 30000, 100)]
    single = [lib.knobs_prepare7(pn, np.array([r]))[2].loskip_wave_max for r in rows]
    assert lib.knobs_prepare7(pn, np.array(rows))[2].loskip_wave_max == min(single)
    assert len(set(single)) > 1


def test_refusals(lib):
    L = lib.load_library()
    p = _base(lib)
    kin = (lib.Knobs7 * 2)()
    for k in range(2):
        kin[k].noise, kin[k].saturation, kin[k].contrast, kin[k].white_point = 24, 10, 180, 100
    recs, levs = (lib.KnobRec * 2)(), (lib.LevelRec * 2)()
    env, lenv = lib.KnobsEnv(), lib.LevelsEnv()
    call = L.crthip_knobs_prepare7
    assert call(C.byref(p), 2, kin, recs, levs, C.byref(env), C.byref(lenv)) == 0
    assert call(C.byref(p), 0, kin, recs, levs, C.byref(env), C.byref(lenv)) == -1
    assert call(C.byref(p), -3, kin, recs, levs, C.byref(env), C.byref(lenv)) == -1
    assert call(None, 2, kin, recs, levs, C.byref(env), C.byref(lenv)) == -1
    assert call(C.byref(p), 2, None, recs, levs, C.byref(env), C.byref(lenv)) == -1
    assert call(C.byref(p), 2, kin, None, levs, C.byref(env), C.byref(lenv)) == -1
    assert call(C.byref(p), 2, kin, recs, None, C.byref(env), C.byref(lenv)) == -1
    assert call(C.byref(p), 2, kin, recs, levs, None, C.byref(lenv)) == -1
    assert call(C.byref(p), 2, kin, recs, levs, C.byref(env), None) == -1
    raw = lib.Params()
    L.crthip_params_default(C.byref(raw), 0, 1)
    assert call(C.byref(raw), 2, kin, recs, levs, C.byref(env), C.byref(lenv)) == -1          # not finalized
    pb = _base(lib, "ntscbloom")
    kin[1].noise = -1
    assert call(C.byref(pb), 2, kin, recs, levs, C.byref(env), C.byref(lenv)) == -1           # bloom: negative noise, as prepare5
    assert call(C.byref(p), 2, kin, recs, levs, C.byref(env), C.byref(lenv)) == 0
    for bad in (np.zeros((2, 6), dtype=np.int64), np.zeros((2, 8), dtype=np.int64), np.zeros((2, 7)), np.zeros((7,), dtype=np.int64)):
        with pytest.raises(ValueError):
            lib.knobs_prepare(p, bad)
        with pytest.raises(ValueError):
            lib.knobs_prepare7(p, bad)


def test_dispatch_bound_model(lib):
    """what encoder_fast_ok decides by for a call with levels: lenv's maxima, both below 2^13 -- the batch inside the bound is, every
    batch with one field outside is not; the cases sit exactly on 8191 | 8192"""
    for name in ("ntsc", "snes", "nesrgb", "vhs"):
        p = _base(lib, name)
        for cid, rows in LV.bound_batches(name).items():
            _, levs, _, lenv = lib.knobs_prepare7(p, np.array(rows))
            fast = lenv.white_abs_max < LV.FAST_WHITE and lenv.ire_base_abs_max < LV.FAST_IRE
            assert fast == LV.fast_model(name, rows) == (cid == "inside"), (name, cid)
            assert max(lenv.white_abs_max, lenv.ire_base_abs_max) == (8191 if cid == "inside" else 8192)
            if cid != "inside":
                over = (np.abs(levs[:, 0]) >= LV.FAST_WHITE) | (np.abs(levs[:, 1]) >= LV.FAST_IRE)
                assert over.sum() == 1, "a single field outside the bound"
    assert LV.fast_model("ntsc", LV.corner_rows("ntsc"))


def test_straddle_geometry_and_distinct_pairs(lib):
    p = _base(lib)
    assert p.desth % 64 != 0 and p.desth > 64, "a wavefront of 64 rows holds rows of two fields"
    pairs = [LV.levels_of("ntsc", r) for r in LV.STRADDLE]
    assert len(set(pairs)) == len(pairs) >= 3


@pytest.mark.parametrize("cid", sorted(_all_batches()))
def test_oracle_against_the_compiled_reference_and_clear_of_its_over_read(cid):
    """the yardstick itself: the oracle per field with its seven knobs == the compiled reference, and no field of a GPU case sits in
    the reference's undefined over-read (the GPU tests exclude nothing)"""
    rows = _all_batches()[cid]
    images = LV.corner_images(LV.SMALL) if cid == "corners" else None
    want = LV.expected(("ntsc", cid, 2), lambda: LV.oracle_fields7("ntsc", LV.SMALL, rows, steps=2, images=images))
    assert not any(w["undefined"] for per in want for w in per)
    if not R.have_ref("ntsc"):
        pytest.skip("oracle/_ref not built")
    ref = R.RefLib("ntsc")
    for k, (noise, hue, sat, brightness, contrast, black_point, white_point) in enumerate(rows):
        c = ref.new_crt(LV.SMALL["outw"], LV.SMALL["outh"], R.FMT_BGRA)
        c.set("scanlines", 1)
        for a, v in (("hue", hue), ("saturation", sat), ("brightness", brightness), ("contrast", contrast),
                     ("black_point", black_point), ("white_point", white_point)):
            c.set(a, v)
        img = images[k] if images is not None else KC.image(LV.SMALL, k)
        field, frame = KC.parity(k)
        c.settings(np.concatenate([img, img[-1:]], axis=0), format=R.FMT_BGRA, w=LV.SMALL["w"], h=LV.SMALL["h"], as_color=1,
                   field=field, frame=frame)
        c.modulate()
        c.demodulate(noise)
        w = want[k][0]
        assert (c.get("hsync"), c.get("vsync"), c.get("rn")) == (w["hsync"], w["vsync"], w["rn"]), (cid, k)
        np.testing.assert_array_equal(c.inp[:w["inp"].shape[0]], w["inp"], err_msg="%s field %d inp" % (cid, k))
        np.testing.assert_array_equal(c.out, w["out"], err_msg="%s field %d" % (cid, k))


@pytest.mark.parametrize("cid", sorted(LV.SEQ_CASES))
def test_sequence_loop_against_the_compiled_reference(cid):
    """the serial-loop construction of sequence mode: all seven knobs turned between the fields of ONE struct CRT"""
    case = LV.SEQ_CASES[cid]
    orc = LV.seq_expected(case)
    assert not any(w["undefined"] for w in orc)
    assert len({r[5:] for r in case["rows"]}) >= 4          # the levels really change mid-video
    if not R.have_ref(case["name"]):
        pytest.skip("oracle/_ref not built")
    ref = LV.seq_expected(case, R.RefLib(case["name"]))
    for k, (a, b) in enumerate(zip(ref, orc)):
        assert (a["hsync"], a["vsync"], a["rn"]) == (b["hsync"], b["vsync"], b["rn"]), (cid, k)
        np.testing.assert_array_equal(a["out"], b["out"], err_msg="%s field %d" % (cid, k))

"""CPU checks of the picture knobs (crthip_knobs_prepare5, include/crt_hip.h; the GPU side is tests/test_gpu_picknobs.py): the records
and bounds against a Python restatement at every bound the code branches on, the refusals, that crthip_knobs_prepare gives what it
gave, and the yardstick of the GPU tests -- the oracle with five knobs per field -- against the compiled reference."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import knobs_cases as KC
import picknobs_cases as PK


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    R.build_oracle()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_knobs_prepare5")
    return crtlib


def _base(lib, name="ntsc", **kw):
    return lib.make_params(name, w=64, h=48, outw=160, outh=120, format=lib.FMT_BGRA, out_format=lib.FMT_BGRA, **kw)


def test_structs_and_abi(lib):
    assert (C.sizeof(lib.Knobs5), C.sizeof(lib.KnobRec), C.sizeof(lib.KnobsEnv)) == (32, 32, 32)
    assert lib.load_library().crthip_abi_version() == 6


def test_the_hand_made_floors_are_the_formula_s():
    for cid, rows in PK.BOUND_CASES.items():
        assert [PK.floor_of(r[3] - 7, r[4]) for r in rows] == PK.FLOORS[cid], cid
    assert sorted({f for fl in PK.FLOORS.values() for f in fl}) == [0, 2, 3]


@pytest.mark.parametrize("cid", sorted(PK.BOUND_CASES))
def test_records_against_the_restatement(lib, cid):
    """bright as crthip_params_finalize derives it, contrast, the tier floor of decoder_min_tier's formula at every bound; the first
    five words are crthip_knobs_prepare's; the env's flag, smallest / largest floor and largest tier-0 |bright|"""
    rows = PK.BOUND_CASES[cid]
    p = _base(lib)
    # the formula's coefficient conditions hold for this blob (PK.floor_of leaves them out)
    assert 32768 <= p.eq_lf[0] < 98304 and 32768 <= p.eq_hf[0] < 98304
    assert all(0 < p.eq_lf[k] < 32768 and 0 < p.eq_hf[k] < 32768 for k in (1, 2))
    recs, env = lib.knobs_prepare(p, np.array(rows, dtype=np.int64))
    recs3, env3 = lib.knobs_prepare(p, np.array([r[:3] for r in rows]))
    np.testing.assert_array_equal(recs[:, :5], recs3[:, :5])
    black = 7 + p.black_point
    floors = []
    for k, r in enumerate(rows):
        bright = r[3] - black
        q = _base(lib, brightness=r[3], contrast=r[4])
        assert q.bright == bright
        assert recs[k, lib.REC_BRIGHT] == bright and recs[k, lib.REC_CONTRAST] == r[4], (cid, k)
        assert recs[k, lib.REC_TIER_FLOOR] == PK.floor_of(bright, r[4]) == PK.FLOORS[cid][k], (cid, k, r)
        # ... and the library's own shared definition, called like decoder_min_tier calls it
        assert lib.load_library().crt_setup_decoder_floor(C.byref(q), q.bright, q.contrast) == PK.FLOORS[cid][k]
        floors.append(PK.FLOORS[cid][k])
    assert (env.magic, env.n, env.noise_max, env.sat_abs_max, env.loskip_wave_max) == \
           (env3.magic, env3.n, env3.noise_max, env3.sat_abs_max, env3.loskip_wave_max)
    assert env.pic == 1 and (env.tier_floor_min, env.tier_floor_max) == (min(floors), max(floors))
    assert env.bright_abs_lo == max([abs(r[3] - black) for r, f in zip(rows, floors) if f < 2] or [0])
    assert env.bright_abs_lo <= PK.T0_BRIGHT_MAX


def test_black_point_enters_bright(lib):
    p = _base(lib, black_point=5)
    recs, _ = lib.knobs_prepare(p, np.array([(0, 0, 10, 2612, 180), (0, 0, 10, 2613, 180)]))
    assert recs[:, lib.REC_BRIGHT].tolist() == [2600, 2601] and recs[:, lib.REC_TIER_FLOOR].tolist() == [0, 2]


def test_uniform_picture_values_give_prepare_s_first_five_words(lib):
    p = _base(lib, brightness=-12, contrast=222)
    trip = KC.SMALL_TRIPLES
    r5, e5 = lib.knobs_prepare(p, np.array([t + (-12, 222) for t in trip]))
    r3, e3 = lib.knobs_prepare(p, np.array(trip))
    np.testing.assert_array_equal(r5[:, :5], r3[:, :5])
    assert (r5[:, lib.REC_BRIGHT] == p.bright).all() and (r5[:, lib.REC_CONTRAST] == 222).all() and not r5[:, lib.REC_TIER_FLOOR].any()
    assert bytes(e5)[:20] == bytes(e3)[:20]


def test_prepare_keeps_its_reserved_words_zero(lib):
    """no existing behaviour changes: records and env of crthip_knobs_prepare carry no picture knobs, whatever the blob's own"""
    p = _base(lib, brightness=5000, contrast=1 << 23)
    recs, env = lib.knobs_prepare(p, np.array(KC.SMALL_TRIPLES))
    assert not recs[:, 5:].any() and not any(env.reserved)
    assert (env.pic, env.tier_floor_min, env.tier_floor_max, env.bright_abs_lo) == (0, 0, 0, 0)


def test_refusals(lib):
    L = lib.load_library()
    p = _base(lib)
    kin = (lib.Knobs5 * 2)()
    for k in range(2):
        kin[k].noise, kin[k].saturation, kin[k].contrast = 24, 10, 180
    recs = (lib.KnobRec * 2)()
    env = lib.KnobsEnv()
    call = L.crthip_knobs_prepare5
    assert call(C.byref(p), 2, kin, recs, C.byref(env)) == 0
    assert call(C.byref(p), 0, kin, recs, C.byref(env)) == -1
    assert call(C.byref(p), -3, kin, recs, C.byref(env)) == -1
    assert call(None, 2, kin, recs, C.byref(env)) == -1
    assert call(C.byref(p), 2, None, recs, C.byref(env)) == -1
    assert call(C.byref(p), 2, kin, None, C.byref(env)) == -1
    assert call(C.byref(p), 2, kin, recs, None) == -1
    raw = lib.Params()
    L.crthip_params_default(C.byref(raw), 0, 1)
    assert call(C.byref(raw), 2, kin, recs, C.byref(env)) == -1          # not finalized
    pb = _base(lib, "ntscbloom")
    kin[1].noise = -1
    assert call(C.byref(pb), 2, kin, recs, C.byref(env)) == -1           # bloom: negative noise, as crthip_knobs_prepare
    assert call(C.byref(p), 2, kin, recs, C.byref(env)) == 0
    for bad in (np.zeros((2, 4), dtype=np.int64), np.zeros((2, 5)), np.zeros((5,), dtype=np.int64)):
        with pytest.raises(ValueError):
            lib.knobs_prepare(p, bad)


@pytest.mark.parametrize("cid", sorted(PK.BOUND_CASES))
def test_oracle_against_the_compiled_reference_and_clear_of_its_over_read(cid):
    """the yardstick itself: the oracle per field with its five knobs == the compiled reference, and no field of a GPU case sits in
    the reference's undefined over-read (the GPU tests exclude nothing)"""
    rows = PK.BOUND_CASES[cid]
    want = PK.expected(("ntsc", cid, 2), lambda: PK.oracle_fields5("ntsc", PK.SMALL, rows, steps=2))
    assert not any(w["undefined"] for per in want for w in per)
    if not R.have_ref("ntsc"):
        pytest.skip("oracle/_ref not built")
    ref = R.RefLib("ntsc")
    for k, (noise, hue, sat, brightness, contrast) in enumerate(rows):
        c = ref.new_crt(PK.SMALL["outw"], PK.SMALL["outh"], R.FMT_BGRA)
        c.set("scanlines", 1)
        for a, v in (("hue", hue), ("saturation", sat), ("brightness", brightness), ("contrast", contrast)):
            c.set(a, v)
        img = KC.image(PK.SMALL, k)
        field, frame = KC.parity(k)
        c.settings(np.concatenate([img, img[-1:]], axis=0), format=R.FMT_BGRA, w=PK.SMALL["w"], h=PK.SMALL["h"], as_color=1,
                   field=field, frame=frame)
        c.modulate()
        c.demodulate(noise)
        w = want[k][0]
        assert (c.get("hsync"), c.get("vsync"), c.get("rn")) == (w["hsync"], w["vsync"], w["rn"]), (cid, k)
        np.testing.assert_array_equal(c.out, w["out"], err_msg="%s field %d" % (cid, k))


@pytest.mark.parametrize("cid", sorted(PK.SEQ_CASES))
def test_sequence_loop_against_the_compiled_reference(cid):
    case = PK.SEQ_CASES[cid]
    orc = PK.seq_expected(case)
    assert not any(w["undefined"] for w in orc)
    if not R.have_ref(case["name"]):
        pytest.skip("oracle/_ref not built")
    ref = PK.seq_expected(case, R.RefLib(case["name"]))
    for k, (a, b) in enumerate(zip(ref, orc)):
        assert (a["hsync"], a["vsync"], a["rn"]) == (b["hsync"], b["vsync"], b["rn"]), (cid, k)
        np.testing.assert_array_equal(a["out"], b["out"], err_msg="%s field %d" % (cid, k))


def test_sequence_cases_cross_the_tier_bounds_mid_video():
    floors = [PK.floor_of(r[3] - 7, r[4]) for r in PK.SEQ_RAMP]
    assert floors == [0, 0, 0, 2, 3, 0]

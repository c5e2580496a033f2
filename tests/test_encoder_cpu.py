"""What the hand-made images of tests/encoder_cases.py claim to reach, proven without a GPU: the oracle against the real reference on
every case; the colour extremes, clamp ends, floor residues and the NES's -128 on the oracle's analog[]; a Python model of the
encoder's dispatch bound on crthip_params; the source-column step for every width the table uses."""
import numpy as np
import pytest

import crtref as R
import encoder_cases as E

needs_ref = pytest.mark.skipif(not R.have_ref("ntsc"), reason="oracle/_ref not built (no reference sources on this machine)")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def _params(lib, cid, noise=None):
    case = E.CASES[cid]
    imgs = E.images(cid)
    nz = E.noises(case)
    kw = dict(w=int(imgs.shape[2]), h=int(imgs.shape[1]), outw=E.OUTW, outh=E.OUTH, out_format=E.OUTFMT, hue=case["hue"],
              xoffset=case["xoffset"], noise=nz[0] if noise is None else noise)
    if not E.is_nes(case["name"]):
        kw["format"] = case["fmt"]
        kw["raw"] = case["raw"]
    kw.update(case["knobs"])
    return lib.make_params(case["name"], **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the oracle is the reference on every case
# ---------------------------------------------------------------------------------------------------------------------------
# The reference computes in `int`.  On the RGB systems no product of these cases leaves 32 bits: |y + i + q| <= 2161 times |white| <=
# 8192 is below 2^25, (byte - 0x7f) * noise at |noise| <= 32768 below 2^23.  On the NES the sample is (ire * white_point / 100) >> 12
# with |ire| up to 4 * 112965 + black: at the white points of the knob table (|white_point| ~ 7447) and at ire_base = +-8192 the
# product leaves 32 bits -- undefined in C, wrapping in the oracle by contract (-fwrapv).  The pinned build of the reference wraps the
# same way on every such case, so no case carries the gpu_only mark.
@needs_ref
@pytest.mark.parametrize("cid", sorted(E.CASES))
def test_oracle_equals_the_reference(cid):
    case = E.CASES[cid]
    assert case["gpu_only"] is None, "the aim is that no case needs the mark: " + str(case["gpu_only"])
    if not R.have_ref(case["name"]):
        pytest.skip("no reference build of " + case["name"])
    want = E.expected(cid)
    got = E.run_checker(R.RefLib(case["name"]), cid)
    for k in range(case["n"]):
        for step in range(E.STEPS):
            o, r = want[k][step], got[k][step]
            what = "%s field %d pass %d " % (cid, k, step)
            np.testing.assert_array_equal(r["analog"], o["analog"], err_msg=what + "analog")
            np.testing.assert_array_equal(r["ccf_mod"], o["ccf_mod"], err_msg=what + "ccf after modulate")
            np.testing.assert_array_equal(r["inp"], o["inp"], err_msg=what + "inp")
            assert r["rn"] == o["rn"], what + "rn"
            if o["undefined"]:
                break
            np.testing.assert_array_equal(r["ccf"], o["ccf"], err_msg=what + "ccf")
            assert (r["hsync"], r["vsync"]) == (o["hsync"], o["vsync"]), what + "hsync, vsync"
            np.testing.assert_array_equal(r["out"], o["out"], err_msg=what + "out")


def test_shapes_and_exclusions():
    """2 .. 4 fields, both field parities, both frame values over the table; no field drops out outside the noise-edge cases"""
    for cid, case in E.CASES.items():
        imgs = E.images(cid)
        assert 2 <= case["n"] <= 4, cid
        if case["family"] not in ("geometry", "kn", "nes") and not E.is_nes(case["name"]):
            assert 8 <= imgs.shape[1] <= 48, cid
        if not E.is_progressive(case["name"]):
            assert {E.field_of(k, s) for k in range(case["n"]) for s in range(E.STEPS)} == {0, 1}
        if not E.is_noise_edge(case):
            want = E.expected(cid)
            assert not any(r["undefined"] for per in want for r in per), cid
    assert {E.frame_of(k) for k in range(4)} == {0, 1}
    assert {E.CASES[c]["name"] for c in E.CASES} == set(E.SYSTEMS)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. each family reaches what it names
# ---------------------------------------------------------------------------------------------------------------------------
def test_extreme_colours_are_the_extremes_of_all_colours():
    """per-colour Y, I and Q (sum >> 14) of the cube's corners against the minima and maxima over all 2^24 colours, computed here"""
    sy, si, sq = (s.astype(np.int64) >> 14 for s in E.colour_sums())

    def yiq(rgb):
        return tuple(int(sum(k * c for k, c in zip(coef, rgb))) >> 14 for coef in (E.KY, E.KI, E.KQ))
    corners = [yiq(c) for c in E.CORNERS]
    assert (min(c[0] for c in corners), max(c[0] for c in corners)) == (int(sy.min()), int(sy.max()))
    assert (min(c[1] for c in corners), max(c[1] for c in corners)) == (int(si.min()), int(si.max()))
    assert (min(c[2] for c in corners), max(c[2] for c in corners)) == (int(sq.min()), int(sq.max()))
    assert yiq(E.COLOURS["I"])[1] == int(si.max()) and yiq(E.COLOURS["i"])[1] == int(si.min())
    assert yiq(E.COLOURS["Q"])[2] == int(sq.max()) and yiq(E.COLOURS["q"])[2] == int(sq.min())
    assert yiq(E.COLOURS["W"])[0] == int(sy.max()) and yiq(E.COLOURS["K"])[0] == int(sy.min()) == 0
    assert all(tuple(E.COLOURS[ch]) in E.CORNERS for ch in "IiQqWK")
    # every run length at every start, with either colour first, for every pair of opposite corners (ntsc: four variants)
    seen = {(p, (r + 48 * v) % 80, v >> 1) for v in range(4) for p in range(4) for r in range(48)}
    assert seen == {(p, i, pol) for p in range(4) for i in range(80) for pol in (0, 1)}
    assert {(r + 48 * v) % 80 for v in range(2) for r in range(48)} == set(range(80))      # the other systems: two variants
    for run, start in E.RUN_ROWS:
        row = E.runs_image(80, 80, 0, 0)[E.RUN_ROWS.index((run, start))]
        edges = np.flatnonzero((row[1:] != row[:-1]).any(axis=1)) + 1
        assert start in edges or start == 0 and (row[0] == 0).all(), (run, start)
        assert (np.diff(edges) == run).all()


REACH = sorted(c for c, case in E.CASES.items() if case["family"] in ("extremes", "phase") and not case["knobs"])


@pytest.mark.parametrize("cid", REACH)
def test_extremes_and_phase_cases_reach_both_clamp_ends(lib, cid):
    """default white point: analog[] holds 0 and 110 inside the encoder's rectangle (the blanking level is 0 too, so only there)"""
    case = E.CASES[cid]
    p = _params(lib, cid)
    orc = E.oracle(case["name"])
    if case["raw"] == 0:
        assert p.destw == E.destw(case["name"])
        assert E.images(cid).shape[2] == p.destw, "a 1:1 image"
    seen = set()
    for per in E.expected(cid):
        for r in per:
            a = np.concatenate([r["analog"], np.zeros(orc.hres, dtype=np.int8)])[:(orc.input_size // orc.hres) * orc.hres]
            rect = a.reshape(-1, orc.hres)[p.yo:p.yo + p.desth, p.xo:min(p.xo + p.destw, orc.hres)]
            seen |= set(np.unique(rect).tolist())
    assert 0 in seen and 110 in seen, (cid, min(seen), max(seen))
    assert min(seen) >= 0 and max(seen) <= 110


def test_floors_image_holds_every_residue_class():
    """I and Q: sums of both signs at residues 0, 1, 16383, 16382 (and +-2); Y sums are never negative (asserted), so one sign"""
    img = E.floors_image().reshape(-1, 3).astype(np.int64)
    assert img.shape[0] < 64 * 48
    assert int(E.colour_sums()[0].min()) == 0            # no colour has a negative Y sum: one sign to look for
    for ch, coef in zip("YIQ", (E.KY, E.KI, E.KQ)):
        s = img @ np.array(coef, dtype=np.int64)
        for res in (0, 1, 16383, 16382):
            hit = s[(s % 16384) == res]
            assert (hit >= 0).any(), (ch, res)
            if ch != "Y":
                assert (hit < 0).any(), (ch, res)
    grey = img[(img[:, 0] == img[:, 1]) & (img[:, 1] == img[:, 2])]
    assert set(grey[:, 0].tolist()) == set(range(256))
    for cid in ("ntsc-floors", "ntsc-floors-rgb", "ntsc-floors-argb", "snes-floors", "snes-floors-rgba"):
        # the image arrives in the case's byte order with alternating alpha
        arr, fmt = E.images(cid)[0], E.CASES[cid]["fmt"]
        back = {R.FMT_RGB: (0, 1, 2), R.FMT_BGR: (2, 1, 0), R.FMT_ARGB: (1, 2, 3), R.FMT_RGBA: (0, 1, 2), R.FMT_ABGR: (3, 2, 1),
                R.FMT_BGRA: (2, 1, 0)}[fmt]
        np.testing.assert_array_equal(arr[..., list(back)].reshape(-1, 3), E.floors_image().reshape(-1, 3))
        if arr.shape[-1] == 4:
            alpha = arr[..., 0 if fmt in (R.FMT_ARGB, R.FMT_ABGR) else 3]
            assert set(alpha.reshape(-1).tolist()) == {0, 255} and (alpha[:, 1:] != alpha[:, :-1]).all()


# (white 8191 on the ramp and white -8192 on the narrow random images happen not to wrap onto -128: the narrow widths have cases of their own)
NES_EXTREME = ["nes-white8192", "nes-white-8191", "nes-white-8192", "nes-minus128-w8", "nes-minus128-w7", "nes-minus128-w4",
               "nes-minus128-w8-noise0", "nes-minus128-w7-noise0", "nes-minus128-w4-noise0", "nes-minus128-ramp-noise0"]


@pytest.mark.parametrize("cid", NES_EXTREME)
def test_nes_cases_at_extreme_knobs_hold_minus_128(cid):
    """-128 in analog[]: the value the fused path's CLAMP exists for (crt_core.c:363-364 brings it to -127 in inp[])"""
    assert NES_EXTREME
    lo = min(int(r["analog"].min()) for per in E.expected(cid) for r in per)
    assert lo == -128, (cid, lo)
    for per in E.expected(cid):
        for r in per:
            assert int(r["inp"].min()) >= -127


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a model of the dispatch bound
# ---------------------------------------------------------------------------------------------------------------------------
def model_fast_ok(lib, p):
    """encoder_fast_ok, crt_encode.hip:1226-1233, restated on crthip_params alone:
        ok = |white| < (1 << 13) && |ire_base| < (1 << 13) && |noise| < (1 << 15);  HIPASS: never;
        every modI / modQ inside +-2048;  band-limited systems: 0 < iir_c[0] <= 2048 in the form the system was compiled for
        ((iir_c[0] >= 1024) == IIR_Y_NEAR: every system but the VHS), 0 < iir_c[1], iir_c[2] < 1024"""
    ok = abs(p.white) < (1 << 13) and abs(p.ire_base) < (1 << 13) and abs(p.noise) < (1 << 15)
    if p.flags & lib.F_HIPASS:
        ok = False
    for r in range(lib.CARRIER_ROWS):
        for k in range(lib.MAX_CCS):
            ok = ok and -2048 < p.modI[r][k] < 2048 and -2048 < p.modQ[r][k] < 2048
    # S::BANDLIMIT is no member of crthip_params: this rests on crthip_params_finalize zeroing iir_c and filling it only for systems
    # with low-pass frequencies (crt_setup.c, `if (d.y_freq != 0)`), i.e. exactly where CRT_DO_BANDLIMITING is 1
    if any(p.iir_c):
        y_near = p.system != lib.SYSTEM_VHS
        ok = ok and 0 < p.iir_c[0] <= 2048 and (p.iir_c[0] >= 1024) == y_near and 0 < p.iir_c[1] < 1024 and 0 < p.iir_c[2] < 1024
    return bool(ok)


def test_dispatch_model_places_every_case(lib):
    sides = {}
    for cid, case in E.CASES.items():
        for nz in sorted(set(E.noises(case))):
            p = _params(lib, cid, noise=nz)
            white, ire, want = E.intended(case, nz)
            assert (p.white, p.ire_base, p.noise) == (white, ire, nz), "%s: the knobs do not give what the table means" % cid
            assert model_fast_ok(lib, p) == want, (cid, nz, p.white, p.ire_base, p.noise)
            sides.setdefault(case["name"], set()).add((p.white, p.ire_base, p.noise, want))
    for name in ("ntsc", "snes", "pv1k", "vhslcg", "ntscbloom", "temp", "ntscp0", "nesrgb"):
        s = sides[name]
        white = {w: ok for w, i, n, ok in s if i == E.oracle(name).sys.black_level and abs(n) < 100}
        assert white[8191] is True and white[8192] is False and white[-8192] is False, name
        ire = {i: ok for w, i, n, ok in s if w == E.oracle(name).sys.white_level and abs(n) < 100}
        assert ire[8191] is True and ire[-8191] is True and ire[-8192] is False, name
        noise = {n: ok for w, i, n, ok in s if w == E.oracle(name).sys.white_level and i == E.oracle(name).sys.black_level}
        assert noise[32767] is True and noise[32768] is False, name
    s = sides["ntsc"]
    assert {w for w, i, n, ok in s} >= set(E.WHITES) and {i for w, i, n, ok in s} >= set(E.IRES) and {n for w, i, n, ok in s} >= set(E.NOISES)
    assert (8191, 8191, 32767, True) in s and (-8191, -8191, -32767, True) in s
    assert all(ok is False for w, i, n, ok in sides["ntschipass"]) and len(sides["ntschipass"]) >= 6


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the source column
# ---------------------------------------------------------------------------------------------------------------------------
def test_source_column_step_for_every_width_of_the_table(lib):
    """crthip_params.col_step (see test_abi_cpu.py: test_source_column_step_is_exact) for every destw the case table produces against
    every w it uses and 2^k +- 1 for k up to 24, all x < destw (+ 3: the tiled path runs up to 3 samples over)"""
    geoms = {}
    for cid, case in E.CASES.items():
        if E.is_nes(case["name"]):
            continue                                     # (the NES kernels walk the column by quotient and remainder)
        p = _params(lib, cid)
        geoms.setdefault((case["name"], case["raw"], p.destw), set()).add(int(E.images(cid).shape[2]))
    widths = sorted(set().union(*geoms.values()) | {(1 << k) + d for k in range(1, 25) for d in (-1, 1)})
    assert {E.destw("ntsc"), E.destw("ntscbloom"), E.destw("pv1k"), 200, 33} <= {d for _, _, d in geoms}
    for (name, raw, dw), own in sorted(geoms.items()):
        for w in (sorted(own) if raw else widths):       # raw: destw follows w, the pair is the case's own
            p = lib.make_params(name, w=w, h=8, outw=E.OUTW, outh=E.OUTH, raw=raw)
            assert p.destw == dw, (name, raw, w)
            step = (p.col_step_hi << 32) | p.col_step_lo
            assert step == -((-(w << 32)) // dw)
            x = np.arange(dw + 3, dtype=np.uint64)
            np.testing.assert_array_equal((x * np.uint64(step)) >> np.uint64(32), (x * np.uint64(w)) // np.uint64(dw), err_msg=str((name, w, dw)))


def test_the_pinned_set_covers_what_it_says():
    """the cases test_gpu_encoder.py pins every instantiation on: every family, the widths on either side of the image-tile switch and
    of the NES's narrow loop, 3- and 4-byte pixels, per-field noise with all four values in one batch"""
    assert all(c in E.CASES for c in E.PINNED) and len(set(E.PINNED)) == len(E.PINNED)
    fam = {E.CASES[c]["family"] for c in E.PINNED}
    assert {"extremes", "phase", "knob", "geometry", "kn", "nes", "floors"} <= fam
    assert {E.images(c).shape[2] for c in E.PINNED} >= {1279, 1280, 256, 8, 7, 4}
    assert {E.images(c).shape[-1] for c in E.PINNED if not E.is_nes(E.CASES[c]["name"])} == {3, 4}
    assert sorted(E.CASES["ntsc-kn-mixed"]["noise"]) == [-32767, 0, 1, 32767]


OVERSHOOT = sorted(c for c in E.CASES if "-overshoot-" in c)


@pytest.mark.parametrize("cid", OVERSHOOT)
def test_overshoot_cases_reach_where_the_24bit_product_would_wrap(cid):
    """white 16383, ire_base 8191: v * white * 64 + (ire_base << 16) reaches 2^31 from v = y + mi + mq >= 1537 on.  analog[] is clamped
    to 110, so v is read off the same images at white 64, ire_base 0, where analog = (v * 64) >> 10 = v >> 4: 97 there means v >= 1552."""
    assert OVERSHOOT and (1537 * 16383 * 64 + (8191 << 16)) >= 1 << 31 > (1536 * 16383 * 64 + (8191 << 16)) and 97 << 4 >= 1537
    case = E.CASES[cid]
    assert E.intended(case, E.KNOB_NOISE) == (16383, 8191, False)
    orc = E.oracle(case["name"])
    imgs = E.images(cid)
    top = 0
    for k in range(case["n"]):
        c = orc.new_crt(E.OUTW, E.OUTH, E.OUTFMT)
        c.set("white_point", E.white_point_for(case["name"], 64))
        c.set("black_point", -orc.sys.black_level)
        c.settings(np.concatenate([imgs[k], imgs[k][-1:]]), w=int(imgs.shape[2]), h=int(imgs.shape[1]), **E.settings_kw(case, k, 0))
        c.modulate()
        top = max(top, int(c.analog.max()))
    assert top >= 97, (cid, top)

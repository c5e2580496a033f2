"""Cases and expected values of the PICTURE knobs -- brightness and contrast per field beside noise, monitor hue and saturation
(crthip_knobs_prepare5; every per-field-knob entry point takes the records); no tests in here.

A case row is (noise, mon_hue, saturation, brightness, contrast).  The values sit on the bounds the code branches on
(crt_setup_decoder_floor, crt_setup.c; T0_BRIGHT_MAX / FAST_BRIGHT_MAX, crt_setup.h), one field each, neighbours on opposite sides,
the defaults (0, 180) in between: the wavefronts that straddle two fields then hold lines of different tier floors.  Expected
pictures and states never come from the library: the oracle runs once per field with that field's five knobs (field-pass), or the
reference's serial loop runs on ONE CRT whose five knobs are turned between the fields (sequence mode).  Geometry, images and
parities are those of tests/knobs_cases.py / tests/seqknobs_cases.py."""
import ctypes as C

import numpy as np

import crtref as R
import knobs_cases as KC
import seqknobs_cases as SK
from test_phosphor_cpu import display_step_np

SMALL = KC.SMALL
BLEND = SK.BLEND

# crt_setup.h / crt_dev.h
T0_BRIGHT_MAX, FAST_BRIGHT_MAX = 2600, 130000
BLACK = {"ntsc": 7, "vhs": 7, "vhslcg": 7, "ntscbloom": 7, "ntscfir7": 7, "snes": 7, "nes": 0}      # BLACK_LEVEL of the system tables


def floor_of(bright, contrast):
    """decoder_min_tier's formula (crt_decode.hip before it moved to crt_setup.c), without the context switches, for coefficients
    inside the 64-bit-mad tiers' ranges (every system of the cases below; tests/test_picknobs_cpu.py asserts it on the blob)"""
    b, ct = abs(bright), abs(contrast)
    if b > FAST_BRIGHT_MAX or ct >= 1 << 23:
        return 3
    if b > T0_BRIGHT_MAX:
        return 2
    vmax = 16380 * (10 * (127 + b) + 64) + 11551 * 3870
    return 2 if ((vmax >> 12) + 1) * ct >= 1 << 31 else 0


def contrast_max(bright):
    """the largest contrast for which ((vmax >> 12) + 1) * |contrast| < 2^31 at this bright"""
    vmax = 16380 * (10 * (127 + abs(bright)) + 64) + 11551 * 3870
    return ((1 << 31) - 1) // ((vmax >> 12) + 1)


def br(bright, black=7):
    """the brightness that gives this luma offset: bright = brightness - (BLACK_LEVEL + black_point)"""
    return bright + black


D = (24, 0, 10)                                        # the other three knobs where they are not the point
DEF = D + (0, 180)
CM0, CMT = contrast_max(-7), contrast_max(T0_BRIGHT_MAX)
assert (CM0, CMT) == (129922, 17862) and floor_of(-7, CM0) == 0 and floor_of(-7, CM0 + 1) == 2 and floor_of(2600, CMT + 1) == 2

# brightness bounds: +-2600 | +-2601 (tier 0 | 24-bit tier), 130 000 | 130 001 (24-bit | exact)
BRIGHT_BOUNDS = [DEF, D + (br(2600), 180), D + (br(2601), 180), DEF, D + (br(-2600), 180), D + (br(-2601), 180),
                 D + (br(130000), 180), D + (br(130001), 180)]
# ... the negative far bound; the contrast bound at the default bright; contrast 0, negative, 2^23 - 1
CONTRAST_BOUNDS = [D + (br(-130000), 180), D + (br(-130001), 180), DEF, D + (0, CM0), D + (0, CM0 + 1), D + (0, 0), D + (0, -180),
                   D + (0, (1 << 23) - 1)]
# ... 2^23; the contrast bound at the far end of tier 0's brightness (both bounds in one field); the negative contrast bound
BOTH_BOUNDS = [D + (0, 1 << 23), DEF, D + (br(2600), CMT), D + (br(2600), CMT + 1), D + (0, -CM0), D + (0, -CM0 - 1)]
# all five differ per field: KC.SMALL_TRIPLES' saturations and hues (tier flags from the carrier amplitude, different inside one
# wavefront) meet the floors of brightness / contrast
ALL_FIVE = [t + pc for t, pc in zip(KC.SMALL_TRIPLES, [(0, 180), (br(2601), 120), (-40, 240), (br(-2600), CM0 + 1), (br(130001), 90), (33, -200)])]
BOUND_CASES = {"bright": BRIGHT_BOUNDS, "contrast": CONTRAST_BOUNDS, "both": BOTH_BOUNDS, "allfive": ALL_FIVE}
# the floors the tables are there for, worked out by hand from the bounds above
FLOORS = {"bright": [0, 0, 2, 0, 0, 2, 2, 3], "contrast": [2, 3, 0, 0, 2, 0, 0, 2], "both": [3, 0, 0, 2, 0, 2],
          "allfive": [0, 2, 0, 2, 3, 0]}

# sequence mode: a brightness ramp through +2600 and a contrast step over the bound, mid-video; SK.SIX's noise / hue / saturation
SEQ_RAMP = [t + pc for t, pc in zip(SK.SIX, [(0, 180), (1300, 180), (br(2600), 180), (br(2601), CM0 + 1), (3900, 1 << 23), (0, 180)])]
SETS_FIRST = SK.SETS_FIRST                             # three ragged sets: 1, 4 and 2 fields
SETS_ROWS = SEQ_RAMP + [(45, -100, 25, br(-2601), 200)]


def per_system(name, n):
    """n rows for the one-case-per-system tests: KC's drawn triples, brightness / contrast walking over the tiers"""
    trip = KC.drawn_triples(n, 600 + n, noise_max=40, sat_lo=-15, sat_hi=30)
    b = BLACK[name]
    pcs = [(0, 180), (br(2601, b), 200), (-25, 150), (40, contrast_max(33) + 1), (br(130001, b), 180), (br(-2600, b), 240)]
    return [t + pcs[k % 6] for k, t in enumerate(trip)]


def oracle_fields5(name, geo, rows, steps=1, crt_knobs=None, seeds=None, fmt=R.FMT_BGRA):
    """KC.oracle_fields with brightness and contrast per field as well (and the output format): field k of a batch as an n = 1 call
    of the reference gives it, `steps` field-passes in a row on its own CRT.  Per field a list of per-step dicts."""
    libc = C.CDLL(None)
    orc = R.Oracle(name)
    nes = orc.system == R.SYS_NES
    dc = orc.system in R.DOT_CRAWL_SYSTEMS
    out = []
    for k, (noise, hue, sat, brightness, contrast) in enumerate(rows):
        c = orc.new_crt(geo["outw"], geo["outh"], fmt)
        c.set("scanlines", 1)
        for a, v in (crt_knobs or {}).items():
            c.set(a, v)
        c.set("hue", hue)
        c.set("saturation", sat)
        c.set("brightness", brightness)
        c.set("contrast", contrast)
        field, frame = KC.parity(k)
        if nes:
            ppu = KC.ppu_image(k)
            c.settings(np.concatenate([ppu, ppu[-1:]], axis=0), w=256, h=240, dot_crawl_offset=KC.dot_crawl(name, k), hue=0)
        else:
            img = KC.image(geo, k)
            c.settings(np.concatenate([img, img[-1:]], axis=0), format=R.FMT_BGRA, w=geo["w"], h=geo["h"], as_color=1)
            if orc.system not in R.PROGRESSIVE_SYSTEMS:
                c.sset("field", field)
                c.sset("frame", frame)
            if dc:
                c.sset("dot_crawl_offset", KC.dot_crawl(name, k))
        if seeds is not None:
            libc.srand(seeds[k])
        per = []
        for step in range(steps):
            c.analog[:] = 0
            if orc.system in R.PROGRESSIVE_SYSTEMS:
                c.sset("field_initialized", 0)
            c.modulate()
            hs_before = c.get("hsync")
            c.demodulate(noise, trace=True)
            per.append(dict(inp=c.inp.copy(), out=c.out.copy(), hsync=c.get("hsync"), vsync=c.get("vsync"), rn=c.get("rn"),
                            ccf=c.ccf.copy(), undefined=R.reads_past_inp(orc, c.trace, c.get("vsync"), hs_before)))
            if not nes and orc.system not in R.PROGRESSIVE_SYSTEMS:
                field ^= 1
                if step % 2 == 0:
                    frame ^= 1
                c.sset("field", field)
                c.sset("frame", frame)
        out.append(per)
    return out


def seq_case(id, rows, geo=SMALL, knobs=None, mode="keep", set_first=None, init="per_set", incoming=None):
    """a case in the format of seqknobs_cases (its helpers read `triples` for noise / hue / saturation), plus `rows`"""
    c = SK._case(id, "ntsc", [r[:3] for r in rows], geo=geo, knobs=knobs, mode=mode, set_first=set_first, init=init, incoming=incoming)
    c["rows"] = [tuple(int(v) for v in r) for r in rows]
    return c


SEQ_CASES = {c["id"]: c for c in [
    seq_case("ramp", SEQ_RAMP),
    seq_case("ramp-blend", SEQ_RAMP, geo=BLEND, knobs=dict(blend=1)),
    seq_case("ramp-fade", SEQ_RAMP, mode="fade"),
    seq_case("sets", SETS_ROWS, set_first=SETS_FIRST, incoming="per_set"),
]}


def serial_loop5(lib, case, lo, hi, init, state_in):
    """SK.serial_loop with all five knobs turned between the fields: the reference's loop on ONE struct CRT over fields [lo, hi)"""
    par, dco = SK.parities(case), SK.dot_crawl(case)
    c = SK._new_crt(lib, case)
    c.out[:] = init.reshape(-1)
    c.set("hsync", state_in[0])
    c.set("vsync", state_in[1])
    c.set("rn", state_in[2])
    want = []
    for k in range(lo, hi):
        noise, hue, sat, brightness, contrast = case["rows"][k]
        if case["mode"] != "keep":
            c.out[:] = display_step_np(c.out, R.FMT_BGRA, case["mode"])
        c.set("hue", hue)
        c.set("saturation", sat)
        c.set("brightness", brightness)
        c.set("contrast", contrast)
        SK._settings(c, case, k, par[k], dco[k])
        c.modulate()
        hs_before = c.get("hsync")
        undefined = None
        if isinstance(lib, R.Oracle):
            c.demodulate(noise, trace=True)
            undefined = R.reads_past_inp(lib, c.trace, c.get("vsync"), hs_before)
        else:
            c.demodulate(noise)
        want.append(dict(out=c.out.copy(), hsync=c.get("hsync"), vsync=c.get("vsync"), rn=c.get("rn"), ccf=c.ccf.copy(),
                         undefined=undefined))
    return want


_EXPECTED = {}


def seq_expected(case, lib=None):
    """per-set serial loops of the oracle (or `lib`) -> one dict per field, in batch order; the oracle's is computed once per case"""
    if lib is None and case["id"] in _EXPECTED:
        return _EXPECTED[case["id"]]
    use = lib or R.Oracle(case["name"])
    init, inc = SK.init_pictures(case), SK.incoming(case)
    want = []
    for s, (lo, hi) in enumerate(SK.sets_of(case)):
        want += serial_loop5(use, case, lo, hi, SK._init_of_set(case, init, s), inc[s])
    if lib is None:
        _EXPECTED[case["id"]] = want
    return want


_FIELDS = {}


def expected(key, fn):
    """an expected result is computed once and shared by the tests that need it: treat it as read-only"""
    if key not in _FIELDS:
        _FIELDS[key] = fn()
    return _FIELDS[key]

"""Cases and expected values of the HUE knob -- the ENCODER hue per field beside the other seven (crthip_knobs_prepare8 +
crthip_bind_hues; every per-field-knob entry point reads the binding); no tests in here.

A case row is (noise, mon_hue, saturation, brightness, contrast, black_point, white_point, hue).  The hue is NTSC_SETTINGS.hue (keys
5 / 6 of the interactive driver): it rotates burst, modI and modQ (crt_ntsc.c:174-183 and its siblings) and so reaches the active
video, the burst samples of every video line and the ccf preset.  Expected pictures, signals and states never come from the
library: the oracle runs once per field with that field's eight knobs (field-pass), or the reference's serial loop runs on ONE struct
CRT / NTSC_SETTINGS whose knobs -- hue included -- are turned between the fields (sequence mode): the construction of
tests/levels_cases.py.  Geometry and parities are those of tests/knobs_cases.py: 64x48 -> 160x120, 3 to 6 fields."""
import ctypes as C

import numpy as np

import crtref as R
import encoder_cases as EC
import knobs_cases as KC
import levels_cases as LV
import picknobs_cases as PK
import seqknobs_cases as SK
from test_phosphor_cpu import display_step_np

SMALL = KC.SMALL
BLEND = SK.BLEND
D7 = (24, 0, 10, 0, 180, 0, 100)                        # the other seven where they are not the point

# the values the issue names: 0, +-1, the burst offset itself, the quadrants, the last angle before a turn; a whole turn of either
# sign (the reference's integer division decides whether it equals 0: the oracle is asked, nothing is assumed), more than a turn,
# negative angles (C truncates towards zero)
HUES_A = [0, 1, -1, 33, 90, 180]
HUES_B = [359, 360, -360, 405, -90, -123]
# at least three pairwise distinct hues: with desth no multiple of 64 a wavefront holds rows of two fields
STRADDLE = [0, 77, -45, 200, -300]
BATCHES = {
    "a": [D7 + (h,) for h in HUES_A],
    "b": [D7 + (h,) for h in HUES_B],
    "straddle": [D7 + (h,) for h in STRADDLE],
    # the hue together with the other seven: LV.COMBINED (a clean field in a noisy batch, a contrast above the 24-bit tier, levels
    # of both signs)
    "combined": [r + (h,) for r, h in zip(LV.COMBINED, [405, -90, 33, -123, 180, 359])],
}
# dot crawl offsets 0..5 beside negative hues (the line-class systems: the unreduced carrier row matters)
DCO6 = [0, 1, 2, 3, 4, 5]
DCO_HUES = [-123, 0, -90, 405, -1, -360]


def dot_crawl(name, k):
    return DCO6[k % 6]


def per_system(name, n):
    """n rows for the one-case-per-system tests: KC's drawn triples, LV's level pairs, hues of DCO_HUES"""
    rows = LV.per_system(name, n)
    return [tuple(r) + (DCO_HUES[k % 6],) for k, r in enumerate(rows)]


def default_images(geo, n):
    return [KC.image(geo, k) for k in range(n)]


def oracle_fields8(name, geo, rows, steps=1, crt_knobs=None, seeds=None, fmt=R.FMT_BGRA, images=None, ifmt=R.FMT_BGRA, as_color=1,
                   dco=None, noise_stage=True):
    """LV.oracle_fields7 with the encoder hue per field as well: field k of a batch as an n = 1 call of the reference gives it,
    `steps` field-passes in a row on its own CRT.  Per field a list of per-step dicts (`analog`: the clean signal of the step)."""
    libc = C.CDLL(None)
    orc = R.Oracle(name)
    dc = orc.system in R.DOT_CRAWL_SYSTEMS
    out = []
    for k, (noise, mon_hue, sat, brightness, contrast, black_point, white_point, hue) in enumerate(rows):
        c = orc.new_crt(geo["outw"], geo["outh"], fmt)
        c.set("scanlines", 1)
        for a, v in (crt_knobs or {}).items():
            c.set(a, v)
        for a, v in (("hue", mon_hue), ("saturation", sat), ("brightness", brightness), ("contrast", contrast),
                     ("black_point", black_point), ("white_point", white_point)):
            c.set(a, v)
        field, frame = KC.parity(k)
        img = images[k] if images is not None else KC.image(geo, k)
        c.settings(np.concatenate([img, img[-1:]], axis=0), format=ifmt, w=geo["w"], h=geo["h"], as_color=as_color)
        c.sset("hue", hue)
        if orc.system not in R.PROGRESSIVE_SYSTEMS:
            c.sset("field", field)
            c.sset("frame", frame)
        if dc:
            c.sset("dot_crawl_offset", dot_crawl(name, k) if dco is None else dco[k])
        if seeds is not None:
            libc.srand(seeds[k])
        per = []
        for step in range(steps):
            c.analog[:] = 0
            if orc.system in R.PROGRESSIVE_SYSTEMS:
                c.sset("field_initialized", 0)
            c.modulate()
            analog = np.array(c.analog).copy()
            hs_before = c.get("hsync")
            c.demodulate(noise, trace=True)
            per.append(dict(analog=analog, inp=c.inp.copy(), out=c.out.copy(), hsync=c.get("hsync"), vsync=c.get("vsync"),
                            rn=c.get("rn"), ccf=c.ccf.copy(), undefined=R.reads_past_inp(orc, c.trace, c.get("vsync"), hs_before)))
            if orc.system not in R.PROGRESSIVE_SYSTEMS:
                field ^= 1
                if step % 2 == 0:
                    frame ^= 1
                c.sset("field", field)
                c.sset("frame", frame)
        out.append(per)
    return out


# sequence mode: a recorded session in which the user turns the encoder hue (and the other seven) mid-video
SEQ_HUES = [0, 33, 33, -90, 405, -123]
SEQ_ROWS = [r + (h,) for r, h in zip(LV.SEQ_ROWS, SEQ_HUES)]
SETS_FIRST = SK.SETS_FIRST                             # three ragged sets: 1, 4 and 2 fields
SETS_ROWS = SEQ_ROWS + [LV.SETS_ROWS[-1] + (359,)]

SEQ_CASES = {c["id"]: c for c in [
    PK.seq_case("hues", SEQ_ROWS),
    PK.seq_case("hues-blend", SEQ_ROWS, geo=BLEND, knobs=dict(blend=1)),
    PK.seq_case("hues-fade", SEQ_ROWS, mode="fade"),
    PK.seq_case("hues-sets", SETS_ROWS, set_first=SETS_FIRST, incoming="per_set"),
    PK.seq_case("hues-sets-blend", SETS_ROWS, geo=BLEND, knobs=dict(blend=1), set_first=SETS_FIRST, incoming="per_set"),
]}


def serial_loop8(lib, case, lo, hi, init, state_in):
    """LV.serial_loop7 with all eight knobs turned between the fields: the reference's loop on ONE struct CRT over fields [lo, hi)"""
    par, dco = SK.parities(case), SK.dot_crawl(case)
    c = SK._new_crt(lib, case)
    c.out[:] = init.reshape(-1)
    c.set("hsync", state_in[0])
    c.set("vsync", state_in[1])
    c.set("rn", state_in[2])
    want = []
    for k in range(lo, hi):
        noise, mon_hue, sat, brightness, contrast, black_point, white_point, hue = case["rows"][k]
        if case["mode"] != "keep":
            c.out[:] = display_step_np(c.out, R.FMT_BGRA, case["mode"])
        for a, v in (("hue", mon_hue), ("saturation", sat), ("brightness", brightness), ("contrast", contrast),
                     ("black_point", black_point), ("white_point", white_point)):
            c.set(a, v)
        SK._settings(c, case, k, par[k], dco[k])
        c.sset("hue", hue)
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
        want += serial_loop8(use, case, lo, hi, SK._init_of_set(case, init, s), inc[s])
    if lib is None:
        _EXPECTED[case["id"]] = want
    return want


_FIELDS = {}


def expected(key, fn):
    """an expected result is computed once and shared by the tests that need it: treat it as read-only"""
    if key not in _FIELDS:
        _FIELDS[key] = fn()
    return _FIELDS[key]


def burst_positions(name, yo):
    """the model of the margin patch: the set of (line, t) an HU margin kernel rewrites = where skeleton() writes burst -- columns
    cb_beg .. cb_beg + cb_len of the active lines (NES timing) or of every line without equalising pulses or vertical sync"""
    sd = EC.oracle(name).sys
    out = set()
    for n in range(sd.vres):
        if name.startswith("nesrgb"):
            on = yo <= n < yo + sd.lines
        else:
            on = not (sd.equ_a_lo <= n <= sd.equ_a_hi or sd.equ_b_lo <= n <= sd.equ_b_hi or sd.vs_lo <= n <= sd.vs_hi)
        if on:
            out.update((n, t) for t in range(sd.cb_beg, sd.cb_beg + sd.cb_len))
    return out

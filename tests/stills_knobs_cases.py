"""Cases and expected values of stills with one look per still (crthip_stills_knobs / CRT.stills_knobs, include/crt_hip.h); no tests
in here.

A case is a batch of n images that all take the same schedule of field-passes onto their own picture (tests/stills_cases.py), still k
with row k of the case as its look in EVERY pass: (noise, mon_hue, saturation[, brightness, contrast[, black_point, white_point[,
hue]]]) -- the row widths CRT.upload_knobs takes.  Expected pictures and states never come from the library: per still the oracle (or
the compiled reference) runs the reference's loop on ONE struct CRT that carries the still's values -- per schedule entry: display step
(phosphor cases), clean analog[], crt_modulate with the still's NTSC_SETTINGS.hue, crt_demodulate(noise_k).  Geometry: the SMALL one of
tests/knobs_cases.py, 64x48 -> 160x120 (row collisions: outh < 240; desth is no multiple of 64, so with the lane-per-scanline shape a
wavefront's rows belong to two stills), 5 or 6 stills; one case has a single still, one 160x480 pictures without scanlines (duplicated
rows), and the aberration band keeps the 160x240 of tests/stills_cases.py (its v_fac = 8 keeps every read of the reference defined)."""
import numpy as np

import crtref as R
import hues_cases as HU
import knobs_cases as KC
import levels_cases as LV
import picknobs_cases as PK
import stills_cases as SC
from test_phosphor_cpu import display_step_np

SMALL = KC.SMALL
CLI_BLEND = SC.CLI_BLEND
NOBLEND = dict(scanlines=1, blend=0)
INTERLACED0, INTERLACED1, PROGRESSIVE, CUSTOM5 = SC.INTERLACED0, SC.INTERLACED1, SC.PROGRESSIVE, SC.CUSTOM5
SNES_DOTS = [(r & 1, (r >> 1) & 1, r % 3) for r in range(5)]          # dot_crawl_offset 0, 1, 2, 0, 1 beside both parities: 5 distinct entries
SNES_DOTS_SHARED = SNES_DOTS + SNES_DOTS[:3]                        # ... three of them used twice
CRT_KNOBS = ("hue", "saturation", "brightness", "contrast", "black_point", "white_point")      # row[1:7], struct CRT's names

# (shape, padded signal lines, set_exact): both kernel shapes everywhere; both layouts and the exact encoder on the cases that list them
BOTH = ((1, 1, 0), (2, 1, 0))
ALL_CONFIGS = ((1, 1, 0), (1, 0, 0), (2, 1, 0), (2, 0, 0), (1, 1, 1), (2, 1, 1), (2, 0, 1))


def with_noise(rows, noise):
    """the rows with their noise column replaced (one int for all, or one per still)"""
    ns = [noise] * len(rows) if isinstance(noise, int) else list(noise)
    assert len(ns) == len(rows)
    return [(int(z),) + tuple(r[1:]) for z, r in zip(ns, rows)]


# saturation on both sides of tier 0's chroma bound and in the exact tier (KC.SMALL_TRIPLES: 900 / 40 / 13 / -70)
SAT_ROWS = KC.SMALL_TRIPLES
# one still at the first contrast that takes the 24-bit tier at brightness 0 (PK.CM0 + 1 = 129 923), its neighbours in tier 0
PIC_ROWS = [t + pc for t, pc in zip(KC.SMALL_TRIPLES[:5], [(0, 180), (5, 200), (0, PK.CM0 + 1), (-40, 240), (33, 90)])]
# the eight values at once (HU.BATCHES["combined"]: hues 405, -90, 33, -123, 180, 359; a contrast above the 24-bit tier)
COMBINED = HU.BATCHES["combined"]
# the hues the issue names
NAMED_HUES = [HU.D7 + (h,) for h in (0, -123, 405, 359, 77)]


def bound_rows(which):
    """(white, ire_base) exactly on either side of the encoder's fast-path bound: `inside` = six stills with +-8191, the others five
    stills with ONE on +-8192 (LV.bound_batches); every still with a hue of its own"""
    rows = list(LV.bound_batches("ntsc")[which])
    if which != "inside":
        rows.append(LV.at("ntsc", noise=30, sat=12))
    return [tuple(r) + (h,) for r, h in zip(rows, (0, -123, 405, 359, 33, -45))]


def _case(id, name, rows, sched, knobs=CLI_BLEND, mode="keep", out=(SMALL["outw"], SMALL["outh"]), configs=BOTH, seeds=None):
    nes = R.SYSTEMS[name][0] == R.SYS_NES
    rows = [tuple(int(v) for v in r) for r in rows]
    assert len({len(r) for r in rows}) == 1 and len(rows[0]) in (3, 5, 7, 8)
    return dict(id=id, name=name, inp=(256, 240) if nes else (SMALL["w"], SMALL["h"]), outw=out[0], outh=out[1], ofmt=R.FMT_BGRA,
                knobs=knobs, n=len(rows), rows=rows, sched=sched, mode=mode, configs=configs, seeds=seeds)


CASES = [
    # every still at noise 0: the clean signal of every distinct entry encoded once, with the records' blob
    _case("ntsc-cli-sat-noise0", "ntsc", with_noise(SAT_ROWS, 0), INTERLACED0),
    _case("ntsc-custom5-hues-noise0", "ntsc", with_noise(NAMED_HUES, 0), CUSTOM5, knobs=NOBLEND, configs=ALL_CONFIGS),
    _case("ntsc-bound-inside-noise0", "ntsc", with_noise(bound_rows("inside"), 0), PROGRESSIVE),
    _case("ntsc-bound-white+-noise0", "ntsc", with_noise(bound_rows("white+"), 0), PROGRESSIVE),
    _case("ntsc-bound-ire--noise0", "ntsc", with_noise(bound_rows("ire-"), 0), PROGRESSIVE),
    _case("ntsc-one-still-noise0", "ntsc", with_noise(COMBINED[3:4], 0), INTERLACED0),
    _case("ntsc-fade-noise0", "ntsc", with_noise(SAT_ROWS[:5], 0), INTERLACED0, mode="fade"),
    _case("ntsc-duprows-pic-noise0", "ntsc", with_noise(PIC_ROWS, 0), PROGRESSIVE, knobs=dict(scanlines=0, blend=1), out=(160, 480)),
    _case("ntscfir7-levels-noise0", "ntscfir7", with_noise(LV.STRADDLE, 0), INTERLACED1),
    _case("snes-dots-noise0", "snes", with_noise(HU.per_system("snes", 6), 0), SNES_DOTS_SHARED),
    _case("vhslcg-band-noise0", "vhslcg", with_noise(HU.per_system("vhslcg", 5), 0), SC.VHS_BAND, knobs=SC.VHS_BAND_KNOBS, out=(160, 240)),
    # one noisy still in the batch: every pass encodes
    _case("ntsc-cli1-combined-one-noisy", "ntsc", with_noise(COMBINED, [0, 24, 0, 0, 0, 0]), INTERLACED1, configs=((1, 1, 0), (2, 0, 0))),
    _case("nes-dots-pic-one-noisy", "nes", with_noise(PIC_ROWS, [0, 24, 0, 0, 0]), SC.NES_DOTS),
    _case("vhslcg-band-one-noisy", "vhslcg", with_noise(HU.per_system("vhslcg", 5), [0, 24, 0, 0, 0]), SC.VHS_BAND, knobs=SC.VHS_BAND_KNOBS,
          out=(160, 240)),
    # every still above 0, and mixes with clean stills inside a noisy batch
    _case("ntsc-prog-pic-all-noisy", "ntsc", with_noise(PIC_ROWS, [24, 7, 110, 30, 60]), PROGRESSIVE, knobs=NOBLEND),
    _case("ntsc-bound-white--noisy", "ntsc", bound_rows("white-"), PROGRESSIVE),
    _case("ntsc-bound-ire+-noisy", "ntsc", bound_rows("ire+"), PROGRESSIVE),
    _case("ntscbloom-max-e-per-still", "ntscbloom", [(24, 0, 10), (0, 17, 14), (30, -20, 12), (24, 350, 40), (60, 77, 13)], INTERLACED0),
    _case("temp-dots-noisy", "temp", HU.per_system("temp", 6), SNES_DOTS),
    _case("vhs-rand-levels", "vhs", LV.per_system("vhs", 5), INTERLACED0, seeds=SC.VHS_SEEDS),
]
CASE_IDS = [c["id"] for c in CASES]


def case(id):
    return CASES[CASE_IDS.index(id)]


def width(case):
    return len(case["rows"][0])


def noise_max(case):
    return max(r[0] for r in case["rows"])


def images(case):
    """the n different images of the case: [n, h, w, 4] BGRA (KC.image), or [n, 240, 256] PPU pixels for the NES (KC.ppu_image)"""
    if SC.sysid(case) == R.SYS_NES:
        return np.stack([KC.ppu_image(k) for k in range(case["n"])])
    return np.stack([KC.image(SMALL, k) for k in range(case["n"])])


def still_loop(lib, case, img, row, k, check_reads=False):
    """the reference's loop on ONE struct CRT with still k's look: (out, hsync, vsync, rn, ccf) after the last pass"""
    c = lib.new_crt(case["outw"], case["outh"], case["ofmt"])
    for a, v in case["knobs"].items():
        c.set(a, v)
    for a, v in zip(CRT_KNOBS, row[1:7]):
        c.set(a, v)
    if SC.is_vhs_rand(case):
        lib.srand(case["seeds"][k])
    for r, entry in enumerate(case["sched"]):
        if case["mode"] != "keep":
            c.out[:] = display_step_np(c.out, case["ofmt"], case["mode"])
        SC._pass_settings(case, c, lib, img, entry)
        if len(row) == 8:
            c.sset("hue", row[7])
        c.analog[:] = 0                                    # every field-pass starts from a crt_init-clean analog[] (crt_hip.h)
        if lib.system in R.PROGRESSIVE_SYSTEMS:
            c.sset("field_initialized", 0)                 # ... which the NES encoders then fill again (KC.oracle_fields)
        c.modulate()
        hs_before = c.get("hsync")
        if check_reads:
            c.demodulate(row[0], trace=True)
            assert not R.reads_past_inp(lib, c.trace, c.get("vsync"), hs_before), \
                "%s still %d pass %d: the reference reads past inp[] here (undefined): pick another configuration" % (case["id"], k, r)
        else:
            c.demodulate(row[0])
    return c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn"), np.array(c.ccf, dtype=np.int32).copy()


_EXPECTED = {}


def expected(case, lib=None, check_reads=False, one_image=None, rows=None):
    """[(out, hsync, vsync, rn, ccf)] per still.  The oracle's values are computed once per case and shared (leave them unchanged).
    one_image: every still reads image `one_image` of the case (the image_stride == 0 tests); rows: other looks than the case's."""
    key = (case["id"], one_image, None if rows is None else tuple(map(tuple, rows)))
    if lib is None and not check_reads:
        if key not in _EXPECTED:
            _EXPECTED[key] = expected(case, R.Oracle(case["name"]), False, one_image, rows)
        return _EXPECTED[key]
    lib = lib or R.Oracle(case["name"])
    imgs = images(case)
    use = case["rows"] if rows is None else rows
    return [still_loop(lib, case, imgs[k if one_image is None else one_image], use[k], k, check_reads) for k in range(len(use))]

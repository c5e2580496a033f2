"""The inputs of tests/test_gpu_parity.py (TEST INFRASTRUCTURE ONLY; numpy and the CPU checkers, no GPU, no tests).

test_gpu_parity.py compares the HIP path with the oracle (oracle/crt_oracle.c), our own restatement of the reference.  What pins that
restatement to the REAL reference (oracle/_ref) on these very inputs is tests/test_parity_pin_cpu.py; both files take from here

* the case tables (CASES, WIDE_CASES, F4_CASES, NES_CASES), the random generators with their seeds, and the cases that used to stand
  inline in single tests, by name;
* the input recipe of test_gpu_parity._run_case: image k is crtref.synth_image seed 777 + 13 k ("random" for even k, "bars" for odd k),
  field k starts at parity k & 1 and frame (k >> 1) & 1, the parity toggles every pass and the frame after every even one
  (video_convert.c:259-267), the dot crawl offsets are (k + 1) % 3 (PV-1000, template: (2 k + 1) % 6);
* the recipes of the tests that build their inputs differently: the NES table, the rand()-noise VHS builds, the many-seeds test and
  the wild sync states;
* TABLES: every (table, system-name variant, case) a GPU test runs, with the (n, steps) the pin runs it at -- the largest of the GPU
  tests that use the table; field k's inputs do not depend on n, and fewer passes are a prefix of more;
* EXCLUDED: how many field-passes crtref.reads_past_inp takes out of the comparison, per case.  A field stays out from its first such
  pass on, and every later pass counts.  These are stated conditions: the pin asserts each count exactly, and that no case loses more
  than half of its field-passes (the wild sync states keep their own rule: two of three passes over the fields looked at).  A table
  without an entry excludes nothing, and the GPU tests then assert that no field dropped out at all.

A checker is crtref.Oracle or crtref.RefLib; both are driven through the same functions, so "exactly the inputs of the GPU test" is
one piece of code."""
import ctypes as C

import numpy as np

import crtref as R

_LIBC = C.CDLL(None)

CASES = [
    # name, outw, outh, ofmt, w, h, ifmt, noise, settings, knobs
    ("ntsc", 640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 0, dict(as_color=1), {}),
    ("ntsc", 640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 24, dict(as_color=1), dict(scanlines=1)),
    ("ntsc", 832, 624, R.FMT_ARGB, 640, 480, R.FMT_ABGR, 40, dict(as_color=1, hue=350), dict(hue=17, saturation=14)),
    ("ntsc", 640, 480, R.FMT_RGB, 320, 200, R.FMT_RGB, 12, dict(as_color=1, hue=30), dict(blend=1)),
    ("ntsc", 1920, 1080, R.FMT_RGBA, 1920, 1080, R.FMT_BGR, 0, dict(as_color=1), dict(scanlines=1)),
    ("ntsc", 1920, 1080, R.FMT_BGRA, 1920, 1080, R.FMT_BGRA, 0, dict(as_color=1), dict(scanlines=0, blend=1)),
    ("ntsc", 753, 240, R.FMT_ABGR, 753, 236, R.FMT_RGBA, 5, dict(as_color=0), dict(brightness=9, contrast=200)),
    ("ntsc", 500, 300, R.FMT_BGR, 200, 100, R.FMT_ARGB, 60, dict(as_color=1, raw=1), dict(black_point=3, white_point=90)),
    ("ntsc", 333, 481, R.FMT_RGB, 100, 300, R.FMT_RGB, 100, dict(as_color=1, raw=1, xoffset=8, yoffset=2), dict(v_fac=10)),
    ("ntsc", 257, 243, R.FMT_BGRA, 800, 600, R.FMT_BGRA, 24, dict(as_color=1, hue=180), dict(scanlines=1, blend=1)),
    # between the envelopes: saturation 40 puts the carrier above tier 0's bound (lines flagged NOT64, tier 1),
    # brightness 5000 lifts the whole batch to tier 1
    ("ntsc", 640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 24, dict(as_color=1), dict(saturation=40)),
    ("ntsc", 640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 24, dict(as_color=1), dict(brightness=5000, contrast=20)),
    ("ntsc", 640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 60, dict(as_color=1), dict(brightness=-2600, saturation=24)),
    # either side of tier 0's chroma bound (|wave| <= 65532: I/Q low cascades dropped), with heavy noise
    ("ntsc", 640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 110, dict(as_color=1, hue=77), dict(saturation=13)),
    ("ntsc", 640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 110, dict(as_color=1, hue=77), dict(saturation=14)),
    # outside the 24-bit multiply envelope: huge saturation (lines flagged CRTHIP_LINE_EXACT by k_sync) ...
    ("ntsc", 640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 30, dict(as_color=1), dict(saturation=900, contrast=300)),
    # ... and huge brightness / contrast / white point (host-side check picks the exact kernels)
    ("ntsc", 640, 480, R.FMT_RGBA, 640, 480, R.FMT_RGBA, 10, dict(as_color=1), dict(brightness=200000, contrast=9000000, white_point=9000000)),
    ("ntsc", 320, 240, R.FMT_BGRA, 320, 240, R.FMT_BGRA, 50000000, dict(as_color=1), dict(saturation=-70)),
    # standard NTSC built with CRT_CHROMA_PATTERN 0 (HRES 912, vertical chroma, no phase flip)
    ("ntscp0", 640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 24, dict(as_color=1, hue=40), dict(scanlines=1)),
    ("ntscp0", 832, 624, R.FMT_RGB, 320, 240, R.FMT_BGR, 0, dict(as_color=1, raw=1), dict(blend=1)),
    # outh < CRT_LINES: several CRT lines land on one output row; sequential semantics incl. blend chains
    ("ntsc", 640, 200, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 24, dict(as_color=1), dict(blend=1)),
    ("ntsc", 101, 77, R.FMT_RGB, 64, 48, R.FMT_RGB, 10, dict(as_color=1), dict(scanlines=1)),
    ("ntsc", 64, 120, R.FMT_ABGR, 64, 48, R.FMT_BGRA, 0, dict(as_color=1), dict(blend=1, v_fac=30)),
]

WIDE_CASES = [
    # name, outw, outh, ofmt, w, h, ifmt, noise, settings, knobs -- pictures the 16-scanlines-per-wave decoder takes (crt_decode4.hip)
    ("ntsc", 1920, 1080, R.FMT_BGRA, 1920, 1080, R.FMT_BGRA, 0, dict(as_color=1), dict(scanlines=1)),
    ("ntsc", 1920, 1080, R.FMT_ARGB, 640, 480, R.FMT_RGB, 24, dict(as_color=1, hue=40), dict(scanlines=0, hue=-20, saturation=14)),
    ("ntsc", 2047, 777, R.FMT_ABGR, 333, 100, R.FMT_ABGR, 60, dict(as_color=0), dict(scanlines=1, v_fac=100, brightness=12, contrast=250)),
    ("ntsc", 1700, 300, R.FMT_RGBA, 1281, 601, R.FMT_BGRA, 12, dict(as_color=1, raw=1), dict(scanlines=1, black_point=-5, white_point=120)),
    ("snes", 1920, 1080, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 24, dict(as_color=1), dict(scanlines=1)),
    ("temp", 1664, 1248, R.FMT_BGRA, 832, 624, R.FMT_BGRA, 0, dict(as_color=1), dict(scanlines=1)),
    ("ntscp0", 1920, 1200, R.FMT_BGRA, 1920, 1080, R.FMT_RGBA, 24, dict(as_color=1), dict(scanlines=1)),
    # strong carriers: some 64-scanline groups leave tiers 0 / 1 and stay with the lane-per-scanline kernel, their neighbours do not
    ("ntsc", 1920, 1080, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 24, dict(as_color=1), dict(scanlines=1, saturation=25)),
    ("ntsc", 1920, 1080, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 40, dict(as_color=1), dict(scanlines=1, saturation=60, contrast=300)),
]

# SNES, template, PV-1000 (5 samples per chroma cycle), NES-RGB;  8(f3): CRT_DO_BLOOM builds
F4_CASES = [
    # outw, outh, ofmt, w, h, ifmt, noise, settings, knobs
    (640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 0, dict(as_color=1), {}),
    (640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 24, dict(as_color=1, hue=25), dict(scanlines=1)),
    (832, 624, R.FMT_ARGB, 640, 480, R.FMT_ABGR, 40, dict(as_color=1, hue=350), dict(hue=17, saturation=14)),
    (640, 480, R.FMT_RGB, 320, 200, R.FMT_RGB, 12, dict(as_color=1, hue=-57), dict(blend=1)),
    (500, 300, R.FMT_BGR, 200, 100, R.FMT_ARGB, 60, dict(as_color=1, raw=1, xoffset=8, yoffset=2), dict(black_point=3, white_point=90)),
    (753, 240, R.FMT_ABGR, 753, 236, R.FMT_RGBA, 5, dict(as_color=0), dict(brightness=9, contrast=200)),
    (640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA, 30, dict(as_color=1), dict(saturation=900, contrast=300)),
]

NES_CASES = [
    # name, outw, outh, noise, knobs
    ("nes", 640, 480, 0, {}),
    ("nes", 640, 480, 24, dict(scanlines=1)),
    ("nesp0", 640, 480, 12, dict(blend=1, hue=15)),       # BASELINE configs[4]: CRT_CHROMA_PATTERN 0
    ("nesp0", 256, 240, 0, dict(saturation=12)),
    ("nes", 768, 720, 40, dict(scanlines=1, black_point=2, white_point=95)),
    # round 3: either side of the decoder envelopes that follow from the NES's own signal range (carrier amplitude grows
    # with the saturation: tier 0 -> tier 1 without / with the I/Q low cascades -> 24-bit tier)
    ("nesp0", 640, 480, 12, dict(saturation=8)),
    ("nesp0", 640, 480, 60, dict(saturation=13, scanlines=1)),
    ("nesp0", 640, 480, 100, dict(saturation=16)),
    ("nes", 640, 480, 30, dict(saturation=19, white_point=120)),
    ("nes", 640, 480, 12, dict(saturation=26, contrast=40000)),
    # NES_BORDER 1 (crt_nes.c:69,138-160): the border colour right of the picture
    ("nesborder", 640, 480, 12, dict(scanlines=1)),
    ("nesborder", 512, 480, 0, dict(black_point=4, white_point=90)),
    # wide pictures: the wide-run decoder (crt_decode4.hip), which the NES enters in tier 1 (its carriers do not fit 24 bits)
    ("nesp0", 1920, 1080, 12, dict(scanlines=1)),
    ("nes", 1700, 600, 24, dict(saturation=16)),
]


def random_case(rng):
    w = int(rng.choice([1, 2, 3, 5, 17, 64, 100, 333, 640, 753, 800, 1281]))
    h = int(rng.choice([1, 2, 7, 48, 100, 236, 237, 480, 601]))
    outw = int(rng.choice([1, 3, 4, 5, 31, 32, 33, 250, 640, 1283]))
    outh = int(rng.choice([1, 17, 120, 239, 240, 241, 480, 500, 777]))
    ifmt, ofmt = int(rng.integers(0, 6)), int(rng.integers(0, 6))
    raw = int(rng.integers(0, 2))
    skw = dict(as_color=int(rng.integers(0, 2)), raw=raw, hue=int(rng.integers(-400, 800)))
    if raw and w <= 640 and h <= 200:
        # offsets only where the active rectangle still fits the raster: beyond that crt_modulate scribbles
        # over neighbouring lines (crt_ntsc.c:322) -- outside the contract, the library refuses it
        skw.update(xoffset=int(rng.integers(0, 3)) * 4, yoffset=int(rng.integers(0, 3)))
    knobs = dict(hue=int(rng.integers(-360, 720)), brightness=int(rng.integers(-40, 40)), contrast=int(rng.integers(0, 400)),
                 saturation=int(rng.integers(-5, 40)), black_point=int(rng.integers(-10, 10)),
                 white_point=int(rng.integers(50, 150)), scanlines=int(rng.integers(0, 2)), blend=int(rng.integers(0, 2)),
                 v_fac=int(rng.choice([0, 0, 0, 7, 100])))
    noise = int(rng.choice([0, 1, 24, 77, 300]))
    return ("ntsc", outw, outh, ofmt, w, h, ifmt, noise, skw, knobs)


def random_wide_case(rng):
    """random_case with picture widths the wide-run decoder takes (crt_decode4.hip: outw from ~1650 up, 4-byte pixels, no blend);
    three-byte formats, blend and the narrower widths in the list fall back to the lane-per-scanline kernel -- also a case"""
    case = list(random_case(rng))
    case[0] = str(rng.choice(["ntsc", "ntscp0", "snes", "temp", "nesrgb"]))
    case[1] = int(rng.choice([1500, 1650, 1664, 1700, 1919, 1920, 1921, 2047, 2560, 3001, 3840, 4095]))
    case[2] = int(rng.choice([1, 120, 240, 241, 480, 777, 1080, 1200, 2160]))
    case[3] = int(rng.choice([R.FMT_RGBA, R.FMT_BGRA, R.FMT_ARGB, R.FMT_ABGR, R.FMT_RGBA, R.FMT_BGRA, R.FMT_RGB]))
    case[9] = dict(case[9], blend=int(rng.integers(0, 8) == 0))
    return tuple(case)


RANDOM_SEED0, RANDOM_SEEDS = 1000, 48                     # test_random_configurations (both shapes): n = 2, 2 passes
RANDOM_WIDE_SEED0, RANDOM_WIDE_SEEDS = 7000, 16           # test_random_wide_configurations: n = 2, 2 passes
RANDOM_BLOOM_SEED0, RANDOM_BLOOM_SEEDS = 5000, 24         # test_random_configurations_bloom_lane_per_scanline: n = 3, 2 passes
BLOOM_NAMES = ("ntscbloom", "snesbloom", "pv1kbloom")


def random_seed_case(seed):
    return random_case(np.random.default_rng(RANDOM_SEED0 + seed))


def random_wide_seed_case(seed):
    return random_wide_case(np.random.default_rng(RANDOM_WIDE_SEED0 + seed))


def random_bloom_seed_case(seed):
    return (BLOOM_NAMES[seed % 3],) + tuple(random_case(np.random.default_rng(RANDOM_BLOOM_SEED0 + seed))[1:])


def renamed(name, case):
    """a row of CASES under another build's name"""
    return (name,) + tuple(case[1:])


# ---------------------------------------------------------------------------------------------------------------------------
# the cases that single tests used to hold inline
# ---------------------------------------------------------------------------------------------------------------------------
_STD = (640, 480, R.FMT_BGRA, 640, 480, R.FMT_BGRA)

FIR_TAPS, FIR_CASES = (7, 6, 5, 4), (1, 2, 4, 8)                                  # test_fir_decoder_parity: rows of CASES
FIR_ENVELOPE_KNOBS = [dict(saturation=900, contrast=300), dict(brightness=200000, contrast=9000000, white_point=9000000)]


def fir_envelope_case(knobs):
    """test_fir_decoder_outside_the_24bit_envelope"""
    return ("ntscfir7",) + _STD + (30, dict(as_color=1), knobs)


PV1K_TIER_KNOBS = [dict(saturation=3), dict(saturation=7, contrast=250), dict(saturation=12, brightness=40), dict(saturation=18),
                   dict(saturation=30, contrast=20000), dict(saturation=-9), dict(saturation=200)]


def pv1k_tier_case(knobs):
    """test_pv1k_decoder_tiers"""
    return ("pv1k",) + _STD + (24, dict(as_color=1, hue=11), dict(knobs, scanlines=1))


ENVELOPE_SATURATIONS = [11, 15, 17, 19, 22]


def between_the_envelopes_case(sat):
    """test_ntsc_between_the_envelopes"""
    return ("ntsc",) + _STD + (24, dict(as_color=1), dict(saturation=sat, scanlines=1))


BLOOM_TIER_KNOBS = [dict(saturation=14), dict(saturation=19), dict(saturation=40), dict(brightness=5000, contrast=20),
                    dict(saturation=900, contrast=300), dict(brightness=200000, contrast=9000000, white_point=9000000),
                    dict(blend=1, v_fac=30), dict(scanlines=1, blend=1)]
BLOOM_TIER_GEOMS = [(640, 480, R.FMT_BGRA), (64, 48, R.FMT_RGB), (1920, 1080, R.FMT_RGBA), (100, 300, R.FMT_BGR)]


def bloom_tier_case(knobs, geom):
    """test_bloom_lane_per_scanline_tiers_and_geometries"""
    outw, outh, ofmt = geom
    return ("ntscbloom", outw, outh, ofmt, 320, 240, R.FMT_BGRA, 24, dict(as_color=1, hue=33), knobs)


LAYOUT_FALLBACK_XOFFSETS = ((24, False), (16, True), (4, True))                   # (xoffset, padded layout kept)


def layout_fallback_case(xoff):
    """test_padded_signal_layout_falls_back_for_rows_it_cannot_hold"""
    return ("ntsc",) + _STD + (30, dict(as_color=1, xoffset=xoff, yoffset=1), dict(scanlines=1))


# test_rectangle_running_over_the_line_end (its xoffset 150 part compares the encoder alone and stays with the test)
LINE_END_CASES = [("ntsc",) + _STD + (24, dict(as_color=1, xoffset=4), {}),
                  ("ntsc",) + _STD + (0, dict(as_color=1, xoffset=16, yoffset=1), dict(scanlines=1))]

# test_library_picks_the_shape_by_batch_size: 300 fields, one pass
SHAPE_PICK_CASE = ("ntsc", 96, 240, R.FMT_BGRA, 64, 48, R.FMT_BGRA, 24, dict(as_color=1), dict(scanlines=1))
SHAPE_PICK_N = 300

# test_padded_signal_layout_is_what_the_fused_path_runs: (name, row); the ntsc / ntscp0 names take the row of CASES, the others
# that row of F4_CASES
PADDED_LAYOUT = [("ntsc", 0), ("ntsc", 1), ("ntsc", 2), ("ntsc", 5), ("ntsc", 9), ("ntsc", 13), ("ntscp0", 18), ("snes", 1), ("temp", 1),
                 ("pv1k", 1), ("nesrgb", 1), ("ntscbloom", 1), ("pv1kbloom", 1), ("vhslcg", 1), ("ntscnovsync", 1)]


def padded_layout_case(name, row):
    if name in ("ntsc", "ntscp0"):
        return renamed(name, CASES[row])
    return (name,) + F4_CASES[row]


F4_NAMES = ("snes", "temp", "pv1k")                                               # test_f4_systems_parity: every row of F4_CASES
BLOOM_ROWS = (0, 1, 2, 3, 4, 5)                                                   # test_bloom_*_parity: rows of F4_CASES
VARIANT_NAMES = ("vhslcg", "ntscnovsync", "ntscnohsync", "ntschipass")            # test_build_time_variants_parity
VARIANT_CASES = (1, 3, 7, 8)                                                      # ... rows of CASES


# ---------------------------------------------------------------------------------------------------------------------------
# the recipe of _run_case
# ---------------------------------------------------------------------------------------------------------------------------
def image(case, k):
    """field k's image [h, w, bpp]; the same for any batch size"""
    w, h, ifmt = case[4], case[5], case[6]
    return R.synth_image(w, h, R.bpp4fmt(ifmt), 777 + 13 * k, "random" if k % 2 == 0 else "bars")


def images(case, n):
    return np.stack([image(case, k) for k in range(n)])


def field_of(k, step):
    return (k ^ step) & 1


def frame_of(k, step):
    """the frame toggles after passes 0, 2, 4, ... (video_convert.c:259-267)"""
    return ((k >> 1) ^ ((step + 1) >> 1)) & 1


def dco_of(name, k):
    return (2 * k + 1) % 6 if name.startswith(("pv1k", "temp")) else (k + 1) % 3


def is_reference(lib):
    return isinstance(lib, R.RefLib)


def checker_crt(lib, case, k, img=None):
    """struct CRT + NTSC_SETTINGS of field k before pass 0, on either checker.  The progressive systems' settings have no field / frame
    (crtref.PROGRESSIVE_SYSTEMS) and no as_color / raw: the oracle's common struct takes them, as _run_case hands them over, and the
    oracle must ignore them; the reference's struct has no such members, so it gets the ones it has."""
    name, outw, outh, ofmt, w, h, ifmt, noise, skw, knobs = case
    img = image(case, k) if img is None else img
    c = lib.new_crt(outw, outh, ofmt)
    for kk, v in knobs.items():
        c.set(kk, v)
    if is_reference(lib) and lib.system in R.PROGRESSIVE_SYSTEMS:
        skw = {kk: v for kk, v in skw.items() if kk in lib.soff}
    c.settings(np.concatenate([img, img[-1:]], axis=0), format=ifmt, w=w, h=h, **skw)      # row h is addressable: crt_ntsc.c:263
    checker_walk(lib, c, k, 0)
    if lib.system in R.DOT_CRAWL_SYSTEMS:
        c.sset("dot_crawl_offset", dco_of(name, k))
    return c


def checker_walk(lib, c, k, step):
    """field / frame of field k in pass `step`"""
    if is_reference(lib) and lib.system in R.PROGRESSIVE_SYSTEMS:
        return
    c.sset("field", field_of(k, step))
    c.sset("frame", frame_of(k, step))


# ---------------------------------------------------------------------------------------------------------------------------
# the NES table (test_nes_parity): new PPU pixels, hue, dot crawl offset and border colour every pass
# ---------------------------------------------------------------------------------------------------------------------------
NES_N, NES_STEPS = 3, 4
NES_BORDERS = [0x21, 0x16, 0x1c0 | 0x2a, 0x0d]


def nes_ppu(step, k):
    return R.synth_ppu(256, 240, 31 * step + k)


def nes_settings(step, k):
    return dict(w=256, h=240, dot_crawl_offset=(step + k) % 3, hue=(step * 50) % 360, border_color=NES_BORDERS[step])


def nes_checker_crt(lib, case):
    name, outw, outh, noise, knobs = case
    c = lib.new_crt(outw, outh, R.FMT_BGRA)
    for kk, v in knobs.items():
        c.set(kk, v)
    return c


def nes_checker_pass(c, step, k, fused):
    """settings + crt_modulate of pass `step`.  The fused path starts every field from a crt_init-clean analog[] (documented batch
    semantics): mirrored in the checker by re-running setup_field on a zeroed signal"""
    ppu = nes_ppu(step, k)
    c.settings(np.concatenate([ppu, ppu[-1:]], axis=0), **nes_settings(step, k))
    if fused:
        c.analog[:] = 0
        c.sset("field_initialized", 0)
    c.modulate()


# ---------------------------------------------------------------------------------------------------------------------------
# the rand()-noise VHS builds (_vhs_fieldpass): the decoder's noise is the C library's rand() stream (crt_core.c:344-351).  Field k's
# generator starts at srand(seed_k) and carries over from pass to pass, and BOTH checkers draw from the one stream of the process:
# a checker runs a field's whole sequence under srand(seed_k), then the other checker runs it under the same seed; never interleaved.
# ---------------------------------------------------------------------------------------------------------------------------
VHS_NAMES = ("vhs", "vhsbloom", "vhslp", "vhsep")
VHS_NOISES = (0, 12, 40)
VHS_N, VHS_STEPS, VHS_SEEDS = 3, 3, [1, 77, 20260924]
VHS_SIZE, VHS_WIDE_SIZE = (832, 624), (1920, 1080)


def srand(lib, seed):
    """both spellings reach the process's libc; the reference's goes through its own library as its callers' would"""
    if is_reference(lib):
        lib.srand(seed)
    else:
        _LIBC.srand(C.c_uint(seed))


def vhs_images(size):
    w, h = size
    return np.stack([R.synth_image(w, h, 4, 60 + k, "random" if k != 1 else "bars") for k in range(VHS_N)])


def vhs_sequence(lib, sysname, fused, noise, size, k, img, stages=False):
    """field k's VHS_STEPS passes on one checker -> [(inp, out, hsync, vsync, rn, ccf)] (stages: + analog, ccf after modulate)"""
    w, h = size
    c = lib.new_crt(w, h, R.FMT_BGRA)
    c.set("scanlines", 1)
    c.settings(np.concatenate([img, img[-1:]]), format=R.FMT_BGRA, w=w, h=h, as_color=1, field=k & 1, frame=0, do_aberration=0)
    srand(lib, VHS_SEEDS[k])
    per = []
    for step in range(VHS_STEPS):
        if fused:
            c.analog[:] = 0                        # batch semantics: clean analog[] per field-pass
        c.modulate()
        mod = (np.array(c.analog).copy(), np.array(c.ccf).copy()) if stages else ()
        c.demodulate(noise)
        per.append((np.array(c.inp).copy(), c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn"), np.array(c.ccf).copy()) + mod)
        c.sset("field", c.sget("field") ^ 1)
    return per


# test_vhs_rand_noise_many_seeds: one encoded field under 40 generator seeds, two crt_demodulate calls in a row
MANY_SEEDS_NOISES = (7, 100)
MANY_SEEDS_N, MANY_SEEDS_SIZE = 40, (96, 240)
MANY_SEEDS = [1 + 7919 * k for k in range(MANY_SEEDS_N)]


def many_seeds_analog(lib):
    """a properly encoded field (the decoder must find its sync pulses, or it reads past inp[] like the reference would), the same
    for every seed"""
    w, h = MANY_SEEDS_SIZE
    img = R.synth_image(w, h, 4, 4242)
    c0 = lib.new_crt(w, h, R.FMT_BGRA)
    c0.settings(np.concatenate([img, img[-1:]]), format=R.FMT_BGRA, w=w, h=h, as_color=1, field=0, frame=0, do_aberration=0)
    c0.modulate()
    return np.array(c0.analog).copy()


def many_seeds_sequence(lib, analog, noise, k):
    """seed k: -> [(inp, out, hsync, vsync, rn)] of the two calls"""
    w, h = MANY_SEEDS_SIZE
    c = lib.new_crt(w, h, R.FMT_BGRA)
    c.analog[:] = analog
    srand(lib, MANY_SEEDS[k])
    per = []
    for step in range(2):
        c.demodulate(noise)
        per.append((np.array(c.inp).copy(), c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn")))
    return per


# ---------------------------------------------------------------------------------------------------------------------------
# the wild sync states (test_wild_sync_states_against_the_oracle): fields started far from lock, three passes
# ---------------------------------------------------------------------------------------------------------------------------
WILD_PARAMS = [("ntsc", 24, 0, 0), ("ntsc", 24, 150, 0), ("ntsc", 520, 60, 1), ("snes", 24, 100, 0), ("pv1k", 12, 90, 0),
               ("nes", 24, 80, 0), ("ntscbloom", 24, 40, 0), ("ntsc", 24, 150, 1), ("snes", 24, 100, 1), ("nes", 24, 80, 1)]
WILD_HS0 = [0, 3, 30, 60, 140, 300, 500, 700, 880, 892, 905, 909]
WILD_VS0 = [0, 4, 9, 100, 180, 250, 255, 258, 261]
WILD_STEPS, WILD_OUT = 3, (640, 480)


def wild_inputs(name, n):
    """-> dict(base images [uniq, h, w(, 4)], hs, vs, fields, uniq, check: the fields the test looks at)"""
    nes = name == "nes"
    w, h = (256, 240) if nes else (640, 480)
    uniq = min(n, 24)
    if nes:
        base = np.stack([R.synth_ppu(w, h, 8100 + k) for k in range(uniq)]).astype(np.int16)
    else:
        base = np.stack([R.synth_image(w, h, 4, 8100 + k, "bars" if k % 3 == 1 else "random") for k in range(uniq)])
        base[2::3] //= 16                                  # dark pictures: a noisy candidate line crosses the threshold more easily
    hs = [WILD_HS0[(k // uniq + k) % len(WILD_HS0)] for k in range(n)]
    vs = [WILD_VS0[(k // uniq * 5 + k) % len(WILD_VS0)] for k in range(n)]
    return dict(nes=nes, w=w, h=h, uniq=uniq, base=base, hs=hs, vs=vs, fields=[k & 1 for k in range(n)], check=wild_check(n))


def wild_check(n):
    """the fields the test compares with the checker: all of a small batch, every seventh and the last of a large one"""
    return list(range(n)) if n <= 64 else list(range(0, n, 7)) + [n - 1]


def wild_checker_crt(lib, name, inp, k):
    nes = inp["nes"]
    c = lib.new_crt(WILD_OUT[0], WILD_OUT[1], R.FMT_BGRA)
    c.set("scanlines", 1)
    c.set("hsync", inp["hs"][k])
    c.set("vsync", inp["vs"][k])
    b = inp["base"][k % inp["uniq"]]
    pad = np.concatenate([b, b[-1:]])
    if nes:
        c.settings(pad.astype(np.uint16), w=inp["w"], h=inp["h"], dot_crawl_offset=k % 3, hue=0)
    else:
        c.settings(pad, format=R.FMT_BGRA, w=inp["w"], h=inp["h"], as_color=1, field=inp["fields"][k], frame=0)
        if name in ("snes", "pv1k"):
            c.sset("dot_crawl_offset", k % 3)
    return c


def wild_checker_modulate(c, nes):
    c.analog[:] = 0                                # batch semantics: every field-pass starts from a clean analog[]
    if nes:
        c.sset("field_initialized", 0)
    c.modulate()


# ---------------------------------------------------------------------------------------------------------------------------
# every (table, variant, case) a GPU test runs, for the pin: TABLES[table] = dict(kind, n, steps, cases = {id: case})
# ---------------------------------------------------------------------------------------------------------------------------
TABLES = {}


def _table(table, kind, n, steps, cases):
    TABLES[table] = dict(kind=kind, n=n, steps=steps, cases=dict(cases))


def _rows(names, rows, source, plain=False):
    return [("%s-%d" % (name, r), (name,) + source[r] if plain else renamed(name, source[r])) for name in names for r in rows]


# "run": the recipe of _run_case.  n, steps: the largest any GPU test runs the table at.
_table("CASES", "run", 3, 4, [("%s-%d" % (c[0], i), c) for i, c in enumerate(CASES)])
_table("WIDE_CASES", "run", 5, 3, [("%s-%d" % (c[0], i), c) for i, c in enumerate(WIDE_CASES)])
_table("RANDOM", "run", 2, 2, [("seed%d" % (RANDOM_SEED0 + s), random_seed_case(s)) for s in range(RANDOM_SEEDS)])
_table("RANDOM_WIDE", "run", 2, 2, [("seed%d-%s" % (RANDOM_WIDE_SEED0 + s, random_wide_seed_case(s)[0]), random_wide_seed_case(s))
                                    for s in range(RANDOM_WIDE_SEEDS)])
_table("RANDOM_BLOOM", "run", 3, 2, [("seed%d-%s" % (RANDOM_BLOOM_SEED0 + s, BLOOM_NAMES[s % 3]), random_bloom_seed_case(s))
                                     for s in range(RANDOM_BLOOM_SEEDS)])
_table("FIR", "run", 3, 2, _rows(["ntscfir%d" % t for t in FIR_TAPS], FIR_CASES, CASES))
_table("FIR_ENVELOPE", "run", 3, 2, [("ntscfir7-%d" % i, fir_envelope_case(k)) for i, k in enumerate(FIR_ENVELOPE_KNOBS)])
_table("F4_CASES", "run", 3, 3, _rows(F4_NAMES, range(len(F4_CASES)), F4_CASES, plain=True))
_table("PADDED_LAYOUT", "run", 3, 4, [("%s-%d" % (nm, r), padded_layout_case(nm, r)) for nm, r in PADDED_LAYOUT if nm not in ("ntsc", "ntscp0")])
_table("BUILD_VARIANTS", "run", 3, 3, _rows(VARIANT_NAMES, VARIANT_CASES, CASES))
_table("BLOOM", "run", 5, 3, _rows(BLOOM_NAMES, BLOOM_ROWS, F4_CASES, plain=True))
_table("BLOOM_TIERS", "run", 3, 2, [("knobs%d-%dx%d" % (i, g[0], g[1]), bloom_tier_case(k, g))
                                    for i, k in enumerate(BLOOM_TIER_KNOBS) for g in BLOOM_TIER_GEOMS])
_table("PV1K_TIERS", "run", 3, 3, [("pv1k-knobs%d" % i, pv1k_tier_case(k)) for i, k in enumerate(PV1K_TIER_KNOBS)])
_table("BETWEEN_ENVELOPES", "run", 3, 3, [("ntsc-saturation%d" % s, between_the_envelopes_case(s)) for s in ENVELOPE_SATURATIONS])
_table("LAYOUT_FALLBACK", "run", 3, 2, [("ntsc-xoffset%d" % x, layout_fallback_case(x)) for x, _ in LAYOUT_FALLBACK_XOFFSETS])
_table("LINE_END", "run", 3, 2, [("ntsc-xoffset%d" % c[8]["xoffset"], c) for c in LINE_END_CASES])
# 300 fields, one pass: the pin takes them fifty at a time (case: (the case, first field, one past the last))
_table("SHAPE_PICK", "run", SHAPE_PICK_N, 1, [("ntsc-fields%d" % k0, (SHAPE_PICK_CASE, k0, min(k0 + 50, SHAPE_PICK_N))) for k0 in range(0, SHAPE_PICK_N, 50)])
_table("NES_CASES", "nes", NES_N, NES_STEPS, [("%s-%d-%s" % (c[0], i, "fused" if f else "stagewise"), (c, f))
                                              for i, c in enumerate(NES_CASES) for f in (False, True)])
_table("VHS", "vhs", VHS_N, VHS_STEPS, [("%s-noise%d-%s" % (nm, nz, "fused" if f else "stagewise"), (nm, f, nz, VHS_SIZE))
                                        for nm in VHS_NAMES for nz in VHS_NOISES for f in (False, True)]
       + [("vhs-noise12-fused-1920x1080", ("vhs", True, 12, VHS_WIDE_SIZE))])
_table("VHS_MANY_SEEDS", "seeds", MANY_SEEDS_N, 2, [("vhs-noise%d" % nz, nz) for nz in MANY_SEEDS_NOISES])


def _wild_cases():
    out = []
    for name, n, noise in sorted({p[:3] for p in WILD_PARAMS}):
        check = wild_check(n)
        for i in range(0, len(check), 12):               # twelve fields per test id
            out.append(("%s-n%d-noise%d-part%d" % (name, n, noise, i // 12), (name, n, noise, check[i:i + 12])))
    return out


_table("WILD_SYNC", "wild", None, WILD_STEPS, _wild_cases())

# Field-passes that crtref.reads_past_inp takes out, {table: {case id: count}}: computed on the CPU with both checkers built, asserted
# exactly by tests/test_parity_pin_cpu.py.  No entry: none.
EXCLUDED = {
    # every table of the _run_case recipe, the NES table: none (the four nesrgb seeds of RANDOM_WIDE included).  The VHS tables'
    # GPU tests compare every field unconditionally, so does the pin.
    # The wild sync states are made to start far from lock: some fields leave in their first pass (3 passes each), under heavy noise
    # some later.  35 of the 3 * (5 * 24 + 12 + 76) = 624 field-passes looked at:
    "WILD_SYNC": {"nes-n24-noise80-part0": 3, "ntsc-n24-noise0-part0": 3, "ntsc-n24-noise150-part0": 5, "ntsc-n24-noise150-part1": 8,
                  "ntsc-n520-noise60-part1": 3, "ntsc-n520-noise60-part6": 3, "ntscbloom-n24-noise40-part0": 3, "pv1k-n12-noise90-part0": 4,
                  "snes-n24-noise100-part0": 3},
}


def excluded(table, cid=None):
    per = EXCLUDED.get(table, {})
    return sum(per.values()) if cid is None else per.get(cid, 0)


def excludes_nothing(table):
    """the GPU tests of such a table assert that no field dropped out"""
    return excluded(table) == 0

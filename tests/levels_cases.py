"""Cases and expected values of the LEVEL knobs -- black point and white point per field beside the other five
(crthip_knobs_prepare7 + crthip_bind_levels; every per-field-knob entry point reads the binding); no tests in here.

A case row is (noise, mon_hue, saturation, brightness, contrast, black_point, white_point).  The two new values are the first knobs
that enter the ENCODER's arithmetic: ire = (BLACK_LEVEL + black_point) + (((y + i + q) * white) >> 10), white = WHITE_LEVEL *
white_point / 100 (crt_ntsc.c:311-318), and the black point once more the decoder's bright (crt_core.c:305).  Expected pictures,
signals and states never come from the library: the oracle runs once per field with that field's seven knobs (field-pass), or the
reference's serial loop runs on ONE struct CRT whose knobs are turned between the fields (sequence mode) -- the construction of
tests/picknobs_cases.py.  Geometry and parities are those of tests/knobs_cases.py: 64x48 -> 160x120, 3 to 6 fields."""
import ctypes as C

import numpy as np

import crtref as R
import encoder_cases as EC
import knobs_cases as KC
import picknobs_cases as PK
import seqknobs_cases as SK
from test_phosphor_cpu import display_step_np

SMALL = KC.SMALL
BLEND = SK.BLEND
FAST_WHITE, FAST_IRE = EC.FAST_WHITE, EC.FAST_IRE      # encoder_fast_ok: |white| and |ire_base| below 2^13 for the 24-bit kernels


def levels_of(name, row):
    """(white, ire_base) of a row as crthip_params_finalize derives them: C's truncating division"""
    sysd = EC.oracle(name).sys
    return EC.c_div(sysd.white_level * row[6], 100), sysd.black_level + row[5]


def at(name, white=None, ire=None, noise=24, hue=0, sat=10, brightness=None, contrast=180):
    """a row whose encoder levels are exactly (white, ire_base) -- None: the system's defaults --, from the system's own WHITE_LEVEL /
    BLACK_LEVEL as tests/encoder_cases.py finds them; brightness None = ire_base, which keeps the decoder's bright at 0"""
    sysd = EC.oracle(name).sys
    wp = 100 if white is None else EC.white_point_for(name, white)
    bp = 0 if ire is None else ire - sysd.black_level
    return (noise, hue, sat, sysd.black_level + bp if brightness is None else brightness, contrast, bp, wp)


def bound_batches(name):
    """{id: rows}: one batch entirely inside the fast-path bound with fields ON its last values (white +-8191, ire_base +-8191, both
    at once), and four batches with a SINGLE field on the first value outside (white +-8192, ire_base +-8192): the whole call then
    takes the exact kernels, with identical samples"""
    inside = [at(name), at(name, white=8191), at(name, ire=-8191), at(name, white=-8191, sat=14), at(name, ire=8191),
              at(name, white=8191, ire=-8191, noise=30)]
    out = {"inside": inside}
    for cid, kw in (("white+", dict(white=8192)), ("white-", dict(white=-8192)), ("ire+", dict(ire=8192)), ("ire-", dict(ire=-8192))):
        out[cid] = [at(name), at(name, white=8191, ire=8191), at(name, **kw), at(name, white=-8191)]
    return out


D = (24, 0, 10, 0, 180)                                 # the other five where they are not the point
# at least three fields with pairwise distinct (black, white): with desth no multiple of 64 a wavefront holds rows of two fields
STRADDLE = [D + (0, 100), D + (10, 80), D + (-5, 120), D + (3, 55), D + (-12, 140)]
# white point 0 (a flat field), negative, black point of both signs, and a black point that moves ONE field's bright across
# +-2600 | +-2601 (brightness 0: bright = -(7 + black_point)) while its neighbours stay in tier 0
EDGES = [D + (0, 0), D + (0, -50), D + (20, 100), D + (-20, 100), D + (-2607, 100), D + (-2608, 100)]
EDGES_NEG = [D + (0, 100), D + (2593, 100), D + (2594, 100), D + (0, 100)]
EDGE_FLOORS = {"edges": [0, 0, 0, 0, 0, 2], "edges-neg": [0, 0, 2, 0]}
# with the other five: a clean field inside the noisy batch, a field whose contrast is above the 24-bit tier's bound (2^23), the
# saturations / hues of KC.SMALL_TRIPLES that spread the lines of a wavefront over the chroma tiers
COMBINED = [t + pc + lv for t, pc, lv in zip(KC.SMALL_TRIPLES,
                                             [(0, 180), (5, 200), (-40, 240), (0, 1 << 23), (33, 90), (0, -200)],
                                             [(0, 100), (8, 90), (-6, 115), (4, 70), (-15, 130), (2, -60)])]
BATCHES = {"straddle": STRADDLE, "edges": EDGES, "edges-neg": EDGES_NEG, "combined": COMBINED}


def corner_images(geo):
    """the solid cube corners and opposite-corner runs of tests/encoder_cases.py (they maximise |y + i + q|), as BGRA"""
    w, h = geo["w"], geo["h"]
    rgb = [EC.solid_image(w, h, 7), EC.solid_image(w, h, 0), EC.solid_image(w, h, 4), EC.solid_image(w, h, 3),
           EC.runs_image(w, h, 1, 0), EC.runs_image(w, h, 2, 3)]
    return [EC.lay(im, R.FMT_BGRA) for im in rgb]


def corner_rows(name):
    """the corner images at the last fast values of both levels, in all four sign combinations, and at the defaults"""
    return [at(name, white=8191, ire=8191), at(name, white=8191, ire=-8191), at(name, white=-8191, ire=8191),
            at(name, white=-8191, ire=-8191), at(name), at(name, white=8191, noise=0)]


def per_system(name, n):
    """n rows for the one-case-per-system tests: KC's drawn triples, level pairs that differ per field, one of them on the system's
    own fast bound"""
    trip = KC.drawn_triples(n, 700 + n, noise_max=40, sat_lo=-15, sat_hi=30)
    rows = []
    lv = [(0, 100), (9, 85), (-7, 118), None, (4, 60), (-11, -40)]
    for k, t in enumerate(trip):
        if lv[k % 6] is None:
            rows.append(at(name, white=8191, ire=-8191, noise=int(t[0]), hue=int(t[1]), sat=int(t[2])))
        else:
            rows.append(tuple(int(v) for v in t) + (0, 180) + lv[k % 6])
    return rows


def default_images(geo, n):
    return [KC.image(geo, k) for k in range(n)]


def oracle_fields7(name, geo, rows, steps=1, crt_knobs=None, seeds=None, fmt=R.FMT_BGRA, images=None, ifmt=R.FMT_BGRA):
    """PK.oracle_fields5 with black point and white point per field as well: field k of a batch as an n = 1 call of the reference
    gives it, `steps` field-passes in a row on its own CRT.  Per field a list of per-step dicts."""
    libc = C.CDLL(None)
    orc = R.Oracle(name)
    dc = orc.system in R.DOT_CRAWL_SYSTEMS
    out = []
    for k, (noise, hue, sat, brightness, contrast, black_point, white_point) in enumerate(rows):
        c = orc.new_crt(geo["outw"], geo["outh"], fmt)
        c.set("scanlines", 1)
        for a, v in (crt_knobs or {}).items():
            c.set(a, v)
        for a, v in (("hue", hue), ("saturation", sat), ("brightness", brightness), ("contrast", contrast),
                     ("black_point", black_point), ("white_point", white_point)):
            c.set(a, v)
        field, frame = KC.parity(k)
        img = images[k] if images is not None else KC.image(geo, k)
        c.settings(np.concatenate([img, img[-1:]], axis=0), format=ifmt, w=geo["w"], h=geo["h"], as_color=1)
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
            if orc.system not in R.PROGRESSIVE_SYSTEMS:
                field ^= 1
                if step % 2 == 0:
                    frame ^= 1
                c.sset("field", field)
                c.sset("frame", frame)
        out.append(per)
    return out


# sequence mode: a recorded session in which the user turns both levels mid-video (SK.SIX's noise / hue / saturation)
SEQ_ROWS = [t + pc + lv for t, pc, lv in zip(SK.SIX, [(0, 180), (10, 180), (0, 200), (-2600, 180), (0, 150), (0, 180)],
                                             [(0, 100), (6, 100), (6, 88), (-6, 88), (-6, 120), (12, -70)])]
SETS_FIRST = SK.SETS_FIRST                             # three ragged sets: 1, 4 and 2 fields
SETS_ROWS = SEQ_ROWS + [(45, -100, 25, 0, 200, -9, 64)]

SEQ_CASES = {c["id"]: c for c in [
    PK.seq_case("levels", SEQ_ROWS),
    PK.seq_case("levels-blend", SEQ_ROWS, geo=BLEND, knobs=dict(blend=1)),
    PK.seq_case("levels-sets", SETS_ROWS, set_first=SETS_FIRST, incoming="per_set"),
    PK.seq_case("levels-sets-blend", SETS_ROWS, geo=BLEND, knobs=dict(blend=1), set_first=SETS_FIRST, incoming="per_set"),
]}


def serial_loop7(lib, case, lo, hi, init, state_in):
    """PK.serial_loop5 with all seven knobs turned between the fields: the reference's loop on ONE struct CRT over fields [lo, hi)"""
    par, dco = SK.parities(case), SK.dot_crawl(case)
    c = SK._new_crt(lib, case)
    c.out[:] = init.reshape(-1)
    c.set("hsync", state_in[0])
    c.set("vsync", state_in[1])
    c.set("rn", state_in[2])
    want = []
    for k in range(lo, hi):
        noise, hue, sat, brightness, contrast, black_point, white_point = case["rows"][k]
        if case["mode"] != "keep":
            c.out[:] = display_step_np(c.out, R.FMT_BGRA, case["mode"])
        for a, v in (("hue", hue), ("saturation", sat), ("brightness", brightness), ("contrast", contrast),
                     ("black_point", black_point), ("white_point", white_point)):
            c.set(a, v)
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
        want += serial_loop7(use, case, lo, hi, SK._init_of_set(case, init, s), inc[s])
    if lib is None:
        _EXPECTED[case["id"]] = want
    return want


_FIELDS = {}


def expected(key, fn):
    """an expected result is computed once and shared by the tests that need it: treat it as read-only"""
    if key not in _FIELDS:
        _FIELDS[key] = fn()
    return _FIELDS[key]


def fast_model(name, rows):
    """the dispatch bound restated: the 24-bit kernels iff EVERY field's |white| and |ire_base| are below 2^13"""
    lv = [levels_of(name, r) for r in rows]
    return max(abs(w) for w, _ in lv) < FAST_WHITE and max(abs(b) for _, b in lv) < FAST_IRE

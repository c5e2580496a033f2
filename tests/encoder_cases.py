"""Hand-made images for the encoder (TEST INFRASTRUCTURE ONLY; numpy and the CPU oracle, no GPU).

Every earlier GPU test feeds crt_encode.hip random bytes, colour bars or random PPU pixels.  Here the images are made to reach the
corners of its arithmetic, and the knobs sit ON the bounds of its dispatch (encoder_fast_ok, crt_encode.hip):

* `extremes`  the eight corners of the RGB cube as solid fields, and 1:1 images (w == destw: source column = sample) whose rows are runs
              of two opposite corners -- run lengths RUNS, a run edge on every pixel of STARTS (0 .. 3, and 15 .. 17, 31 .. 33: the edges
              of the 16- and 32-pixel image tiles): the full-swing steps that test the one-multiply low-passes;
* `phase`     1:1 images of period 4 (PV-1000: 5) in x whose positions hold the colours of largest / smallest I and Q, white or black, in
              every rotation and both polarities: whatever the line's carriers are, one row is sign-matched to them;
* `floors`    the colours whose Y, I or Q sum (crt_ntsc.c:307-309, before >> 14) lies within +-2 of a multiple of 16384, found by an
              exhaustive search over all 2^24 colours, and the grey ramp;
* `random`    the control: crtref.synth_image as every other test uses it;
* NES         the PPU ramp p = (x + 256 * (y & 1)) & 511 (every 9-bit pixel on each line pair) and crtref.synth_ppu, 256, 8, 7 and 4
              pixels wide (below 8 the NES takes the per-lane loop of k_active instead of its table kernel).

Images are generated in memory; nothing is a fixture.  A case is 2 .. 4 fields (both field parities, both frame values), two passes
with the field toggled, to a 64 x 48 picture; the signal has the system's full line length whatever the picture.  What a case claims
to reach is asserted by tests/test_encoder_cpu.py, which also pins the oracle to the real reference on every case; expected() and
images() are what a GPU test of the same cases compares against."""
import ctypes as C

import numpy as np

import crtref as R

OUTW, OUTH, OUTFMT = 64, 48, R.FMT_BGRA
KY, KI, KQ = (19595, 38470, 7471), (39059, -18022, -21103), (13894, -34275, 20382)     # crt_ntsc.c:307-309, by (R, G, B)
RUNS = (1, 2, 3, 4, 5, 8, 16, 64)
STARTS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33)
RUN_ROWS = [(run, start) for run in RUNS for start in STARTS]
CORNERS = [(255 * (c >> 2 & 1), 255 * (c >> 1 & 1), 255 * (c & 1)) for c in range(8)]  # corner c and corner 7 - c are opposite
RAND_BUILDS = ("vhs", "vhslp")                  # the decoder's noise is the C library's rand() (crt_core.c:344-351)
SEEDS = (1, 77, 20260924, 5)
FAST_WHITE, FAST_IRE, FAST_NOISE = 1 << 13, 1 << 13, 1 << 15       # encoder_fast_ok: |white|, |ire_base|, |noise| below these

_ORC = {}


def oracle(name):
    if name not in _ORC:
        _ORC[name] = R.Oracle(name)
    return _ORC[name]


def c_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def destw(name):
    """width of the encoder's rectangle for an image that is not `raw` (crt_ntsc.c:132-133, 148-152; bloom builds: 55500 / 65536)"""
    av = oracle(name).av_len
    return (av * 55500) >> 16 if R.is_bloom(name) else av


def is_nes(name):
    return oracle(name).system == R.SYS_NES


def is_progressive(name):
    return oracle(name).system in R.PROGRESSIVE_SYSTEMS


# ---------------------------------------------------------------------------------------------------------------------------
# image families, by meaning (R, G, B)
# ---------------------------------------------------------------------------------------------------------------------------
def _extreme(coef, largest):
    return tuple(255 if (c > 0) == largest else 0 for c in coef)


COLOURS = {"I": _extreme(KI, True), "i": _extreme(KI, False), "Q": _extreme(KQ, True), "q": _extreme(KQ, False),
           "W": (255, 255, 255), "K": (0, 0, 0)}
_SWAP = {"I": "i", "i": "I", "Q": "q", "q": "Q", "W": "K", "K": "W"}
OVERSHOOT = (COLOURS["I"], COLOURS["Q"], (255, 255, 0), (255, 0, 0))
PHASE_BASES = {4: ("IIii", "QqqQ", "IqiQ", "WKWK", "WWKK"), 5: ("IIWii", "QqqQK", "IqiQW", "WWKKK")}


def phase_rows(period):
    """every rotation and both polarities of the bases, then the six constant rows"""
    rows = []
    for base in PHASE_BASES[period]:
        for pol in (0, 1):
            b = "".join(_SWAP[ch] for ch in base) if pol else base
            rows += [b[r:] + b[:r] for r in range(period)]
    return rows + [ch * period for ch in "IiQqWK"]


def phase_image(name, w=None):
    period = oracle(name).ccs
    rows = phase_rows(period)
    w = w or destw(name)
    img = np.zeros((len(rows), w, 3), dtype=np.uint8)
    x = np.arange(w)
    for r, pat in enumerate(rows):
        table = np.array([COLOURS[ch] for ch in pat], dtype=np.uint8)
        img[r] = table[x % period]
    return img


def runs_image(w, h, pair, variant, colours=None):
    """row r: runs of corner `pair` and its opposite (or of the two `colours`), (run, start) = RUN_ROWS[(r + h * variant) % 80]: a run
    edge on pixel `start`; variants 2 and 3 start with the other colour"""
    a, b = colours or (CORNERS[pair], CORNERS[7 - pair])
    a, b = np.array(a, dtype=np.uint8), np.array(b, dtype=np.uint8)
    if variant & 2:
        a, b = b, a
    x = np.arange(w)
    img = np.zeros((h, w, 3), dtype=np.uint8)
    for r in range(h):
        run, start = RUN_ROWS[(r + h * variant) % len(RUN_ROWS)]
        img[r] = np.where(((((x - start) // run) & 1) == 1)[:, None], b, a)
    return img


def solid_image(w, h, corner):
    return np.broadcast_to(np.array(CORNERS[corner], dtype=np.uint8), (h, w, 3)).copy()


_SEARCH = {}


def colour_sums():
    """Y, I, Q sums of all 2^24 colours, index (R << 16) | (G << 8) | B; computed once per session"""
    if "sums" not in _SEARCH:
        v = np.arange(256, dtype=np.int32)
        r, g, b = v[:, None, None], v[None, :, None], v[None, None, :]
        _SEARCH["sums"] = tuple((k[0] * r + k[1] * g + k[2] * b).reshape(-1) for k in (KY, KI, KQ))
    return _SEARCH["sums"]


FLOOR_RESIDUES = (0, 1, 2, 16382, 16383)
FLOOR_CAP = 100


def floor_colours():
    """{(channel, negative, residue): colour indices}: the sums within +-2 of a multiple of 16384, at most FLOOR_CAP per class,
    spread evenly over the class"""
    if "floors" not in _SEARCH:
        found = {}
        for ch, s in zip("YIQ", colour_sums()):
            res = s & 16383
            for want in FLOOR_RESIDUES:
                for neg in (False, True):
                    idx = np.flatnonzero((res == want) & ((s < 0) == neg))
                    if idx.size:
                        found[(ch, neg, want)] = idx[np.linspace(0, idx.size - 1, min(FLOOR_CAP, idx.size)).astype(np.int64)]
        _SEARCH["floors"] = found
    return _SEARCH["floors"]


def floors_image():
    """64 pixels wide, below 48 rows: every class of floor_colours, then the grey ramp"""
    idx = np.concatenate([v for _, v in sorted(floor_colours().items())])
    rgb = np.stack([idx >> 16, (idx >> 8) & 255, idx & 255], axis=1).astype(np.uint8)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    px = np.concatenate([rgb, grey])
    h = (px.shape[0] + 63) // 64
    assert h < 48
    img = np.zeros((h * 64, 3), dtype=np.uint8)
    img[:px.shape[0]] = px
    return img.reshape(h, 64, 3)


def lay(rgb, fmt):
    """(h, w, 3) by meaning -> the pixel format's bytes; alpha alternates 0x00 / 0xff"""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    h, w = r.shape
    a = (((np.arange(w)[None, :] + np.arange(h)[:, None]) & 1) * 255).astype(np.uint8)
    order = {R.FMT_RGB: (r, g, b), R.FMT_BGR: (b, g, r), R.FMT_ARGB: (a, r, g, b), R.FMT_RGBA: (r, g, b, a),
             R.FMT_ABGR: (a, b, g, r), R.FMT_BGRA: (b, g, r, a)}[fmt]
    return np.ascontiguousarray(np.stack(order, axis=-1))


def ppu_ramp(w, h):
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    return ((x + 256 * (y & 1)) & 511).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------------
# knob table: from the oracle's constants of the system
# ---------------------------------------------------------------------------------------------------------------------------
def white_point_for(name, white):
    """white = WHITE_LEVEL * white_point / 100 (crt_ntsc.c:134, C's division)"""
    wl = oracle(name).sys.white_level
    for wp in range(c_div(white * 100, wl) - 3, c_div(white * 100, wl) + 4):
        if c_div(wl * wp, 100) == white:
            return wp
    raise ValueError((name, white))


def ire_knobs(name, ire_base):
    """ire_base = BLACK_LEVEL + black_point; brightness = ire_base keeps the decoder's `bright` at 0 (crt_core.c:305)"""
    return dict(black_point=ire_base - oracle(name).sys.black_level, brightness=ire_base)


WHITES = (8191, 8192, -8191, -8192, 1, 0, -100, 100)
IRES = (8191, 8192, -8191, -8192)
NOISES = (32767, 32768, -32767, -32768, 1, -1, 0)
HUES = (0, 33, -40, 350)
KNOB_NOISE = 24                  # white / ire_base / hue rows: the fused path runs its NOISE kernels (the scaled clamp); stage level has none


def knob_rows(name, full):
    """[(label, struct CRT knobs, noise, encoder hue, (white, ire_base) meant or None)]; full: the whole table, else the rows on either side of each bound"""
    rand = name in RAND_BUILDS
    noise = 12 if rand else KNOB_NOISE
    whites = WHITES if full else (8191, 8192, -8192)
    ires = IRES if full else (8191, -8191, -8192)
    rows = [("white%d" % v, dict(white_point=white_point_for(name, v)), noise, 0, (v, None)) for v in whites]
    rows += [("ire%d" % v, ire_knobs(name, v), noise, 0, (None, v)) for v in ires]
    if rand:
        rows += [("noise%d" % v, {}, v, 0, None) for v in (0, 40)]                # the noise values of the VHS tests of test_gpu_parity.py
    else:
        for v in (NOISES if full else (32767, 32768, -32768)):
            if v < 0 and R.is_bloom(name):
                continue                                                    # setup refuses negative noise in bloom builds
            rows.append(("noise%d" % v, {}, v, 0, None))
    if full:
        rows += [("hue%d" % v, {}, noise, v, None) for v in HUES]
        # all three at their last fast values at once, in four sign combinations: the sum the bound's comment adds up
        for sw, si, sn in ((1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1)):
            k = dict(white_point=white_point_for(name, sw * 8191))
            k.update(ire_knobs(name, si * 8191))
            rows.append(("corner%+d%+d%+d" % (sw, si, sn), k, sn * 32767, 0, (sw * 8191, si * 8191)))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------
SYSTEMS = ("ntsc", "ntscp0", "snes", "temp", "pv1k", "nesrgb", "nes", "vhslcg", "vhs", "vhslp", "ntscbloom", "ntschipass")
CASES = {}


def _case(cid, name, images, fmt=R.FMT_BGRA, n=4, knobs=None, noise=0, hue=0, raw=0, xoffset=0, family="", gpu_only=None, target=None):
    """images: field index -> (h, w, 3) by meaning, or (h, w) PPU pixels; noise: one value, or one per field (fieldpass_knobs).
    gpu_only: the reason why a case is compared GPU-against-oracle only (None: the oracle is pinned to the reference on it);
    target: the (white, ire_base) the knobs are meant to give (None: the system's levels) -- with the noise, what decides the side of
    encoder_fast_ok the case is meant for (intended_fast)"""
    assert cid not in CASES, cid
    CASES[cid] = dict(name=name, images=images, fmt=fmt, n=n, knobs=knobs or {}, noise=noise, hue=hue, raw=raw, xoffset=xoffset,
                      family=family, gpu_only=gpu_only, target=target)


def _mixed(name, w=None):
    """fields 0, 1: the phase image; fields 2, 3: runs of corner pairs 2 and 3 -- the image of the knob rows"""
    w = w or destw(name)
    h = len(phase_rows(oracle(name).ccs))

    def images(k):
        return phase_image(name, w) if k < 2 else runs_image(w, h, k, k)
    return images


def _nes_images(w, h, kind):
    def images(k):
        return ppu_ramp(w, h) if kind == "ramp" else R.synth_ppu(w, h, 8300 + k)
    return images


def _white_point_with_minus128(name, ppu):
    orc = oracle(name)
    pad = np.concatenate([ppu, ppu[-1:]]).astype(np.uint16)
    for wp in range(white_point_for(name, 8192), white_point_for(name, 8192) + 32):       # (the first one does, at every width of the table: three modulate calls at import)
        c = orc.new_crt(OUTW, OUTH, OUTFMT)
        c.set("white_point", wp)
        c.settings(pad, w=int(ppu.shape[1]), h=int(ppu.shape[0]), hue=0, dot_crawl_offset=0)
        c.sset("field_initialized", 0)
        c.modulate()
        if int(c.analog.min()) == -128:
            return wp
    raise ValueError("no white point puts -128 into analog[]")


def _build_table():
    for name in SYSTEMS:
        if is_nes(name):
            for w in (256, 8, 7, 4):
                for kind in ("ramp", "ppu"):
                    _case("%s-%s-w%d" % (name, kind, w), name, _nes_images(w, 16, kind), n=3, noise=KNOB_NOISE, family="nes")
            for label, knobs, noise, hue, target in knob_rows(name, True):
                _case("%s-%s" % (name, label), name, _nes_images(256, 16, "ramp"), n=3, knobs=knobs, noise=noise, hue=hue, family="knob",
                      target=target)
            for w in (8, 7, 4):
                _case("%s-white-8192-w%d" % (name, w), name, _nes_images(w, 16, "ppu"), n=3, noise=KNOB_NOISE,
                      knobs=dict(white_point=white_point_for(name, -8192)), family="knob", target=(-8192, None))
                # -128 in analog[] (what the fused path's CLAMP exists for) at the narrow widths too: the first white point beyond the
                # table's that puts it there, found on the oracle
                wp = _white_point_with_minus128(name, _nes_images(w, 16, "ppu")(0))
                _case("%s-minus128-w%d" % (name, w), name, _nes_images(w, 16, "ppu"), n=3, noise=KNOB_NOISE, knobs=dict(white_point=wp),
                      family="knob", target=(c_div(oracle(name).sys.white_level * wp, 100), None))
                # ... and without noise: only there is the clamp the kernel's own (with noise, noisy() ends in it)
                _case("%s-minus128-w%d-noise0" % (name, w), name, _nes_images(w, 16, "ppu"), n=3, noise=0, knobs=dict(white_point=wp),
                      family="knob", target=(c_div(oracle(name).sys.white_level * wp, 100), None))
            _case(name + "-minus128-ramp-noise0", name, _nes_images(256, 16, "ramp"), n=3, noise=0,
                  knobs=dict(white_point=white_point_for(name, 8192)), family="knob", target=(8192, None))
            continue
        dw = destw(name)
        fused_noise = 12 if name in RAND_BUILDS else KNOB_NOISE
        _case(name + "-solid-a", name, lambda k, dw=dw: solid_image(dw, 8, k), noise=fused_noise, family="extremes")
        _case(name + "-solid-b", name, lambda k, dw=dw: solid_image(dw, 8, 4 + k), noise=fused_noise, family="extremes")
        for variant in range(4 if name == "ntsc" else 2):
            _case("%s-runs%d" % (name, variant), name, lambda k, dw=dw, v=variant: runs_image(dw, 48, k, v), noise=fused_noise,
                  family="extremes")
        _case(name + "-phase", name, lambda k, name=name: phase_image(name), noise=fused_noise, family="phase")
        _case(name + "-phase-noise0", name, lambda k, name=name: phase_image(name), noise=0, n=2, family="phase")
        _case(name + "-floors", name, lambda k: floors_image(), noise=fused_noise, n=2, family="floors")
        _case(name + "-random", name, lambda k: R.synth_image(64, 48, 3, 8400 + k), noise=fused_noise, family="random")
        for label, knobs, noise, hue, target in knob_rows(name, name == "ntsc"):
            _case("%s-%s" % (name, label), name, _mixed(name), knobs=knobs, noise=noise, hue=hue, family="knob", target=target)
    # the pixel formats (ntsc; the SNES has no band limiting: what RGB -> YIQ floors to reaches the signal unfiltered)
    for name in ("ntsc", "snes"):
        for fmt, tag in ((R.FMT_RGB, "rgb"), (R.FMT_BGR, "bgr"), (R.FMT_ARGB, "argb"), (R.FMT_RGBA, "rgba"), (R.FMT_ABGR, "abgr")):
            _case("%s-floors-%s" % (name, tag), name, lambda k: floors_image(), fmt=fmt, noise=KNOB_NOISE, n=2, family="floors")
            _case("%s-mixed-%s" % (name, tag), name, _mixed(name), fmt=fmt, noise=KNOB_NOISE, family="extremes")
    _case("ntsc-white8191-rgb", "ntsc", _mixed("ntsc"), fmt=R.FMT_RGB, noise=KNOB_NOISE, knobs=dict(white_point=white_point_for("ntsc", 8191)),
          family="knob", target=(8191, None))
    # Beyond the white bound, where the 24-bit kernels WOULD wrap: (y + mi + mq) * white * 64 + (ire_base << 16) leaves 32 bits from
    # |y + mi + mq| >= 1537 on at white 16383, ire_base 8191.  No single colour gets there (solid yellow: 1360); a saturated colour
    # followed by white does -- the luma low-pass is at white within a few samples while the slower I / Q ones still hold the colour
    # (test_encoder_cpu.py proves it on the oracle).  Runs of the largest-I, largest-Q colours, yellow and red against white.
    for name in ("ntsc", "ntscp0", "vhslcg", "pv1k"):
        dwn = destw(name)
        _case(name + "-overshoot-white16383-ire8191", name,
              lambda k, dwn=dwn: runs_image(dwn, 48, 0, k & 1, (OVERSHOOT[k], COLOURS["W"])), noise=KNOB_NOISE, family="knob",
              knobs=dict(white_point=white_point_for(name, 16383), **ire_knobs(name, 8191)), target=(16383, 8191))
    # geometry: fields 0, 1 random, fields 2, 3 runs of opposite corners, at the widths where the code takes another path
    dw = destw("ntsc")

    def geo(w, h):
        def images(k):
            return R.synth_image(w, h, 3, 8500 + k) if k < 2 else runs_image(w, h, k, k)
        return images
    for w in (dw - 1, dw + 1, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 1279, 1280, 1281, 4099):
        _case("ntsc-w%d" % w, "ntsc", geo(w, 8), noise=KNOB_NOISE, family="geometry")
    for w in (3, 16, 1279, 1280):
        _case("ntsc-w%d-rgb" % w, "ntsc", geo(w, 8), fmt=R.FMT_RGB, noise=KNOB_NOISE, family="geometry")
    _case("ntsc-w1280-noise32767", "ntsc", geo(1280, 8), noise=32767, family="geometry")
    _case("ntsc-raw-w200-xoffset8", "ntsc", geo(200, 24), noise=KNOB_NOISE, raw=1, xoffset=8, family="geometry")
    _case("ntsc-raw-w33-xoffset-12-argb", "ntsc", geo(33, 24), fmt=R.FMT_ARGB, noise=KNOB_NOISE, raw=1, xoffset=-12, family="geometry")
    _case("pv1k-raw-w200-xoffset10", "pv1k", geo(200, 24), noise=KNOB_NOISE, raw=1, xoffset=10, family="geometry")
    # per-field noise in one batch (fieldpass_knobs: the KN kernels), against the oracle's loop over batches of one
    per_field = [0, 1, 32767, -32767]
    _case("ntsc-kn-mixed", "ntsc", _mixed("ntsc"), noise=per_field, family="kn")
    _case("ntsc-kn-mixed-rgb", "ntsc", _mixed("ntsc"), fmt=R.FMT_RGB, noise=per_field, family="kn")
    _case("ntsc-kn-w1280", "ntsc", geo(1280, 8), noise=per_field, family="kn")
    _case("ntsc-kn-white8191", "ntsc", _mixed("ntsc"), noise=per_field, knobs=dict(white_point=white_point_for("ntsc", 8191)), family="kn",
          target=(8191, None))
    _case("snes-kn-mixed", "snes", _mixed("snes"), noise=per_field, family="kn")
    # (no PV-1000 row: fieldpass_knobs refuses the 5-sample system, whose decoder takes its knobs from the uniform parameters)
    _case("nes-kn-ramp", "nes", _nes_images(256, 16, "ramp"), n=3, noise=per_field[1:], family="kn")
    _case("nes-kn-w7", "nes", _nes_images(7, 16, "ppu"), n=3, noise=per_field[1:], family="kn")


_build_table()


def intended(case, noise):
    """-> (white, ire_base, fast): the values the case's knobs are meant to give, and the side of encoder_fast_ok the case is meant
    for at this noise -- from the table's own targets, never from its name"""
    sd = oracle(case["name"]).sys
    white, ire = case["target"] or (None, None)
    white = sd.white_level if white is None else white
    ire = sd.black_level if ire is None else ire
    fast = case["name"] != "ntschipass" and abs(white) < FAST_WHITE and abs(ire) < FAST_IRE and abs(noise) < FAST_NOISE
    return white, ire, fast


def noises(case):
    nz = case["noise"]
    return list(nz) if isinstance(nz, (list, tuple)) else [nz] * case["n"]


def is_noise_edge(case):
    """|noise| >= 32767: the reference's sync search may run past inp[] + 16; the picture comparison is extra there"""
    return max(abs(v) for v in noises(case)) >= 32767


_IMAGES = {}


def images(cid):
    """the n images of a case in its pixel format, [n, h, w, bpp] uint8 (NES: [n, h, w] uint16); built once"""
    if cid not in _IMAGES:
        case = CASES[cid]
        if is_nes(case["name"]):
            _IMAGES[cid] = np.stack([case["images"](k) for k in range(case["n"])]).astype(np.uint16)
        else:
            _IMAGES[cid] = np.stack([lay(case["images"](k), case["fmt"]) for k in range(case["n"])])
    return _IMAGES[cid]


def field_of(k, step):
    return (k & 1) ^ (step & 1)


def frame_of(k):
    return (k >> 1) & 1


def dco_of(name, k, step):
    return (2 * k + 1 + step) % 6 if name.startswith(("pv1k", "temp")) else (k + step) % 3


def settings_kw(case, k, step):
    """NTSC_SETTINGS members of field k in pass `step` (without data, w, h), as the reference names them"""
    name = case["name"]
    orc = oracle(name)
    if is_nes(name):
        return dict(hue=case["hue"], dot_crawl_offset=dco_of(name, k, step))
    if is_progressive(name):
        return dict(format=case["fmt"], hue=case["hue"], dot_crawl_offset=dco_of(name, k, step), xoffset=case["xoffset"])
    kw = dict(format=case["fmt"], as_color=1, raw=case["raw"], field=field_of(k, step), frame=frame_of(k), hue=case["hue"],
              xoffset=case["xoffset"])
    if orc.system in R.DOT_CRAWL_SYSTEMS:
        kw["dot_crawl_offset"] = dco_of(name, k, step)
    if orc.system == R.SYS_VHS:
        kw["do_aberration"] = 0
    return kw


STEPS = 2


def run_checker(lib, cid):
    """the case on `lib` (the Oracle, or the real reference: RefLib), field by field from lock (hsync = vsync = 0), every pass from a
    clean analog[] (the batch semantics of the GPU entry points).  -> [field][pass] dict.  On the oracle, `undefined` says from which
    pass on the reference's reads leave inp[] + 16 (crtref.reads_past_inp)."""
    case = CASES[cid]
    name, imgs, nz = case["name"], images(cid), noises(case)
    is_orc = isinstance(lib, R.Oracle)
    res = []
    for k in range(case["n"]):
        c = lib.new_crt(OUTW, OUTH, OUTFMT)
        for kk, v in case["knobs"].items():
            c.set(kk, v)
        c.set("hsync", 0)
        c.set("vsync", 0)
        pad = np.concatenate([imgs[k], imgs[k][-1:]])
        if name in RAND_BUILDS:
            if is_orc:
                C.CDLL(None).srand(C.c_uint(SEEDS[k]))
            else:
                lib.srand(SEEDS[k])
        per, undefined = [], False
        for step in range(STEPS):
            c.settings(pad, w=int(imgs.shape[2]), h=int(imgs.shape[1]), **settings_kw(case, k, step))
            if is_progressive(name):
                c.sset("field_initialized", 0)
            c.analog[:] = 0
            c.modulate()
            analog, ccf_mod = np.array(c.analog).copy(), np.array(c.ccf).copy()
            hs_before = c.get("hsync")
            if is_orc:
                c.demodulate(nz[k], trace=True)
                undefined = undefined or R.reads_past_inp(lib, c.trace, c.get("vsync"), hs_before)
            else:
                c.demodulate(nz[k])
            per.append(dict(analog=analog, ccf_mod=ccf_mod, inp=np.array(c.inp).copy(), rn=c.get("rn"), hsync=c.get("hsync"),
                            vsync=c.get("vsync"), ccf=np.array(c.ccf).copy(), out=c.out.copy(), undefined=undefined))
        res.append(per)
    return res


_WANT = {}


def expected(cid):
    """the oracle's results of a case; computed once and left alone"""
    if cid not in _WANT:
        _WANT[cid] = run_checker(oracle(CASES[cid]["name"]), cid)
    return _WANT[cid]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases on which tests/test_gpu_encoder.py pins every instantiation (test_encoder_instantiations)
# ---------------------------------------------------------------------------------------------------------------------------
PINNED = ["ntsc-runs0", "ntsc-solid-b", "ntsc-phase", "ntsc-white8191", "ntsc-white8192", "ntsc-ire-8191", "ntsc-ire-8192", "ntsc-noise32767",
          "ntsc-noise-32768", "ntsc-corner+1+1+1", "ntsc-corner-1-1-1", "ntsc-overshoot-white16383-ire8191", "ntsc-w1280", "ntsc-w1279",
          "ntsc-w1280-noise32767", "ntsc-w1280-rgb", "ntsc-w1279-rgb", "ntsc-mixed-rgb", "ntsc-mixed-argb", "ntsc-white8191-rgb",
          "ntsc-floors", "ntsc-kn-mixed", "ntsc-kn-w1280", "ntsc-kn-mixed-rgb", "ntsc-kn-white8191", "snes-phase", "snes-floors",
          "snes-kn-mixed", "pv1k-phase", "pv1k-white8191", "vhslcg-runs0", "vhslcg-noise32767", "ntscbloom-phase", "nesrgb-phase",
          "ntschipass-phase", "nes-ramp-w256", "nes-ramp-w7", "nes-ppu-w4", "nes-ppu-w8", "nes-minus128-w8", "nes-minus128-w7",
          "nes-minus128-w8-noise0", "nes-minus128-w7-noise0", "nes-minus128-ramp-noise0", "nes-kn-ramp", "nes-kn-w7"]

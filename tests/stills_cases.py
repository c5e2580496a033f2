"""Cases and expected values of the stills mode (crthip_stills / CRT.stills, include/crt_hip.h); no tests in here.

A case is a batch of n different images that all take the same schedule of field-passes onto their own picture: the accumulate loop
of the reference's `ntsc` program (crt_main.c:241-255) or a schedule of the case's own.  Expected pictures and states never come from
the library: the oracle (or the compiled reference) runs the serial loop ONCE PER IMAGE -- per schedule entry: display step (phosphor
cases), crt_modulate, crt_demodulate -- onto one buffer from a crt_init state (zeros, rn 194).  The shapes are the smallest that
still reach every branch: tiny inputs, outputs with row collisions (96x72), one row per line (160x240) and duplicated rows (640x480
without scanlines), and one 1920x1080 picture for the wide-run decoder."""
import ctypes as C

import numpy as np

import crtref as R
from test_phosphor_cpu import display_step_np

CLI_BLEND = dict(scanlines=1, blend=1)               # crt_main.c:235-236


def cli_schedule(interlaced, first_field, n_frames):
    """a literal transcription of crt_main.c:241-255: the (field, frame) every crt_modulate of the loop sees"""
    out = []
    field, frame = first_field & 1, 0                # ntsc.field = field & 1; ntsc.frame = 0
    err = 0
    while err < n_frames:                            # while (err < 4)
        out.append((field, frame, 0))                # crt_modulate; crt_demodulate
        if interlaced:                               # if (!progressive)
            field ^= 1                               # ntsc.field ^= 1
            out.append((field, frame, 0))            # crt_modulate; crt_demodulate
            if (err & 1) == 0:                       # a frame is two fields
                frame ^= 1
        err += 1
    return out


def _case(id, name, inp, outw, outh, ofmt, knobs, noise, n, sched, mode="keep", shapes=(0,)):
    return dict(id=id, name=name, inp=inp, outw=outw, outh=outh, ofmt=ofmt, knobs=knobs, noise=noise, n=n, sched=sched, mode=mode,
                shapes=shapes)


INTERLACED0, INTERLACED1, PROGRESSIVE = cli_schedule(1, 0, 4), cli_schedule(1, 1, 4), cli_schedule(0, 0, 4)
# five passes of the case's own, field / frame beyond 0 / 1 (masked with 1, crt_ntsc.c:197-198): (0,0) (1,0) (1,0) (0,1) (0,0), 3 distinct entries
CUSTOM5 = [(0, 0, 0), (3, 0, 0), (1, 2, 0), (0, 1, 0), (2, 2, 0)]
NES_DOTS = [(0, 0, r % 3) for r in range(5)]         # dot_crawl_offset 0, 1, 2, 0, 1
PV1K_DOTS = [(0, 0, r % 5) for r in range(7)]          # aux cycling through CRT_CC_VPER = 5
# aux = an aberration height (crt_ntscvhs.c:205-207 draws 6 .. 17), 0 = none.  The band's lines carry no sync pulse, hsync runs away
# on them, and a band that reaches the field's last decoded line makes the reference read far behind inp[] (undefined).  v_fac = 8
# leaves the last 7 lines undecoded (beg >= outh, crt_core.c:431): the band is seen (hsync ends beyond 60) and every read is defined.
VHS_BAND = [(0, 0, 0), (1, 0, 12), (1, 1, 0), (0, 1, 17), (0, 1, 17), (1, 1, 0), (1, 0, 12), (0, 0, 0)]
VHS_BAND_KNOBS = dict(scanlines=1, blend=1, v_fac=8)

CASES = [
    # the CLI's own configuration: noise 0 (every distinct entry encoded once), interlaced from field 0, every kernel shape (the
    # forced shapes keep the padded signal lines)
    _case("ntsc-cli-noise0", "ntsc", (64, 48), 160, 240, R.FMT_BGRA, CLI_BLEND, 0, 4, INTERLACED0, shapes=(0, 1, 2)),
    _case("ntsc-cli-field1-noise24", "ntsc", (40, 30), 96, 72, R.FMT_BGRA, CLI_BLEND, 24, 3, INTERLACED1, shapes=(0, 1)),
    _case("ntsc-progressive-rgb-duprows", "ntsc", (80, 60), 640, 480, R.FMT_RGB, dict(scanlines=0, blend=1), 0, 3, PROGRESSIVE, shapes=(0, 2)),
    _case("ntsc-custom5-noise120-noblend", "ntsc", (72, 54), 96, 72, R.FMT_BGRA, dict(scanlines=1, blend=0), 120, 5, CUSTOM5),
    _case("ntsc-custom5-noise0-noblend", "ntsc", (72, 54), 160, 240, R.FMT_ARGB, dict(scanlines=1, blend=0), 0, 5, CUSTOM5, shapes=(0, 2)),
    _case("ntsc-fade-noise0", "ntsc", (64, 48), 160, 240, R.FMT_BGRA, CLI_BLEND, 0, 3, INTERLACED0, mode="fade"),
    _case("ntscbloom-noise0", "ntscbloom", (64, 48), 160, 240, R.FMT_BGRA, CLI_BLEND, 0, 3, INTERLACED0, shapes=(0, 1)),
    _case("ntscbloom-noise24", "ntscbloom", (64, 48), 160, 240, R.FMT_BGRA, CLI_BLEND, 24, 3, PROGRESSIVE),
    _case("nes-dots-noise0", "nes", (256, 240), 160, 240, R.FMT_BGRA, CLI_BLEND, 0, 3, NES_DOTS),
    _case("nes-dots-noise24", "nes", (256, 240), 96, 72, R.FMT_BGRA, CLI_BLEND, 24, 3, NES_DOTS),
    _case("pv1k-dots-noise0", "pv1k", (64, 48), 160, 240, R.FMT_BGRA, CLI_BLEND, 0, 3, PV1K_DOTS, shapes=(0, 1)),
    _case("pv1k-dots-noise24", "pv1k", (64, 48), 160, 240, R.FMT_BGRA, dict(scanlines=1, blend=0), 24, 3, PV1K_DOTS),
    _case("vhs-rand-noise24", "vhs", (64, 48), 160, 240, R.FMT_BGRA, CLI_BLEND, 24, 3, INTERLACED0),
    _case("vhs-rand-noise0", "vhs", (64, 48), 160, 240, R.FMT_BGRA, CLI_BLEND, 0, 3, PROGRESSIVE),
    _case("vhslcg-band-noise0", "vhslcg", (64, 48), 160, 240, R.FMT_BGRA, VHS_BAND_KNOBS, 0, 3, VHS_BAND, shapes=(0, 1)),
    _case("vhslcg-band-noise24", "vhslcg", (64, 48), 160, 240, R.FMT_BGRA, VHS_BAND_KNOBS, 24, 3, VHS_BAND),
    # 1920x1080 in and out through the lane-per-scanline shape: the wide-run decoder (k_decode_wide)
    _case("wide-progressive2", "ntsc", (1920, 1080), 1920, 1080, R.FMT_BGRA, CLI_BLEND, 0, 1, cli_schedule(0, 0, 2), shapes=(1,)),
]
CASE_IDS = [c["id"] for c in CASES]
VHS_SEEDS = [7, 1001, 424242, 5, 99]                 # srand() of every still of the rand()-noise VHS cases


def case(id):
    return CASES[CASE_IDS.index(id)]


def sysid(case):
    return R.SYSTEMS[case["name"]][0]


def is_vhs_rand(case):
    return sysid(case) == R.SYS_VHS and case["name"] != "vhslcg"


def images(case, seed=900):
    """the n different images of the case: [n, h, w, 4] BGRA, or [n, h, w] PPU pixels for the NES"""
    w, h = case["inp"]
    if sysid(case) == R.SYS_NES:
        return np.stack([R.synth_ppu(w, h, seed + k) for k in range(case["n"])])
    return np.stack([R.synth_image(w, h, 4, seed + k, "bars" if k % 3 == 1 else "random") for k in range(case["n"])])


def distinct_entries(case):
    """the distinct (field & 1, frame & 1, aux) of the schedule, in order of first use"""
    out = []
    for f, fr, aux in case["sched"]:
        e = (f & 1, fr & 1, aux)
        if e not in out:
            out.append(e)
    return out


_BAND_SEED = {}


def _seed_for_band(height):
    """a srand() seed after which crt_modulate draws this aberration height (crt_ntscvhs.c:205-207: rand() % 12 - 8 + 14)"""
    if height not in _BAND_SEED:
        libc = C.CDLL(None)
        _BAND_SEED[height] = next(sd for sd in range(1, 5000) if (libc.srand(sd), ((libc.rand() % 12) - 8) + 14)[1] == height)
    return _BAND_SEED[height]


def _pass_settings(case, c, lib, img, entry):
    """NTSC_SETTINGS of one pass (the image is followed by a readable row: crt_ntsc.c:263)"""
    field, frame, aux = entry[0] & 1, entry[1] & 1, entry[2]
    pad = np.concatenate([img, img[-1:]], axis=0)
    w, h = case["inp"]
    sid = sysid(case)
    if sid == R.SYS_NES:
        c.settings(pad, w=w, h=h, dot_crawl_offset=aux, hue=0)
    elif sid == R.SYS_NESRGB:
        c.settings(pad, format=R.FMT_BGRA, w=w, h=h, dot_crawl_offset=aux, hue=0)
    else:
        c.settings(pad, format=R.FMT_BGRA, w=w, h=h, as_color=1, field=field, frame=frame)
        if sid in R.DOT_CRAWL_SYSTEMS:
            c.sset("dot_crawl_offset", aux)
        if sid == R.SYS_VHS:
            c.sset("do_aberration", 1 if aux else 0)
            if aux:
                lib.srand(_seed_for_band(aux))       # (LCG-noise build: crt_modulate's draw is the only use of rand())


def still_loop(lib, case, img, k, check_reads=False):
    """the serial loop on ONE image: (out, hsync, vsync, rn, ccf) after the last pass"""
    c = lib.new_crt(case["outw"], case["outh"], case["ofmt"])
    for a, v in case["knobs"].items():
        c.set(a, v)
    if is_vhs_rand(case):
        lib.srand(VHS_SEEDS[k])
    for r, entry in enumerate(case["sched"]):
        if case["mode"] != "keep":
            c.out[:] = display_step_np(c.out, case["ofmt"], case["mode"])
        _pass_settings(case, c, lib, img, entry)
        c.modulate()
        hs_before = c.get("hsync")
        if check_reads:
            c.demodulate(case["noise"], trace=True)
            assert not R.reads_past_inp(lib, c.trace, c.get("vsync"), hs_before), \
                "%s still %d pass %d: the reference reads past inp[] here (undefined): pick another configuration" % (case["id"], k, r)
        else:
            c.demodulate(case["noise"])
    return c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn"), np.array(c.ccf, dtype=np.int32).copy()


_EXPECTED = {}


def expected(case, lib=None, check_reads=False):
    """[(out, hsync, vsync, rn, ccf)] per still.  The oracle's values are computed once per case and shared (leave them unchanged)."""
    if lib is None and not check_reads:
        if case["id"] not in _EXPECTED:
            _EXPECTED[case["id"]] = expected(case, lib=R.Oracle(case["name"]))
        return _EXPECTED[case["id"]]
    lib = lib or R.Oracle(case["name"])
    imgs = images(case)
    return [still_loop(lib, case, imgs[k], k, check_reads) for k in range(case["n"])]


def write_ppm(path, rgb):
    """P6 as ppm_write24 writes it"""
    h, w = rgb.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb[:, :, :3]).tobytes())


def cli_still(orc, bgra, outw, outh, noise, hue=0, interlaced=True, first_field=0, as_color=1, raw=0):
    """the oracle's still of one BGRA image exactly as crt_main.c sets it up (BGRA in and out, blend 1, scanlines 1): [outh, outw, 3] RGB"""
    h, w = bgra.shape[:2]
    c = orc.new_crt(outw, outh, R.FMT_BGRA)
    c.set("blend", 1)
    c.set("scanlines", 1)
    pad = np.concatenate([bgra, bgra[-1:]], axis=0)
    for field, frame, _ in cli_schedule(interlaced, first_field, 4):
        c.settings(pad, format=R.FMT_BGRA, w=w, h=h, as_color=as_color, raw=raw, hue=hue, field=field, frame=frame)
        c.modulate()
        c.demodulate(noise)
    return c.out.reshape(outh, outw, 4)[:, :, 2::-1].copy()

"""Cases and expected values of the many-sets sequence mode (crthip_sequence_sets / CRT.sequence_sets); no tests in here.

A case is a batch of n fields cut into sets by `set_first`.  Expected pictures and states never come from the library: the oracle
(or the compiled reference) runs the reference's serial loop -- display step, crt_modulate, crt_demodulate per field, the model is
tests/test_gpu_phosphor.py:_live_loop -- ONCE PER SET, each set from its own incoming (hsync, vsync, rn) and its own initial picture.
The incoming values differ from set to set so that a missing set boundary shows (tests/test_seqsets_cpu.py checks that it would)."""
import numpy as np

import crtref as R
from test_phosphor_cpu import display_step_np

RAGGED = [0, 1, 4, 9, 16, 17]                      # lengths 1, 3, 5, 7, 1
UNIFORM = list(range(0, 49, 6))                    # 8 sets of 6 fields
DEPTH = [0, 3, 48]                                 # a set of 45 fields (> CRTHIP_PHOSPHOR_DEPTH = 38) behind a short one
WIDE = [0, 2, 5]
# every set's state before its first field: far apart, so that the sets' sync chains start differently
HSYNC_IN = [7, -20, 40, 0, 13, -9, 25, 3]
VSYNC_IN = [2, 0, 5, 30, 0, 3, 2, 0]               # (30: a vertical hold that takes fields to lock -- more sync passes)
RN_IN = [194, 77001, 5, 123456789, 31337, 2024, 99, 4242]
# At 320x240 with v_fac 0 every line writes one row and the lines cover every row, so no row is ever carried over; v_fac = 240
# with scanlines 1 leaves a gap row under every line (tests/test_gpu_phosphor.py: SMALL)
SMALL = dict(scanlines=1, v_fac=240)


def _case(id, name, outw, outh, ofmt, knobs, mode, noise, set_first, shapes=(0,), init="per_set", progressive=False):
    return dict(id=id, name=name, outw=outw, outh=outh, ofmt=ofmt, knobs=knobs, mode=mode, noise=noise, set_first=set_first,
                shapes=shapes, init=init, progressive=progressive)


CASES = [
    _case("ntsc-keep-shapes", "ntsc", 640, 480, R.FMT_BGRA, dict(scanlines=1), "keep", 24, RAGGED, shapes=(0, 1, 2)),
    _case("ntsc-blend-keep", "ntsc", 640, 480, R.FMT_BGRA, dict(scanlines=1, blend=1), "keep", 24, RAGGED),
    _case("ntsc-rgb-fade-shared", "ntsc", 832, 624, R.FMT_RGB, dict(scanlines=0), "fade", 12, RAGGED, init="shared"),
    _case("ntsc-rgb-blend-duprows", "ntsc", 832, 624, R.FMT_RGB, dict(scanlines=0, blend=1), "keep", 12, RAGGED, shapes=(0, 2)),
    _case("ntsc-rgb-blend-fade-zeros", "ntsc", 832, 624, R.FMT_RGB, dict(scanlines=0, blend=1), "fade", 12, RAGGED, init="none"),
    _case("ntsc-small-argb-fade-noise120", "ntsc", 320, 240, R.FMT_ARGB, SMALL, "fade", 120, RAGGED),
    _case("ntsc-small-argb-blend-clear", "ntsc", 320, 240, R.FMT_ARGB, dict(SMALL, blend=1), "clear", 24, RAGGED, init="shared"),
    _case("nes-clear", "nes", 640, 480, R.FMT_BGRA, dict(scanlines=1), "clear", 12, RAGGED),
    _case("pv1k-blend-zeros", "pv1k", 640, 480, R.FMT_BGRA, dict(scanlines=0, blend=1), "keep", 30, RAGGED, init="none"),
    _case("ntscbloom-fade", "ntscbloom", 640, 480, R.FMT_BGRA, dict(scanlines=1), "fade", 24, RAGGED, shapes=(0, 1)),
    _case("vhslcg-keep", "vhslcg", 640, 480, R.FMT_BGRA, dict(scanlines=1), "keep", 24, RAGGED, init="shared"),
    _case("vhslcg-blend-fade", "vhslcg", 640, 480, R.FMT_BGRA, dict(scanlines=1, blend=1), "fade", 24, RAGGED),
    _case("uniform-blend-fade", "ntsc", 640, 480, R.FMT_BGRA, dict(scanlines=1, blend=1), "fade", 24, UNIFORM),
    _case("uniform-clear", "ntsc", 640, 480, R.FMT_BGRA, dict(scanlines=1), "clear", 24, UNIFORM, init="none"),
    _case("depth-fade", "ntsc", 320, 240, R.FMT_BGRA, SMALL, "fade", 24, DEPTH, progressive=True),
    _case("depth-blend-fade", "ntsc", 320, 240, R.FMT_BGRA, dict(SMALL, blend=1), "fade", 24, DEPTH, progressive=True),
    # 1920x1080 through the lane-per-scanline shape: the wide-run decoder (k_decode_wide)
    _case("wide-keep", "ntsc", 1920, 1080, R.FMT_BGRA, dict(scanlines=1), "keep", 24, WIDE, shapes=(1,)),
    # taller than the fold kernel's LDS strips hold (2048 rows): the fold by field index, one launch per field of the longest set
    _case("tall-blend-fade", "ntsc", 96, 2112, R.FMT_BGRA, dict(scanlines=0, blend=1), "fade", 24, WIDE),
    _case("wide-blend-fade", "ntsc", 1920, 1080, R.FMT_BGRA, dict(scanlines=1, blend=1), "fade", 24, WIDE, shapes=(1,), init="shared"),
]
CASE_IDS = [c["id"] for c in CASES]
NOISY = "ntsc-small-argb-fade-noise120"            # the case whose sets need different numbers of sync passes
DUPROWS = "ntsc-rgb-blend-duprows"                 # blend with duplicated rows: the fold's cross-row dependency


def case(id):
    return CASES[CASE_IDS.index(id)]


def n_fields(case):
    return case["set_first"][-1]


def sets_of(case):
    sf = case["set_first"]
    return [(sf[s], sf[s + 1]) for s in range(len(sf) - 1)]


def field_parity(j):
    """extra/video_convert.c:261-267 for field j of a set (ntsc-crt_amd/shard.py:field_parity)"""
    return j & 1, ((j + 1) >> 1) & 1


def parities(case):
    """(field, frame) of every field of the batch: every set is a video of its own and starts at its field 0"""
    out = []
    for lo, hi in sets_of(case):
        out += [(0, 0) if case["progressive"] else field_parity(k - lo) for k in range(lo, hi)]
    return out


def dot_crawl(case):
    out = []
    for lo, hi in sets_of(case):
        out += [(k - lo) % 3 for k in range(lo, hi)]
    return out


def frames(case, seed=300):
    n = n_fields(case)
    sysid = R.SYSTEMS[case["name"]][0]
    if sysid == R.SYS_NES:
        return np.stack([R.synth_ppu(256, 240, seed + k) for k in range(n)])
    iw, ih = (256, 240) if sysid == R.SYS_NESRGB else (640, 480)
    return np.stack([R.synth_image(iw, ih, 4, seed + k, "random" if k % 3 else "bars") for k in range(n)])


def incoming(case):
    """[(hsync, vsync, rn)] of every set before its first field"""
    return [(HSYNC_IN[s % 8], VSYNC_IN[s % 8], RN_IN[s % 8]) for s in range(len(case["set_first"]) - 1)]


def init_pictures(case):
    """None, one picture [outh, outw, bpp] or one per set [n_sets, outh, outw, bpp] (different seeds)"""
    bpp = R.bpp4fmt(case["ofmt"])
    shape = (case["outh"], case["outw"], bpp)
    size = shape[0] * shape[1] * shape[2]
    if case["init"] == "none":
        return None
    if case["init"] == "shared":
        return R.lcg_bytes(size, 5).reshape(shape)
    return np.stack([R.lcg_bytes(size, 5 + 11 * s).reshape(shape) for s in range(len(case["set_first"]) - 1)])


def init_of_set(case, init, s):
    if init is None:
        return np.zeros((case["outh"], case["outw"], R.bpp4fmt(case["ofmt"])), dtype=np.uint8)
    return init if init.ndim == 3 else init[s]


def field_settings(case, frame, parity, dco):
    """keyword settings of one field for the oracle / reference"""
    sysid = R.SYSTEMS[case["name"]][0]
    pad = np.concatenate([frame, frame[-1:]], axis=0)
    if sysid == R.SYS_NES:
        return pad, dict(w=256, h=240, dot_crawl_offset=dco, hue=0), None
    h, w = frame.shape[0], frame.shape[1]
    if sysid == R.SYS_NESRGB:
        return pad, dict(format=R.FMT_BGRA, w=w, h=h, dot_crawl_offset=dco, hue=0), None
    kw = dict(format=R.FMT_BGRA, w=w, h=h, as_color=1, field=parity[0], frame=parity[1])
    return pad, kw, (dco if sysid in R.DOT_CRAWL_SYSTEMS else None)


def live_loop(lib, case, fr, par, dco, lo, hi, init, state_in, check_reads=False):
    """the reference's loop on ONE set = fields [lo, hi) of the batch: per field  display step (fade / clear / keep);  crt_modulate;
    crt_demodulate.  lib: R.Oracle(name) or R.RefLib(name).  Returns [(out, hsync, vsync, rn)] after every field."""
    c = lib.new_crt(case["outw"], case["outh"], case["ofmt"])
    for k, v in case["knobs"].items():
        c.set(k, v)
    c.out[:] = init.reshape(-1)
    c.set("hsync", state_in[0])
    c.set("vsync", state_in[1])
    c.set("rn", state_in[2])
    want = []
    for k in range(lo, hi):
        if case["mode"] != "keep":
            c.out[:] = display_step_np(c.out, case["ofmt"], case["mode"])
        pad, kw, d = field_settings(case, fr[k], par[k], dco[k])
        c.settings(pad, **kw)
        if d is not None:
            c.sset("dot_crawl_offset", d)
        c.modulate()
        hs_before = c.get("hsync")
        if check_reads:
            c.demodulate(case["noise"], trace=True)
            assert not R.reads_past_inp(lib, c.trace, c.get("vsync"), hs_before), \
                "%s field %d: the reference reads past inp[] here (undefined): pick another noise / hsync" % (case["id"], k)
        else:
            c.demodulate(case["noise"])
        want.append((c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn")))
    return want


def expected(case, lib=None, check_reads=False):
    """per-set loops of the oracle (or `lib`) -> [(out, hsync, vsync, rn)] for every field of the batch, in batch order"""
    lib = lib or R.Oracle(case["name"])
    fr, par, dco, init, inc = frames(case), parities(case), dot_crawl(case), init_pictures(case), incoming(case)
    want = []
    for s, (lo, hi) in enumerate(sets_of(case)):
        want += live_loop(lib, case, fr, par, dco, lo, hi, init_of_set(case, init, s), inc[s], check_reads)
    return want


def expected_one_long_set(case):
    """the same fields as ONE set from set 0's incoming state and picture: what a library without set boundaries would compute"""
    fr, par, dco, init, inc = frames(case), parities(case), dot_crawl(case), init_pictures(case), incoming(case)
    return live_loop(R.Oracle(case["name"]), case, fr, par, dco, 0, n_fields(case), init_of_set(case, init, 0), inc[0])


def sync_passes_of_set(case, s, want):
    """passes the sync fixed point (DESIGN.md "Sequence mode") needs for set s alone, from the oracle: every pass runs every field's
    sync search from the previous pass's final pair of its predecessor (the set's incoming pair for the first field); it stops
    after the first pass that changes nothing.  want: expected(case) (rn before a field = rn after its predecessor)."""
    lo, hi = sets_of(case)[s]
    fr, par, dco, inc = frames(case), parities(case), dot_crawl(case), incoming(case)[s]
    orc = R.Oracle(case["name"])
    crts = []
    for k in range(lo, hi):
        c = orc.new_crt(case["outw"], case["outh"], case["ofmt"])
        for a, v in case["knobs"].items():
            c.set(a, v)
        pad, kw, d = field_settings(case, fr[k], par[k], dco[k])
        c.settings(pad, **kw)
        if d is not None:
            c.sset("dot_crawl_offset", d)
        crts.append(c)

    def final(k, pair):
        c = crts[k - lo]
        c.modulate()                                   # (the ccf preset of crt_modulate; the field itself is the same every time)
        c.set("hsync", pair[0])
        c.set("vsync", pair[1])
        c.set("rn", inc[2] if k == lo else want[k - 1][3])
        c.demodulate(case["noise"])
        return c.get("hsync"), c.get("vsync")
    guess = [(inc[0], inc[1])] * (hi - lo)
    passes = 0
    while True:
        passes += 1
        fin = [final(k, (inc[0], inc[1]) if k == lo else guess[k - lo - 1]) for k in range(lo, hi)]
        if fin == guess:
            return passes
        guess = fin
        assert passes <= hi - lo + 1

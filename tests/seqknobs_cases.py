"""Cases and expected values of sequence mode with per-field knobs (crthip_sequence_knobs / crthip_sequence_sets_knobs /
crthip_seq_bind_knobs; CRT.sequence_knobs and friends); no tests in here.

A case is a batch of n fields cut into sets by `set_first`, every field with its own (noise, monitor hue, saturation).  Expected
pictures and states never come from the library: the oracle (or the compiled reference) runs the reference's serial loop ONCE PER SET
on ONE CRT -- per field: display step; crt.hue / crt.saturation <- the field's knobs (crt_main.c:351-391); crt_modulate;
crt_demodulate(the field's noise) -- each set from its own incoming (hsync, vsync, rn) and its own initial picture.  Geometry, images
and the tier-mixing triples are those of tests/knobs_cases.py."""
import ctypes as C

import numpy as np

import crtref as R
import knobs_cases as KC
from seqsets_cases import HSYNC_IN, RN_IN, VSYNC_IN, field_parity
from test_phosphor_cpu import display_step_np

SMALL = KC.SMALL
# blend needs one line per output row, outh + v_fac >= CRT_LINES (262): the smallest picture the rule accepts at v_fac 0
BLEND = dict(SMALL, outh=262)
NES_GEO = dict(w=256, h=240, outw=320, outh=240)

# six fields on one set: KC.SMALL_TRIPLES' saturations (either side of tier 0's chroma bound, the exact tier) and hues (tier flags
# flip inside one wavefront), the clean field in the middle, and noise large enough to knock the sync state about from field to field
# (the fixed point then needs more than two passes: tests/test_seqknobs_cpu.py derives the count from the oracle)
SIX = [(24, 0, 10), (200, 17, 14), (0, -20, 900), (24, 350, 40), (230, 77, 13), (60, 725, -70)]


def _case(id, name, triples, geo=SMALL, knobs=None, mode="keep", set_first=None, init="none", incoming=None, seed=None,
          aberration=0):
    n = len(triples)
    return dict(id=id, name=name, triples=[tuple(int(v) for v in t) for t in triples], geo=geo, knobs=dict(knobs or {}), mode=mode,
                set_first=set_first or [0, n], init=init, incoming=incoming, seed=seed, aberration=aberration)


def _drawn(n, seed, **kw):
    return KC.drawn_triples(n, seed, **kw)


SETS_FIRST = [0, 1, 5, 7]                              # three sets of lengths 1, 4 and 2
SETS_TRIPLES = SIX + [(45, -100, 25)]

CASES = [
    _case("six", "ntsc", SIX),
    _case("six-blend", "ntsc", SIX, geo=BLEND, knobs=dict(blend=1), init="per_set"),
    _case("six-fade", "ntsc", SIX, mode="fade", init="per_set"),
    _case("six-clear", "ntsc", SIX, mode="clear", init="per_set"),
    _case("six-blend-fade", "ntsc", SIX, geo=BLEND, knobs=dict(blend=1), mode="fade", init="per_set"),
    _case("six-blend-clear", "ntsc", SIX, geo=BLEND, knobs=dict(blend=1), mode="clear", init="per_set"),
    _case("seventy", "ntsc", _drawn(70, 20261018)),
    _case("bloom", "ntscbloom", _drawn(6, 506, noise_max=40, sat_lo=-15, sat_hi=30)),
    _case("fir7", "ntscfir7", _drawn(4, 504, noise_max=40, sat_lo=-15, sat_hi=30)),
    _case("nes", "nes", _drawn(6, 516, noise_max=40, sat_lo=-15, sat_hi=30), geo=NES_GEO),
    _case("vhs", "vhs", _drawn(5, 505, noise_max=40, sat_lo=-15, sat_hi=30), seed=20260924),
    # the aberration band takes the sync pulses of the field's last lines away, and the reference's video window of one of them then
    # runs past inp[] (undefined there).  v_fac = 8 spreads the 240 lines over 128 rows of which the picture holds 120: the lines
    # behind row 119 are skipped (crt_core.c:431) before they read anything, the band's among them
    _case("vhs-aberration", "vhs", _drawn(5, 515, noise_max=40, sat_lo=-15, sat_hi=30), knobs=dict(v_fac=8), seed=20260925, aberration=1),
    _case("vhslcg-sets", "vhslcg", SETS_TRIPLES, set_first=SETS_FIRST, init="per_set", incoming="per_set"),
    _case("sets", "ntsc", SETS_TRIPLES, set_first=SETS_FIRST, init="per_set", incoming="per_set"),
    _case("sets-blend-fade", "ntsc", SETS_TRIPLES, geo=BLEND, knobs=dict(blend=1), mode="fade", set_first=SETS_FIRST, init="per_set",
          incoming="per_set"),
]
CASE_IDS = [c["id"] for c in CASES]


def case(id):
    return CASES[CASE_IDS.index(id)]


def n_fields(case):
    return case["set_first"][-1]


def sets_of(case):
    sf = case["set_first"]
    return [(sf[s], sf[s + 1]) for s in range(len(sf) - 1)]


def is_nes(case):
    return R.SYSTEMS[case["name"]][0] == R.SYS_NES


def parities(case):
    """(field, frame) of every field of the batch: every set is a video of its own and starts at its field 0"""
    out = []
    for lo, hi in sets_of(case):
        out += [field_parity(k - lo) for k in range(lo, hi)]
    return out


def dot_crawl(case):
    out = []
    for lo, hi in sets_of(case):
        out += [(k - lo) % 3 for k in range(lo, hi)]
    return out


def frame(case, k):
    return KC.ppu_image(k, 5) if is_nes(case) else KC.image(case["geo"], k, 5)


def incoming(case):
    """[(hsync, vsync, rn)] of every set before its first field (crt_init's values unless the case says per_set)"""
    n_sets = len(case["set_first"]) - 1
    if case["incoming"] is None:
        return [(0, 0, 194)] * n_sets
    return [(HSYNC_IN[s % 8], VSYNC_IN[s % 8], RN_IN[s % 8]) for s in range(n_sets)]


def init_pictures(case):
    """None, or one picture [outh, outw, 4] per set (different seeds)"""
    if case["init"] == "none":
        return None
    shape = (case["geo"]["outh"], case["geo"]["outw"], 4)
    return np.stack([R.lcg_bytes(shape[0] * shape[1] * 4, 5 + 11 * s).reshape(shape) for s in range(len(case["set_first"]) - 1)])


def _init_of_set(case, init, s):
    return np.zeros((case["geo"]["outh"], case["geo"]["outw"], 4), dtype=np.uint8) if init is None else init[s]


def _new_crt(lib, case):
    c = lib.new_crt(case["geo"]["outw"], case["geo"]["outh"], R.FMT_BGRA)
    c.set("scanlines", 1)
    for a, v in case["knobs"].items():
        c.set(a, v)
    return c


def _settings(c, case, k, parity, dco):
    img = frame(case, k)
    pad = np.concatenate([img, img[-1:]], axis=0)
    if is_nes(case):
        c.settings(pad, w=256, h=240, dot_crawl_offset=dco, hue=0)
    else:
        c.settings(pad, format=R.FMT_BGRA, w=case["geo"]["w"], h=case["geo"]["h"], as_color=1, field=parity[0], frame=parity[1])
        if case["aberration"]:
            c.sset("do_aberration", 1)


def serial_loop(lib, case, lo, hi, init, state_in):
    """the reference's loop on ONE set = fields [lo, hi) of the batch, the knobs turned between the fields.  lib: R.Oracle(name) or
    R.RefLib(name).  Returns one dict per field: out, hsync, vsync, rn, ccf after it, and (oracle only) `undefined`: the field falls
    into the reference's undefined over-read (crtref.reads_past_inp)."""
    par, dco = parities(case), dot_crawl(case)
    c = _new_crt(lib, case)
    c.out[:] = init.reshape(-1)
    c.set("hsync", state_in[0])
    c.set("vsync", state_in[1])
    c.set("rn", state_in[2])
    if case["seed"] is not None:
        C.CDLL(None).srand(C.c_uint(case["seed"]))
    want = []
    for k in range(lo, hi):
        noise, hue, sat = case["triples"][k]
        if case["mode"] != "keep":
            c.out[:] = display_step_np(c.out, R.FMT_BGRA, case["mode"])
        c.set("hue", hue)
        c.set("saturation", sat)
        _settings(c, case, k, par[k], dco[k])
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


def expected(case, lib=None):
    """per-set loops of the oracle (or `lib`) -> one dict per field of the batch, in batch order.  The oracle's result is computed
    once per case and shared: treat it as read-only."""
    if lib is None and case["id"] in _EXPECTED:
        return _EXPECTED[case["id"]]
    use = lib or R.Oracle(case["name"])
    init, inc = init_pictures(case), incoming(case)
    want = []
    for s, (lo, hi) in enumerate(sets_of(case)):
        want += serial_loop(use, case, lo, hi, _init_of_set(case, init, s), inc[s])
    if lib is None:
        _EXPECTED[case["id"]] = want
    return want


def sync_passes(case, want):
    """passes the joint sync fixed point (DESIGN.md "Sequence mode") needs, from the oracle: every pass runs every field's sync search
    with ITS knobs from the previous pass's final pair of its predecessor (the set's incoming pair for a set's first field); it stops
    after the first pass that changes nothing.  Not for the rand()-noise VHS build (its noise is not a function of rn alone)."""
    assert case["seed"] is None
    orc = R.Oracle(case["name"])
    par, dco, inc = parities(case), dot_crawl(case), incoming(case)
    n = n_fields(case)
    first_of = {}
    for s, (lo, hi) in enumerate(sets_of(case)):
        for k in range(lo, hi):
            first_of[k] = (lo, s)
    crts = []
    for k in range(n):
        c = _new_crt(orc, case)
        c.set("hue", case["triples"][k][1])
        c.set("saturation", case["triples"][k][2])
        _settings(c, case, k, par[k], dco[k])
        crts.append(c)

    def final(k, pair):
        lo, s = first_of[k]
        c = crts[k]
        c.modulate()
        c.set("hsync", pair[0])
        c.set("vsync", pair[1])
        c.set("rn", inc[s][2] if k == lo else want[k - 1]["rn"])
        c.demodulate(case["triples"][k][0])
        return c.get("hsync"), c.get("vsync")
    guess = [inc[first_of[k][1]][:2] for k in range(n)]
    passes = 0
    while True:
        passes += 1
        fin = [final(k, inc[first_of[k][1]][:2] if k == first_of[k][0] else guess[k - 1]) for k in range(n)]
        if fin == guess:
            return passes
        guess = fin
        assert passes <= n + 1

"""Cases and expected values of the many-sets sequence mode on the stock VHS build (crthip_sequence_sets / _sets_knobs with
CRTHIP_F_VHS_SET_STREAMS: every set owns one rand() stream); no tests in here.

A case is a batch of n <= 12 fields cut into sets by `set_first`.  Expected pictures and states never come from the library: the oracle
(or the compiled reference) runs the reference's serial loop ONCE PER SET under srand(the set's seed) -- per field: display step;
settings with do_aberration; crt_modulate; crt_demodulate -- each set from its own incoming (hsync, vsync) and its own initial
picture (the models: tests/seqsets_cases.py:live_loop and test_gpu_parity.py:test_vhs_sequence_mode_equals_sequential_processing).
The VHS signal is CRT_INPUT_SIZE samples whatever the picture: 400x300 images into 416x312 BGRA, as that test."""
import ctypes as C

import numpy as np

import crtref as R
from test_phosphor_cpu import display_step_np

W, H, OUTW, OUTH = 400, 300, 416, 312
# With do_aberration the last lines of a field lose their sync pulse and their filter windows run past inp[] (undefined in the
# reference): exactly the last 12 output rows are not part of the contract, as in
# test_gpu_parity.py:test_vhs_sequence_mode_equals_sequential_processing -- and nothing else is excluded anywhere
ABERRATION_ROWS = 12
RAGGED = [0, 1, 4, 9, 10]                          # lengths 1, 3, 5, 1: a set of one field, and a one-field set behind a longer one
# every set's seed and state before its first field (the rand() build never reads the incoming rn: crt_core.c:349,367; the library
# is given RN_IN, the oracle keeps its default)
SEEDS = [20260924, 77, 31337, 4242]
HSYNC_IN = [7, -20, 40, 0]
VSYNC_IN = [2, 0, 5, 3]
RN_IN = [194, 77001, 5, 123456789]


def _case(id, noise, aberration, mode, blend, init, shapes=(0,), set_first=RAGGED, triples=None):
    return dict(id=id, name="vhs", noise=noise, aberration=aberration, mode=mode, knobs=dict(scanlines=0, blend=blend), init=init,
                shapes=shapes, set_first=set_first, triples=triples)


# (noise, mon_hue, saturation) per field of the batch for the _knobs entry point: distinct triples, a clean field inside the noisy
# set [4, 9) and a noisy field as a set of its own
TRIPLES = [(12, 0, 10), (3, -20, 14), (30, 15, 6), (9, 40, 12), (12, -5, 10), (24, 8, 18), (0, 25, 9), (17, -30, 11), (6, 3, 15), (21, 12, 7)]

# outh = 312 >= CRT_LINES: blend is accepted with v_fac = 0
CASES = [
    _case("n0-keep", 0, 0, "keep", 0, "per_set", shapes=(0, 1, 2)),
    _case("n12-keep-shared", 12, 0, "keep", 0, "shared", shapes=(0, 1, 2)),
    _case("n12-ab-keep-zeros", 12, 1, "keep", 0, "none", shapes=(0, 1, 2)),
    _case("n0-ab-fade", 0, 1, "fade", 0, "per_set"),
    _case("n0-clear-shared", 0, 0, "clear", 0, "shared"),
    _case("n12-blend-keep", 12, 0, "keep", 1, "per_set"),
    _case("n12-blend-fade-shared", 12, 0, "fade", 1, "shared", shapes=(0, 2)),
    _case("n12-ab-blend-clear-zeros", 12, 1, "clear", 1, "none"),
    _case("n12-ab-blend-fade", 12, 1, "fade", 1, "per_set", shapes=(0, 1)),
]
KNOB_CASES = [
    _case("knobs-keep", None, 0, "keep", 0, "per_set", triples=TRIPLES),
    _case("knobs-ab-blend-fade", None, 1, "fade", 1, "shared", triples=TRIPLES),
]
CASE_IDS = [c["id"] for c in CASES]
KNOB_CASE_IDS = [c["id"] for c in KNOB_CASES]


def case(id):
    return {c["id"]: c for c in CASES + KNOB_CASES}[id]


def n_fields(case):
    return case["set_first"][-1]


def sets_of(case):
    sf = case["set_first"]
    return [(sf[s], sf[s + 1]) for s in range(len(sf) - 1)]


def kept_rows(case):
    return OUTH - ABERRATION_ROWS if case["aberration"] else OUTH


def parities(case):
    """(field, frame) of every field: every set is a video of its own (extra/video_convert.c:261-267 from its field 0)"""
    return [((k - lo) & 1, ((k - lo + 1) >> 1) & 1) for lo, hi in sets_of(case) for k in range(lo, hi)]


def frames(case, seed=500):
    return np.stack([R.synth_image(W, H, 4, seed + k, "random" if k % 3 else "bars") for k in range(n_fields(case))])


def incoming(case):
    """[(hsync, vsync)] of every set before its first field"""
    return [(HSYNC_IN[s % 4], VSYNC_IN[s % 4]) for s in range(len(case["set_first"]) - 1)]


def seeds(case):
    return [SEEDS[s % 4] for s in range(len(case["set_first"]) - 1)]


def init_pictures(case):
    """None, one picture [outh, outw, 4] or one per set [n_sets, outh, outw, 4] (different seeds)"""
    shape = (OUTH, OUTW, 4)
    size = OUTH * OUTW * 4
    if case["init"] == "none":
        return None
    if case["init"] == "shared":
        return R.lcg_bytes(size, 5).reshape(shape)
    return np.stack([R.lcg_bytes(size, 5 + 11 * s).reshape(shape) for s in range(len(case["set_first"]) - 1)])


def init_of_set(init, s):
    if init is None:
        return np.zeros((OUTH, OUTW, 4), dtype=np.uint8)
    return init if init.ndim == 3 else init[s]


def field_knobs(case, k):
    """(noise, mon_hue, saturation) of field k: the case's triple, or the uniform noise with crt_init's hue and saturation"""
    return case["triples"][k] if case["triples"] else (case["noise"], 0, 10)


def aberration_height(lib, c):
    """the height crt_modulate drew (crt_ntscvhs.c:205-207), read off the oracle's own signal: the ordinary lines n >= CRT_VRES - height
    carry no sync pulse"""
    sd = lib.sys
    h = 0
    while int(c.analog[(sd.vres - 1 - h) * sd.hres + sd.sync_beg]) != sd.sync_level:
        h += 1
    return h


def stream_loop(lib, case, fr, par, lo, hi, init, state_in, seed, check_reads=False):
    """the reference's loop on ONE set = fields [lo, hi) of the batch under ONE rand() stream from srand(seed).  lib: R.Oracle("vhs")
    or R.RefLib("vhs").  Returns ([(out, hsync, vsync, rn, aux)] after every field, the stream's next rand() after the loop);
    aux = the aberration height drawn for the field (oracle with do_aberration only, else None).
    check_reads: no field may read past inp[] (crtref.reads_past_inp) on a line that writes a row of the contract."""
    c = lib.new_crt(OUTW, OUTH, R.FMT_BGRA)
    for k, v in case["knobs"].items():
        c.set(k, v)
    c.out[:] = init.reshape(-1)
    c.set("hsync", state_in[0])
    c.set("vsync", state_in[1])
    lib.srand(seed)
    want = []
    for k in range(lo, hi):
        noise, hue, sat = field_knobs(case, k)
        if case["mode"] != "keep":
            c.out[:] = display_step_np(c.out, R.FMT_BGRA, case["mode"])
        c.set("hue", hue)
        c.set("saturation", sat)
        pad = np.concatenate([fr[k], fr[k][-1:]], axis=0)
        c.settings(pad, format=R.FMT_BGRA, w=W, h=H, as_color=1, field=par[k][0], frame=par[k][1], do_aberration=case["aberration"])
        c.modulate()
        aux = aberration_height(lib, c) if case["aberration"] and isinstance(lib, R.Oracle) else None
        hs_before = c.get("hsync")
        if check_reads:
            c.demodulate(noise, trace=True)
            # the lines come in row order: those in front of the first line that starts inside the excluded rows
            m = int(np.argmax(c.trace[:, 4] >= kept_rows(case))) if (c.trace[:, 4] >= kept_rows(case)).any() else c.trace.shape[0]
            assert not R.reads_past_inp(lib, c.trace[:m], c.get("vsync"), hs_before), \
                "%s field %d: the reference reads past inp[] here (undefined): pick another seed / noise / hsync" % (case["id"], k)
        else:
            c.demodulate(noise)
        want.append((c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn"), aux))
    return want, C.CDLL(None).rand()                       # (the oracle and the compiled reference both draw from libc's one stream)


def expected(case, lib=None, check_reads=False):
    """per-set loops of the oracle (or `lib`) -> ([(out, hsync, vsync, rn, aux)] for every field in batch order, [next rand() of every
    set's stream after its last field])"""
    lib = lib or R.Oracle("vhs")
    fr, par, init, inc, sd = frames(case), parities(case), init_pictures(case), incoming(case), seeds(case)
    want, nxt = [], []
    for s, (lo, hi) in enumerate(sets_of(case)):
        w, r = stream_loop(lib, case, fr, par, lo, hi, init_of_set(init, s), inc[s], sd[s], check_reads)
        want += w
        nxt.append(r)
    return want, nxt


def expected_one_stream(case):
    """the same fields under ONE stream from set 0's seed, as one long set from set 0's incoming pair and picture: what a library
    without per-set streams would compute"""
    lib = R.Oracle("vhs")
    return stream_loop(lib, case, frames(case), parities(case), 0, n_fields(case), init_of_set(init_pictures(case), 0),
                       incoming(case)[0], seeds(case)[0])[0]

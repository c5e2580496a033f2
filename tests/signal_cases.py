"""Arbitrary signals for the stage-level entry points (TEST INFRASTRUCTURE ONLY; numpy and the CPU oracle, no GPU).

Every GPU test before this one decoded what the library's own encoder had made.  Here analog[] is written by hand: the sync skeleton
comes from the oracle's modulate() of a 64 x 48 picture, then named regions are overwritten.

* burst window: bytes chosen line by line with an integer model of the ccf recurrence (crt_core.c:462-477, p * 127 / 128 with C's
  truncation) so that the per-line carrier amplitude follows a schedule -- a ramp through the decoder's three dispatch bounds, or a
  line exactly AT a bound and another just above it;
* active window (from 8 samples before AV_BEG to the line's end): per line one of PATTERNS, all at +-127;
* sync edges and the noise stage's clamp: SYNC_CASES, NOISE_CASES.

The bounds are the documented ones, restated here and never read from the library.  What a case claims to reach is
asserted on the oracle's trace by tests/test_signals_cpu.py; tests/test_gpu_signals.py runs the same cases on the GPU."""
import numpy as np

import crtref as R

W, H = 64, 48
LOSKIP_WAVE_MAX, T0_WAVE_MAX, FAST_WAVE_MAX, T0_BRIGHT_MAX = 65532, 120000, 524288, 2600
BOUNDS = (LOSKIP_WAVE_MAX, T0_WAVE_MAX, FAST_WAVE_MAX)
HIT_LINE, ABOVE_LINE = 120, 132                # decoded lines (index from CRT_TOP) that carry "exactly the bound" and "just above"

PATTERNS = ("signI", "signQ", "const+", "const-", "sq2", "sq4a0", "sq4a1", "sq4a2", "sq4a3", "sq8", "sq16", "sq64", "step", "impulse",
            "random")

_ORC = {}


def oracle(name):
    if name not in _ORC:
        _ORC[name] = R.Oracle(name)
    return _ORC[name]


def c_div(a, b):
    """C's integer division (toward zero)"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def c_mod(a, b):
    return a - b * c_div(a, b)


def ccf_step(p, s):
    """ccf[k] = ccf[k] * 127 / 128 + sample, crt_core.c:464"""
    return c_div(p * 127, 128) + s


def _ccf_steps_vec(p, s):
    q = p * 127
    return np.where(q >= 0, q // 128, -((-q) // 128)) + s


def hue_terms(orc, hue):
    """huesn, huecs of crt_core.c:318-320"""
    sn, cs = orc.sincos14(c_div((c_mod(hue, 360) + 33) * 8192, 180))
    return sn >> 11, cs >> 11


_SKEL = {}


def skeleton(name):
    """analog[] of a 64 x 48 picture (256 x 240 PPU pixels for the NES), as the oracle's modulate() leaves it"""
    if name not in _SKEL:
        orc = oracle(name)
        c = orc.new_crt(W, H, R.FMT_BGRA)
        if name == "nes":
            img = R.synth_ppu(256, 240, 8100)
            c.settings(np.concatenate([img, img[-1:]]).astype(np.uint16), w=256, h=240, dot_crawl_offset=0, hue=0)
            c.sset("field_initialized", 0)
        else:
            img = R.synth_image(W, H, 4, 8100)
            c.settings(np.concatenate([img, img[-1:]]), format=R.FMT_BGRA, w=W, h=H, as_color=1, field=0, frame=0)
            if orc.system in R.DOT_CRAWL_SYSTEMS:
                c.sset("dot_crawl_offset", 0)
        c.modulate()
        _SKEL[name] = c.analog.copy()
    return _SKEL[name].copy()


def set_ccf(c, ccf):
    if hasattr(c, "v"):
        for r in range(ccf.shape[0]):
            for k in range(ccf.shape[1]):
                c.v.ccf[r][k] = int(ccf[r][k])
    else:
        c.ccf[:] = ccf


def run_checker(lib, signal, knobs, start, noise, steps, geom=(W, H, R.FMT_BGRA)):
    """`steps` consecutive demodulate() calls of `lib` (the Oracle, or the real reference: RefLib) on one analog[], from the start
    state (hsync, vsync, ccf).  Per step a dict; from the step on in which the reference's reads leave inp[] + 16
    (crtref.reads_past_inp, judged on the oracle's trace) `undefined` is True and stays so."""
    c = lib.new_crt(*geom)
    for k, v in knobs.items():
        c.set(k, v)
    c.set("hsync", start[0])
    c.set("vsync", start[1])
    set_ccf(c, start[2])
    c.analog[:] = signal
    res, undefined = [], False
    for _ in range(steps):
        hs_before = c.get("hsync")
        if isinstance(lib, R.Oracle):
            c.demodulate(noise, trace=True)
            undefined = undefined or R.reads_past_inp(lib, c.trace, c.get("vsync"), hs_before)
            trace = c.trace.copy()
        else:
            c.demodulate(noise)
            trace = None
        res.append(dict(inp=np.array(c.inp).copy(), trace=trace, hsync=c.get("hsync"), vsync=c.get("vsync"), rn=c.get("rn"),
                        ccf=np.array(c.ccf).copy(), out=c.out.copy(), undefined=undefined))
    return res


_FREE = {}


def free_lines(name):
    """field lines no vsync search of a locked field looks at (two windows around the lock vsync, crt_core.c:379-396): free to
    overwrite with anything without moving the field"""
    if name not in _FREE:
        sd = oracle(name).sys
        free = np.ones(sd.vres, dtype=bool)
        for i in range(-2 * sd.vsync_window, 2 * sd.vsync_window):
            free[(_lock_start(name)[1] + i) % sd.vres] = False
        _FREE[name] = free
    return _FREE[name]


def zero_ccf(name):
    orc = oracle(name)
    return np.zeros((orc.vper, orc.ccs), dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# the model of the carrier chain: ccf recurrence and the line's carriers (crt_core.c:452-510)
# ---------------------------------------------------------------------------------------------------------------------------
def line_geometry(name, trace, vsync):
    """per decoded line of an oracle trace: (index, field line of sync and burst, field line of the video, hsync, pos)"""
    sd = oracle(name).sys
    rows = []
    for idx in range(trace.shape[0]):
        if int(trace[idx, 0]) != 1:
            continue
        ln = (sd.top + idx + vsync) % sd.vres
        rows.append((idx, ln, (ln + 3) % sd.vres, int(trace[idx, 6]), int(trace[idx, 1])))
    return rows


def burst_positions(sd, ln, hsync):
    """[(flat index, ccf bin)] of the burst samples a line with this hsync reads"""
    base = ln * sd.hres + (hsync & ~3 if sd.cc_samples == 4 else hsync - hsync % sd.cc_samples)
    return [(base + i, i % sd.cc_samples) for i in range(sd.cb_beg, sd.cb_beg + sd.cb_len)]


def carriers(sd, ccr, hsync, sn, cs, saturation):
    """what the trace calls wave0, wave1 (4 samples per cycle: the carriers; 5: dci, dcq), and the amplitude the dispatch compares"""
    n = sd.cc_samples
    a = hsync % n
    if n == 4:
        dci = ccr[(a + 1) & 3] - ccr[(a + 3) & 3]
        dcq = ccr[(a + 2) & 3] - ccr[a & 3]
        w0 = ((dci * cs - dcq * sn) >> 4) * saturation
        w1 = ((dcq * cs + dci * sn) >> 4) * saturation
        return w0, w1, max(abs(w0), abs(w1))
    dci = ccr[(a + 1) % 5] - c_div(ccr[(a + 3) % 5] + ccr[(a + 4) % 5], 2)
    dcq = ccr[(a + 2) % 5] - ccr[a % 5]
    return dci, dcq, (abs(dci) + abs(dcq) + 1) * abs(saturation)


def model_waves(name, inp, geometry, ccf0, hue, saturation):
    """the integer model on a finished inp[]: {line index: (wave0, wave1, amplitude)}"""
    orc = oracle(name)
    sd = orc.sys
    sn, cs = hue_terms(orc, hue)
    ccf = [[int(v) for v in row] for row in ccf0]
    flat = np.concatenate([np.asarray(inp, dtype=np.int64), np.zeros(R.ORC_TAIL, dtype=np.int64)])
    got = {}
    for idx, ln, vln, hs, pos in geometry:
        ccr = ccf[vln % sd.cc_vper]
        for at, k in burst_positions(sd, ln, hs):
            ccr[k] = ccf_step(ccr[k], int(flat[at]))
        got[idx] = carriers(sd, ccr, hs, sn, cs, saturation)
    return got


def _drive(p, target):
    """ten burst samples for one ccf bin: nine equal ones and a last one, ending as near `target` as ten samples can"""
    b = np.arange(-127, 128, dtype=np.int64)
    q = np.full(255, p, dtype=np.int64)
    for _ in range(9):
        q = _ccf_steps_vec(q, b)
    d = _ccf_steps_vec(q, 0)
    last = np.clip(target - d, -127, 127)
    end = d + last
    k = int(np.argmin(np.abs(end - target) * 256 + np.abs(b)))
    return [int(b[k])] * 9 + [int(last[k])], int(end[k])


def _bin_targets(sd, hsync, sn, cs, want):
    """ccf values that give the wanted carriers.  want = (units, dominant, sign): 4 samples per cycle -- carrier `dominant` / saturation
    = sign * units and the other one smaller; 5 samples -- |dci| + |dcq| = units, dci carrying `sign`"""
    units, dom, sign = want
    n = sd.cc_samples
    a = hsync % n
    t = [0] * n
    if n == 5:
        dci = sign * (units - units // 2)
        dcq = -sign * (units // 2)
        t[(a + 1) % 5] = dci - dci // 2
        t[(a + 3) % 5] = t[(a + 4) % 5] = -(dci // 2)
        t[(a + 2) % 5] = dcq - dcq // 2
        t[a % 5] = -(dcq // 2)
        return t
    nn = cs * cs + sn * sn
    x = sign * units * 16
    ci, cq = (x * cs / nn, -x * sn / nn) if dom == 0 else (x * sn / nn, x * cs / nn)
    best = None
    for dci in range(int(ci) - 24, int(ci) + 25):
        for dcq in range(int(cq) - 24, int(cq) + 25):
            xs = ((dci * cs - dcq * sn) >> 4, (dcq * cs + dci * sn) >> 4)
            err = abs(xs[dom] - sign * units) * 1000 + abs(xs[1 - dom])
            if best is None or err < best[0]:
                best = (err, dci, dcq)
    _, dci, dcq = best
    t[(a + 1) & 3] = dci - dci // 2
    t[(a + 3) & 3] = -(dci // 2)
    t[(a + 2) & 3] = dcq - dcq // 2
    t[a & 3] = -(dcq // 2)
    return t


def write_bursts(name, analog, geometry, ccf0, hue, schedule):
    """walks the field's decoded lines in order; where schedule(index) names carriers and the line is locked and free, the line's
    burst samples are rewritten so that the model's ccf lands on them (or as near as a line's forty samples can bring it)"""
    orc = oracle(name)
    sd = orc.sys
    sn, cs = hue_terms(orc, hue)
    ccf = [[int(v) for v in row] for row in ccf0]
    hs_all = [g[3] for g in geometry]
    lock = max(set(hs_all), key=hs_all.count)
    free = free_lines(name)
    seen = np.zeros(analog.size + 2 * sd.hres, dtype=bool)      # samples an earlier line has read as they were: not rewritten
    for idx, ln, vln, hs, pos in geometry:
        ccr = ccf[vln % sd.cc_vper]
        at = burst_positions(sd, ln, hs)
        want = schedule(idx)
        if want is None or hs != lock or not free[ln] or any(seen[p] for p, k in at):
            for p, k in at:
                ccr[k] = ccf_step(ccr[k], max(int(analog[p]), -127) if p < analog.size else 0)
                seen[p] = True
            continue
        targets = _bin_targets(sd, hs, sn, cs, want)
        for k in range(sd.cc_samples):
            samples, ccr[k] = _drive(ccr[k], targets[k])
            for p, s in zip([p for p, kk in at if kk == k], samples):
                analog[p] = s


def _pattern_bytes(pattern, n, waves, rng):
    i = np.arange(n)
    if pattern == "const+":
        return np.full(n, 127)
    if pattern == "const-":
        return np.full(n, -127)
    if pattern.startswith("sq4a"):
        return np.where(((i + int(pattern[4:])) & 3) < 2, 127, -127)
    if pattern.startswith("sq"):
        per = int(pattern[2:])
        return np.where((i % per) < per // 2, 127, -127)
    if pattern in ("signI", "signQ"):
        # 127 * sign(wave[(i + 0) & 3]) / sign(wave[(i + 3) & 3]): every product of the I / the Q demodulator at its positive maximum
        w0, w1 = waves
        four = np.array([w0, w1, -w0, -w1])
        w = four[(i + (0 if pattern == "signI" else 3)) & 3]
        return np.where(w >= 0, 127, -127)
    if pattern == "step":
        return np.where(i < n // 2, -127, 127)
    if pattern == "impulse":
        return np.where(i == n // 2, 127, -127)
    if pattern == "random":
        return rng.integers(-127, 128, n)
    raise ValueError(pattern)


def write_active(name, analog, geometry, waves, pattern_of, seed):
    """the active window of every free video line: from 8 samples in front of the decoder's first sample to the line's end; pattern
    sample 0 is the decoder's sample 0"""
    sd = oracle(name).sys
    rng = np.random.default_rng(seed)
    free = free_lines(name)
    for idx, ln, vln, hs, pos in geometry:
        if not free[vln] or pos // sd.hres != vln:
            continue
        pattern = pattern_of(idx)
        if pattern is None:
            continue
        end = (vln + 1) * sd.hres
        w = waves[idx][:2] if sd.cc_samples == 4 else (1, 1)
        body = _pattern_bytes(pattern, end - pos + 8, w, rng)
        lead = _pattern_bytes(pattern, 16, w, rng)[8:] if pattern != "random" else rng.integers(-127, 128, 8)
        analog[pos - 8:pos] = lead[:8]
        analog[pos:end] = body[:end - pos]


# ---------------------------------------------------------------------------------------------------------------------------
# amplitude and filter cases: from lock
# ---------------------------------------------------------------------------------------------------------------------------
_LOCK = {}


def _lock_start(name):
    """the start state a field of this system settles in: (hsync, vsync) after two passes from 0, 0 on the plain skeleton"""
    if name not in _LOCK:
        r = run_checker(oracle(name), skeleton(name), {}, (0, 0, zero_ccf(name)), 0, 2)
        _LOCK[name] = (r[1]["hsync"], r[1]["vsync"])
    return _LOCK[name]


def ramp_schedule(sat):
    """carrier amplitude 4 000 per decoded line: through 65 532, 120 000 and 524 288 inside one field"""
    def sched(idx):
        return (max(1, 4000 * (idx + 1) // abs(sat)), 0, 1 if sat > 0 else -1)
    return sched


def hit_schedule(bound, sat, dom=0, sign=1):
    """hold the bound exactly up to HIT_LINE, then one unit of |saturation| above it: bound < amplitude <= bound + |saturation|"""
    assert bound % abs(sat) == 0
    four = bound // abs(sat)

    def sched(idx):
        return (four + (1 if idx > HIT_LINE else 0), dom, sign)
    return sched


def hit_schedule5(bound, sat, sign=1):
    """PV-1000: (|dci| + |dcq| + 1) * |saturation| at the bound, then one unit above"""
    assert bound % abs(sat) == 0
    units = bound // abs(sat) - 1

    def sched(idx):
        return (units + (1 if idx > HIT_LINE else 0), 0, sign)
    return sched


def _field(kind, bound=0, dom=0, sign=1, rot=0, corner=None, seed=1):
    return dict(kind=kind, bound=bound, dom=dom, sign=sign, rot=rot, corner=corner, seed=seed)


def _amp_case(name, fields, noise=0, floats=None, **knobs):
    """floats: what float_stages_used must say with the switch on and the lane-per-scanline shape (None: by the documented rule)"""
    return dict(group="amp", name=name, fields=fields, noise=noise, knobs=knobs, floats=floats, steps=2)


def _bright(name, bright):
    """the brightness knob that gives the decoder's `bright` (crt_core.c:305: brightness - (BLACK_LEVEL + black_point))"""
    return bright + oracle(name).sys.black_level


def _amp_cases():
    cases = {}
    for name in ("ntsc", "ntscp0", "snes", "nes", "vhslcg", "ntscfir7", "ntscbloom"):
        blocks = name == "ntscbloom"
        rot = "blocks" if blocks else 0
        cases[name + "-ramp"] = _amp_case(name, [_field("ramp", sign=1, rot=rot, seed=11), _field("ramp", sign=-1, rot=5, seed=12)],
                                          saturation=16)
        cases[name + "-at65532"] = _amp_case(name, [_field("hit", LOSKIP_WAVE_MAX, 0, 1, rot, "signI", 21),
                                                    _field("hit", LOSKIP_WAVE_MAX, 1, -1, 3, "signQ", 22)], saturation=12)
        cases[name + "-at120000"] = _amp_case(name, [_field("hit", T0_WAVE_MAX, 0, -1, rot, "signI", 31),
                                                     _field("hit", T0_WAVE_MAX, 1, 1, 7, "signQ", 32)], saturation=10)
        cases[name + "-at524288"] = _amp_case(name, [_field("hit", FAST_WAVE_MAX, 0, 1, rot, "signI", 41),
                                                     _field("hit", FAST_WAVE_MAX, 0, -1, 9, "signQ", 42)], saturation=16)
    corner = [_field("hit", T0_WAVE_MAX, 0, 1, 0, "signI", 51), _field("hit", T0_WAVE_MAX, 0, -1, 1, "signQ", 52),
              _field("hit", T0_WAVE_MAX, 1, 1, 2, "signI", 53), _field("hit", T0_WAVE_MAX, 1, -1, 4, "signQ", 54)]
    # the corner that matters most: amplitude 120 000, |bright| = 2 600, sign-matched +-127 -- and one step of brightness beyond
    # WHICH KERNEL DECODES THESE LINES.  At the stage-level entry points and in the drop-in crt_demodulate, loskip_wave_max is the
    # any-signal value 65 532 (crthip_params_finalize), so every line above 65 532 is flagged "keep the low cascades" and its whole wave
    # of 64 lines is decoded by the 24-bit tier 2 -- at 120 000 (WIDE | KEEPLO) as at 120 010 (NOT64).  The 120 000 cases therefore test
    # the dispatch flags and tier 2 at that amplitude, NOT tier 1 or the float kernel: float_stages_used() == 1 only says which
    # instantiation was launched, the waves that hold these lines leave it at once.  For the same reason a seeded T0_WAVE_MAX of 120 010
    # cannot change a byte here (tried: all tests pass), like the seeded LOSKIP_WAVE_MAX below; nothing about the bound's slack follows.
    # Tier 1 and the float stages at |wave| in (65 532, 120 000] are reached only by the fused entry points, which widen
    # loskip_wave_max for encoder-made signals (tests/test_gpu_float_stages.py, test_gpu_parity.py); at this corner their arithmetic is
    # covered by the host model on the CPU (test_float_stage_model_holds_on_the_corner_inputs) and not by a GPU test.
    # What the GPU does decode in tier 0 / the float kernel here: the waves whose 64 lines all stay at or below 65 532 -- the early
    # lines of every ramp, and lines 20 .. 63 of the at65532 fields, which hold exactly 65 532 under the whole pattern rotation.
    cases["ntsc-corner-bright+2600"] = _amp_case("ntsc", corner, saturation=10, brightness=_bright("ntsc", 2600), contrast=20)
    cases["ntsc-corner-bright-2600"] = _amp_case("ntsc", corner, saturation=10, brightness=_bright("ntsc", -2600), contrast=400)
    cases["ntsc-corner-bright+2601"] = _amp_case("ntsc", corner, floats=0, saturation=10, brightness=_bright("ntsc", 2601), contrast=20)
    cases["ntsc-corner-bright-2601"] = _amp_case("ntsc", corner, floats=0, saturation=10, brightness=_bright("ntsc", -2601), contrast=400)
    cases["ntsc-corner-sat-10-hue"] = _amp_case("ntsc", corner[:2], saturation=-10, hue=17, brightness=_bright("ntsc", -2600))
    cases["ntsc-corner-sat12-hue"] = _amp_case("ntsc", corner[:2], saturation=12, hue=-40, brightness=_bright("ntsc", 2600), contrast=400)
    cases["ntsc-at65532-sat-4"] = _amp_case("ntsc", [_field("hit", LOSKIP_WAVE_MAX, 0, 1, 0, "signI", 61),
                                                     _field("hit", LOSKIP_WAVE_MAX, 1, 1, 6, "signQ", 62)], saturation=-4, hue=200)
    # saturation +4: the line above the bound sits at 65 536 with the dominant carrier POSITIVE, so carrier << 7 is 2^23 itself, the
    # first value that is no 24-bit signed multiplier (sat -4 above reaches the same amplitude through the negative member).
    # At the stage-level entry points this bound is guarded twice: crthip_params_finalize sets loskip_wave_max to the any-signal
    # value 65 532, so every line above it is flagged "keep the low cascades" and decoded by the 24-bit tier whatever the "carrier
    # << 7 is too wide" flag says.  A seeded LOSKIP_WAVE_MAX of 65 540 therefore changes no result here (tried: all tests pass); the
    # flag decides only in the fused entry points, whose loskip_wave_max is wider on encoder-made signals.
    cases["ntsc-at65532-sat4"] = _amp_case("ntsc", [_field("hit", LOSKIP_WAVE_MAX, 0, 1, 0, "signI", 63),
                                                    _field("hit", LOSKIP_WAVE_MAX, 1, 1, 6, "signQ", 64),
                                                    _field("hit", LOSKIP_WAVE_MAX, 0, -1, 3, "signI", 65)], saturation=4)
    cases["ntsc-ramp-noise"] = _amp_case("ntsc", [_field("ramp", sign=1, rot=2, seed=71), _field("ramp", sign=-1, rot=8, seed=72)],
                                         noise=24, saturation=-16, hue=77)
    # PV-1000, 5 samples per chroma cycle: the bounds on (|dci| + |dcq| + 1) * |saturation|
    cases["pv1k-ramp"] = _amp_case("pv1k", [_field("ramp", sign=1, rot=0, seed=81), _field("ramp", sign=-1, rot=5, seed=82)],
                                   saturation=16)
    cases["pv1k-at65532"] = _amp_case("pv1k", [_field("hit", LOSKIP_WAVE_MAX, 0, 1, 0, "const+", 83),
                                               _field("hit", LOSKIP_WAVE_MAX, 0, -1, 3, "const-", 84)], saturation=12)
    cases["pv1k-at120000"] = _amp_case("pv1k", [_field("hit", T0_WAVE_MAX, 0, 1, 0, "const+", 85),
                                                _field("hit", T0_WAVE_MAX, 0, -1, 3, "const-", 86)], saturation=10)
    cases["pv1k-at524288"] = _amp_case("pv1k", [_field("hit", FAST_WAVE_MAX, 0, 1, 0, "const+", 87),
                                                _field("hit", FAST_WAVE_MAX, 0, -1, 3, "const-", 88)], saturation=16)
    return cases


AMP_CASES = _amp_cases()
_BUILT = {}


def _pattern_of(f):
    if f["rot"] == "blocks":
        # bloom: blocks of constant +127 and -127 lines, so the beam width swings across the lane-per-scanline decoder's sort buckets
        def of(idx):
            if idx in (HIT_LINE, ABOVE_LINE) and f["corner"]:
                return f["corner"]
            return ("const+", "const-", "const+", "random", "const-")[(idx // 9) % 5]
        return of

    def of(idx):
        if idx in (HIT_LINE, ABOVE_LINE) and f["corner"]:
            return f["corner"]
        return PATTERNS[(idx + f["rot"]) % len(PATTERNS)]
    return of


def build_amp_field(name, f, knobs):
    """-> (analog, start state, geometry of pass 0, the model's carriers of pass 0)"""
    orc = oracle(name)
    sat, hue = knobs.get("saturation", 10), knobs.get("hue", 0)
    start = _lock_start(name) + (zero_ccf(name),)
    analog = skeleton(name)
    first = run_checker(orc, analog, {}, start, 0, 1)[0]
    geometry = line_geometry(name, first["trace"], first["vsync"])
    five = orc.ccs == 5
    if f["kind"] == "ramp":
        inner = ramp_schedule(sat)

        def sched(idx):
            u, d, s = inner(idx)
            return (u, f["dom"], f["sign"])
    elif five:
        sched = hit_schedule5(f["bound"], sat, f["sign"])
    else:
        sched = hit_schedule(f["bound"], sat, f["dom"], f["sign"])
    write_bursts(name, analog, geometry, start[2], hue, sched)
    waves = model_waves(name, analog, geometry, start[2], hue, sat)
    write_active(name, analog, geometry, waves, _pattern_of(f), f["seed"])
    waves = model_waves(name, analog, geometry, start[2], hue, sat)      # (the active window must not have reached a burst)
    return analog, start, geometry, waves


def build_case(cid):
    """-> dict(signals [n, input_size] int8, starts, geometry, waves) of an AMP / SYNC / NOISE case; built once"""
    if cid in _BUILT:
        return _BUILT[cid]
    case = ALL_CASES[cid]
    sig, starts, geos, waves = [], [], [], []
    for f in case["fields"]:
        if case["group"] == "amp":
            a, st, g, w = build_amp_field(case["name"], f, case["knobs"])
        else:
            a, st = f["build"](case["name"])
            g, w = None, None
        sig.append(a)
        starts.append(st)
        geos.append(g)
        waves.append(w)
    _BUILT[cid] = dict(signals=np.stack(sig).astype(np.int8), starts=starts, geometry=geos, waves=waves)
    return _BUILT[cid]


_WANT = {}


def expected(cid, geom=(W, H, R.FMT_BGRA)):
    """the oracle's results of a case, [field][step] (run_checker), for one output geometry; computed once and left alone"""
    key = (cid, geom)
    if key not in _WANT:
        case, b = ALL_CASES[cid], build_case(cid)
        _WANT[key] = [run_checker(oracle(case["name"]), b["signals"][k], case["knobs"], b["starts"][k], case["noise"], case["steps"], geom)
                      for k in range(len(case["fields"]))]
    return _WANT[key]


# ---------------------------------------------------------------------------------------------------------------------------
# sync edges (NTSC): each field is the skeleton with a few lines rewritten, and the start state that makes the edge happen
# ---------------------------------------------------------------------------------------------------------------------------
SYNC_GEOM = (64, 480, R.FMT_BGRA)       # 480 rows: the field parity shows in the rows (crt_core.c:403-407), so in the line table
VS0 = 130                               # vsync start state of the vsync cases: the search looks at field lines 122 .. 137


def _quiet_vsync_window(analog, sd, vs0):
    """the lines a vsync search from vs0 looks at keep their hsync pulse and nothing else: none of them reaches the threshold"""
    for i in range(-sd.vsync_window, sd.vsync_window):
        ln = (vs0 + i) % sd.vres
        line = analog[ln * sd.hres:(ln + 1) * sd.hres]
        pulse = line[:sd.bw_beg].copy()
        line[:] = 0
        line[:sd.bw_beg] = pulse
    return analog


def _vsync_field(*runs):
    """runs: (field line, first sample, samples) -- the line is zero but for these samples"""
    def build(name):
        sd = oracle(name).sys
        a = _quiet_vsync_window(skeleton(name), sd, VS0)
        for ln, at, run in runs:
            line = a[ln * sd.hres:(ln + 1) * sd.hres]
            line[:] = 0
            line[at:at + len(run)] = run
        return a, (3, VS0, zero_ccf(name))
    return dict(build=build)


def _hsync_field(window):
    """the sixteen samples of the first decoded line's hsync search, from lock"""
    def build(name):
        orc = oracle(name)
        sd = orc.sys
        hs, vs = _lock_start(name)
        a = skeleton(name)
        ln = (sd.top + vs) % sd.vres
        at = ln * sd.hres + hs + sd.sync_beg - sd.hsync_window
        a[at:at + 2 * sd.hsync_window] = window
        return a, (hs, vs, zero_ccf(name))
    return dict(build=build)


def _no_sync_field():
    """no sample below zero anywhere: neither search ever meets its threshold; hsync walks on by the window per line, through HRES
    and round (POSMOD).  Start hsync 110: in pass 0 the walk is at 8 .. 32 when the field's last lines are read, so the reference
    stays inside inp[] + 16.  No start state keeps BOTH passes inside (the walk is 44 samples further on at the same lines of the
    next pass): pass 1 of this field is the one exclusion of its case."""
    def build(name):
        a = skeleton(name)
        a[a < 0] = 0
        return a, (110, VS0, zero_ccf(name))
    return dict(build=build)


def _tail_field():
    """the whole signal 7 samples and 100 lines late: lock is hsync 10, and the decoded line whose video is field line VRES - 1 reads
    past the field's end into the bytes mirrored behind it (outw, outh: the byte -128 for widths 128 and 640)"""
    def build(name):
        sd = oracle(name).sys
        hs, vs = _lock_start(name)
        a = np.roll(skeleton(name), 100 * sd.hres + 7)
        return a, ((hs + 7) % sd.hres, (vs + 100) % sd.vres, zero_ccf(name))
    return dict(build=build)


def _sync_case(fields, geom=SYNC_GEOM, name="ntsc", **knobs):
    return dict(group="sync", name=name, fields=fields, noise=0, knobs=knobs, floats=None, steps=2, geom=geom)


T_V, T_H = -3760, -160                  # VSYNC_THRESH * SYNC_LEVEL = 94 * -40, HSYNC_THRESH * SYNC_LEVEL = 4 * -40 (crt_ntsc.h)
SYNC_CASES = {
    # field 0: nothing reaches the threshold (gives up: last line of the window, j == HRES, odd); 1: the sum equals it exactly;
    # 2: stays one above on that line, the next line meets it; 3: first met at j == HRES / 2 (even); 4: at HRES / 2 + 1 (odd);
    # 5: thirty samples of -127, the earliest j there is
    "vsync-edges": _sync_case([
        _vsync_field(),
        _vsync_field((VS0 - 3, 0, [-40] * 94)),
        _vsync_field((VS0 - 3, 0, [-40] * 93 + [-39]), (VS0 - 2, 0, [-40] * 94)),
        _vsync_field((VS0 - 3, 455 - 93, [-40] * 94)),
        _vsync_field((VS0 - 3, 456 - 93, [-40] * 94)),
        _vsync_field((VS0 - 3, 0, [-127] * 30)),
    ]),
    # field 0: met on the window's second sample, with equality, and not again; 1: met on its last sample, with equality;
    # 2: one short of the threshold from the second sample on (never met on this line); 3: one short, then equal on the fourth
    "hsync-edges": _sync_case([
        _hsync_field([-100, -60, 60] + [0] * 13),
        _hsync_field([-10] * 16),
        _hsync_field([-127, -32] + [0] * 14),
        _hsync_field([-127, -32, 0, -1, 1] + [0] * 11),
        _no_sync_field(),                                   # 4: never met on any line of the field
    ]),
    # The sync chain is one kernel template over the system's constants (window, threshold, SYNC_BEG, HRES, lines per ccf row), so the
    # full set of edges runs on NTSC; the hsync edges run once more on the two other geometries there are: the PV-1000 (HRES 1920, 5
    # samples per chroma cycle, 5 ccf rows; same window of 16) and the SNES (window of 12, 3 ccf rows) -- the same four fields
    "pv1k-hsync-edges": _sync_case([
        _hsync_field([-100, -60, 60] + [0] * 13),
        _hsync_field([-10] * 16),
        _hsync_field([-127, -32] + [0] * 14),
        _hsync_field([-127, -32, 0, -1, 1] + [0] * 11),
    ], name="pv1k"),
    "snes-hsync-edges": _sync_case([
        _hsync_field([-100, -60, 60] + [0] * 9),
        _hsync_field([-14] * 11 + [-6]),
        _hsync_field([-127, -32] + [0] * 10),
        _hsync_field([-127, -32, 0, -1, 1] + [0] * 7),
    ], name="snes"),
    "tail-128": _sync_case([_tail_field(), _tail_field()], geom=(128, 48, R.FMT_BGRA)),
    "tail-640": _sync_case([_tail_field(), _tail_field()], geom=(640, 48, R.FMT_RGB)),
}
VSYNC_WANT = [(VS0 + 7, 1), (VS0 - 3, 0), (VS0 - 2, 0), (VS0 - 3, 0), (VS0 - 3, 1), (VS0 - 3, 0)]     # (vsync, odd field) after pass 0
# first line's hsync - start hsync: second sample, last sample, never (the window's half width on), fourth sample
HSYNC_WANT = {"hsync-edges": [-7, 7, 8, -5], "pv1k-hsync-edges": [-7, 7, 8, -5], "snes-hsync-edges": [-5, 5, 6, -3]}


# ---------------------------------------------------------------------------------------------------------------------------
# the noise stage's clamps (crt_core.c:362-364)
# ---------------------------------------------------------------------------------------------------------------------------
NOISE_VALUES = (0, 1, 255, 256, -24, 50000000)


def _noise_field(seed):
    def build(name):
        sd = oracle(name).sys
        a = skeleton(name)
        rng = np.random.default_rng(seed)
        for ln in np.flatnonzero(free_lines(name)):
            line = a[ln * sd.hres + sd.av_beg - 8:(ln + 1) * sd.hres]
            k = 0
            while k < line.size:
                run = int(rng.integers(1, 60))
                mode = int(rng.integers(0, 5))
                line[k:k + run] = (-128, -127, 0, 127)[mode] if mode < 4 else rng.integers(-128, 128, min(run, line.size - k))
                k += run
        hs, vs = _lock_start(name)
        return a, (hs, vs, zero_ccf(name))
    return dict(build=build)


# the noise stage is one kernel over INPUT_SIZE bytes: one system per field size and generator path (HRES 910, 909, 1920; the VHS
# build with the LCG; the NES with its own levels)
NOISE_CASES = {}
for _name in ("ntsc", "vhslcg", "pv1k", "snes", "nes"):
    for _noise in NOISE_VALUES:
        NOISE_CASES["%s-noise%d" % (_name, _noise)] = dict(group="noise", name=_name, fields=[_noise_field(91), _noise_field(92)],
                                                           noise=_noise, knobs={}, floats=None, steps=2)

ALL_CASES = dict(AMP_CASES)
ALL_CASES.update(SYNC_CASES)
ALL_CASES.update(NOISE_CASES)


def case_geom(cid):
    return ALL_CASES[cid].get("geom", (W, H, R.FMT_BGRA))


def case_bright(cid):
    case = ALL_CASES[cid]
    return case["knobs"].get("brightness", 0) - oracle(case["name"]).sys.black_level


def line_amplitudes(cid, k, step=0):
    """per decoded line of field k's oracle trace: the amplitude the dispatch compares (0 for lines that are not decoded)"""
    case = ALL_CASES[cid]
    sd = oracle(case["name"]).sys
    tr = expected(cid, case_geom(cid))[k][step]["trace"]
    sat = abs(case["knobs"].get("saturation", 10))
    a0, a1 = np.abs(tr[:, 2].astype(np.int64)), np.abs(tr[:, 3].astype(np.int64))
    amp = np.maximum(a0, a1) if sd.cc_samples == 4 else (a0 + a1 + 1) * sat
    return np.where(tr[:, 0] == 1, amp, 0)

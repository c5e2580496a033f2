"""Encoder-made fields whose carrier amplitude lands within one |saturation| of the decoder's dispatch bounds, through the FUSED entry
points (TEST INFRASTRUCTURE ONLY; numpy and the CPU oracle, no GPU).

Only the fused entry points widen crthip_params.loskip_wave_max (crt_setup_signal_range + crt_setup_loskip_bound, crt_setup.c), so only
there does a line with 65 532 < |wave| <= B run decoder tier 1: carrier products by the 64-bit mad, no I / Q low cascades, k_decode's
float stages.  tests/signal_cases.py cannot reach it (hand-made signals keep the any-signal bound), so here the signal is the encoder's
own and the amplitude is steered by three knobs: the ENCODER hue rotates the burst, hence (dci, dcq), against the 4-bit monitor-hue
terms (huesn, huecs), and the saturation scales the result -- amplitude = X * |saturation| with X = max(|x0|, |x1|) over the lines.
search() sweeps encoder hue x monitor hue x saturation with the integer model of the ccf recurrence (signal_cases) on the oracle's own
inp[], and TUPLES holds what it found as literals; tests/test_envelope_cpu.py proves every claim on the oracle's trace and re-derives a
row, tests/test_gpu_envelope.py runs the cases on the GPU.

B NEVER FALLS TO 65 532.  The noise stage clamps to -127 .. 127 (crt_core.c:363-364), so the widest range crt_setup_signal_range can
report for a system it knows is 254 wide and B's floor is 32765 * 512 / 254 = 66 045 (65 786 for the full range -128 .. 127 it reports
beyond |noise| 2^20 and for the rand() VHS builds).  FLOOR_NOISE is the smallest noise at which B sits on that floor."""
import numpy as np

import crtref as R
import encoder_cases as E
import signal_cases as S

OUTW, OUTH, OUTFMT = 64, 48, R.FMT_BGRA
LOSKIP_WAVE_MAX, T0_WAVE_MAX = 65532, 120000
B_FLOOR = 66045
SYSTEMS = ("ntsc", "ntscp0", "snes", "nes", "vhslcg")
STEPS = 2
SAT_MAX = 40


def oracle(name):
    return S.oracle(name)


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds: crt_setup_signal_range and crt_setup_loskip_bound, restated
# ---------------------------------------------------------------------------------------------------------------------------
_NES_ACTIVE = (0o300, 0o100, 0o500, 0o400, 0o600, 0o200)
_NES_IRE = (-12042, 0, 34406, 81427, -17203, -8028, 19497, 57342, 43581, 75693, 112965, 112965, 26951, 52181, 83721, 83721)


def _nes_level(p, phase):
    """composite level of PPU pixel p at a phase of the 12-step colour clock"""
    hue = p & 15
    if hue >= 14:
        return 0
    high = 1 if hue == 0 else 0 if hue == 13 else int((hue + phase) % 12 < 6)
    emph = int((p & 0o700 & _NES_ACTIVE[(phase >> 1) % 6]) != 0)
    return _NES_IRE[(high << 3) + (emph << 2) + ((p >> 4) & 3)]


def _s8(v):
    v &= 255
    return v - 256 if v > 127 else v


_NES_RANGE = {}


def _nes_video_range(sd, black_point, white_point):
    """smallest and largest active sample over the 512 PPU pixels x 12 phases (four consecutive levels per sample)"""
    key = (sd.black_level, black_point, white_point)
    if key not in _NES_RANGE:
        lev = [[_nes_level(p, ph) for ph in range(15)] for p in range(512)]
        vals = [_s8(S.c_div((sd.black_level + black_point + sum(lev[p][ph:ph + 4])) * white_point, 100) >> 12)
                for p in range(512) for ph in range(12)]
        _NES_RANGE[key] = (min(vals), max(vals))
    return _NES_RANGE[key]


def _burst_range(name, enc_hue):
    """smallest and largest burst sample the encoder writes: (blank + carrier * burst level) >> 5, carrier = sin >> 10"""
    orc = oracle(name)
    sd = orc.sys
    vals = [sd.blank_level >> 5]
    for r in range(3):
        for k in range(sd.cc_samples):
            if E.is_nes(name):
                ang = (enc_hue + k * 90 + r * 120 + 33) % 360
            else:
                ang = r * sd.vert_step + k * (360 // sd.cc_samples) + enc_hue + sd.burst_off
            vals.append(_s8((sd.blank_level + (orc.sincos14(S.c_div(ang * 8192, 180))[0] >> 10) * sd.burst_level) >> 5))
    return min(vals), max(vals)


def signal_range(name, noise, enc_hue=0, black_point=0, white_point=100):
    """[lo, hi] of every byte of a fused field's inp[]: sync tip, blanking, burst, active video, plus the noise term"""
    sd = oracle(name).sys
    if name in E.RAND_BUILDS or abs(noise) > 1 << 20:
        return -128, 127
    lo, hi = _burst_range(name, enc_hue)
    lo, hi = min(lo, 0, sd.sync_level), max(hi, 0, sd.blank_level)
    if E.is_nes(name):
        v = _nes_video_range(sd, black_point, white_point)
        lo, hi = min(lo, v[0]), max(hi, v[1])
    else:
        hi = max(hi, 110)
    t = ((-127 * noise) >> 8, (128 * noise) >> 8)
    return max(lo + min(t), -127), min(hi + max(t), 127)


def loskip_bound(lo, hi):
    """largest |wave| at which u = (s * wave) >> 9, s in [lo, hi], keeps max|u| <= 32766 and the hull's width <= 32765; the width
    term is the one that decides for every range that holds both signs"""
    lo, hi = min(lo, 0), max(hi, 0)
    m, wd = max(-lo, hi), hi - lo
    if m <= 0 or wd <= 0:
        return LOSKIP_WAVE_MAX
    return min(max(min(32766 * 512 // m, 32765 * 512 // wd), LOSKIP_WAVE_MAX), T0_WAVE_MAX)


def bound(name, noise, **kw):
    return loskip_bound(*signal_range(name, noise, **kw))


def floor_noise(name):
    """the smallest noise >= 0 at which B has fallen to its floor (66 045: the clamped range -127 .. 127)"""
    return next(nz for nz in range(1, 1 << 12) if bound(name, nz) == B_FLOOR)


FLOOR_NOISE = {"ntsc": 174, "ntscp0": 174, "snes": 174, "nes": 180, "vhslcg": 174}     # floor_noise(); asserted by the CPU test
NEGATIVE_NOISE = -24
# B as literals, by noise (0, 24, 60, the negative one, one below the floor's noise, the floor's noise): the CPU test requires
# restatement == literal == crthip_knobs_prepare's env.loskip_wave_max.  The four RGB systems share one signal range.
_RGB_BOUNDS = {0: 111837, 24: 96411, 60: 85155, -24: 96969, 173: 66307, 174: 66045}
BOUNDS = {name: dict(_RGB_BOUNDS) for name in ("ntsc", "ntscp0", "snes", "vhslcg")}
BOUNDS["nes"] = {0: 114120, 24: 98103, 60: 86472, -24: 98680, 179: 66307, 180: 66045}      # from the 512 x 12 table: -37 .. 110


# ---------------------------------------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("phase", "runs", "random")


def image(name, family, k):
    if E.is_nes(name):
        return E.ppu_ramp(256, 16) if family != "random" else R.synth_ppu(256, 16, 8600 + k)
    if family == "phase":
        return E.lay(E.phase_image(name), OUTFMT)
    if family == "runs":
        return E.lay(E.runs_image(E.destw(name), 48, k & 3, k & 3), OUTFMT)
    return E.lay(R.synth_image(64, 48, 3, 8600 + k), OUTFMT)


# ---------------------------------------------------------------------------------------------------------------------------
# running a tuple: n fields from lock, both field parities, two passes, every pass from a clean analog[]
# ---------------------------------------------------------------------------------------------------------------------------
def _case_like(name, enc_hue):
    return dict(name=name, hue=enc_hue, fmt=OUTFMT, raw=0, xoffset=0)


def run_fields(lib, name, imgs, noise, enc_hue, mon_hue, sat, starts=None, geom=(OUTW, OUTH, OUTFMT), knobs=None):
    """`lib` = the Oracle or the real reference.  -> [field][pass] dict; on the oracle with the trace, and `undefined` from the pass
    on in which the reference's reads leave inp[] + 16 (crtref.reads_past_inp)."""
    is_orc = isinstance(lib, R.Oracle)
    like = _case_like(name, enc_hue)
    res = []
    for k, img in enumerate(imgs):
        c = lib.new_crt(*geom)
        c.set("hue", mon_hue)
        c.set("saturation", sat)
        for kk, v in (knobs or {}).items():
            c.set(kk, v)
        hs, vs = starts[k] if starts else (0, 0)
        c.set("hsync", hs)
        c.set("vsync", vs)
        pad = np.concatenate([img, img[-1:]])
        per, undefined = [], False
        for step in range(STEPS):
            c.settings(pad, w=int(img.shape[1]), h=int(img.shape[0]), **E.settings_kw(like, k, step))
            if E.is_progressive(name):
                c.sset("field_initialized", 0)
            c.analog[:] = 0
            c.modulate()
            analog, ccf_mod = np.array(c.analog).copy(), np.array(c.ccf).copy()
            hs_before = c.get("hsync")
            trace = None
            if is_orc:
                c.demodulate(noise, trace=True)
                trace = c.trace.copy()
                undefined = undefined or R.reads_past_inp(lib, trace, c.get("vsync"), hs_before)
            else:
                c.demodulate(noise)
            per.append(dict(analog=analog, ccf_mod=ccf_mod, inp=np.array(c.inp).copy(), rn=c.get("rn"), hsync=c.get("hsync"),
                            vsync=c.get("vsync"), ccf=np.array(c.ccf).copy(), out=c.out.copy(), trace=trace, undefined=undefined))
        res.append(per)
    return res


def amplitudes(trace):
    """per decoded line of an oracle trace: max(|wave0|, |wave1|) (4 samples per chroma cycle: what line_tier_flags compares)"""
    tr = trace[trace[:, 0] == 1]
    return np.maximum(np.abs(tr[:, 2].astype(np.int64)), np.abs(tr[:, 3].astype(np.int64)))


# ---------------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------------
def _dc_lines(name, res):
    """(dci, dcq) of every decoded line of every field and pass, by the integer model of the ccf recurrence on the oracle's inp[];
    every pass starts from the ccf the encoder presets (crt_modulate writes it, the VHS build zeros)"""
    sd = oracle(name).sys
    out = []
    for per in res:
        for r in per:
            ccf = [[int(v) for v in row] for row in r["ccf_mod"]]
            flat = np.concatenate([r["inp"].astype(np.int64), np.zeros(2 * sd.hres, dtype=np.int64)])
            for idx, ln, vln, hs, pos in S.line_geometry(name, r["trace"], r["vsync"]):
                ccr = ccf[vln % sd.cc_vper]
                for at, k in S.burst_positions(sd, ln, hs):
                    ccr[k] = S.ccf_step(ccr[k], int(flat[at]))
                a = hs % 4
                out.append((ccr[(a + 1) & 3] - ccr[(a + 3) & 3], ccr[(a + 2) & 3] - ccr[a & 3]))
    return np.array(out, dtype=np.int64)


def mon_hue_terms(name):
    """{(huesn, huecs): the first monitor hue 0 .. 359 that gives the pair}"""
    terms = {}
    for hue in range(360):
        terms.setdefault(S.hue_terms(oracle(name), hue), hue)
    return terms


def search(name, noise, bounds, n=2, enc_hues=range(360), family="random"):
    """-> {bound: {(side, sign of saturation): (distance, encoder hue, monitor hue, saturation, amplitude)}}: per bound the tuples
    whose largest line amplitude over n fields and two passes from lock lies nearest the bound, inside (bound - |sat|, bound] for
    side "below" and inside (bound, bound + |sat|] for "above".  The burst does not depend on the picture, so any family's images
    serve.  360 encoder hues take about half a minute."""
    assert oracle(name).sys.cc_samples == 4
    imgs = [image(name, family, k) for k in range(n)]
    terms = mon_hue_terms(name)
    sats = np.arange(1, SAT_MAX + 1)
    best = {b: {} for b in bounds}
    for enc in enc_hues:
        dc = _dc_lines(name, run_fields(oracle(name), name, imgs, noise, enc, 0, 1))
        for (sn, cs), mon in terms.items():
            x = int(max(np.abs((dc[:, 0] * cs - dc[:, 1] * sn) >> 4).max(), np.abs((dc[:, 1] * cs + dc[:, 0] * sn) >> 4).max()))
            amp = x * sats
            for b in bounds:
                for side, ok, dist in (("below", (amp <= b) & (amp > b - sats), b - amp), ("above", (amp > b) & (amp <= b + sats), amp - b)):
                    for i in np.flatnonzero(ok):
                        for sign in (1, -1):
                            cand = (int(dist[i]), enc, mon, sign * int(sats[i]), int(amp[i]))
                            if (side, sign) not in best[b] or cand < best[b][(side, sign)]:
                                best[b][(side, sign)] = cand
    return best


# ---------------------------------------------------------------------------------------------------------------------------
# what search() found (n = 2, two passes from lock), as literals: (system, noise, bound name, side) -> (encoder hue, monitor hue,
# saturation, largest line amplitude).  bound name "lo" = 65 532, "B" = B(noise, system), "t0" = 120 000.  Distances are in
# DISTANCE below; every one is inside one |saturation|, ntsc has all six rows at noise 0 and at noise 24.  Not reachable on the grid of
# 360 x 360 hues x |saturation| <= 40 (no tuple inside the quantum): snes at noise 0 on either side of B and just above 65 532, nes
# at noise 0 just above B and just below 65 532 -- the encoder presets the ccf to the burst's steady state, so a field's amplitude
# hardly moves and X takes few values.  The other systems hold the sides these two miss.
# ---------------------------------------------------------------------------------------------------------------------------
TUPLES = {
    ("ntsc", 0, "lo", "below"): (3, 29, 15, 65520),
    ("ntsc", 0, "lo", "above"): (3, 57, -16, 65536),
    ("ntsc", 0, "B", "below"): (2, 137, -29, 111824),
    ("ntsc", 0, "B", "above"): (3, 137, 30, 111840),
    ("ntsc", 0, "t0", "below"): (2, 78, 25, 120000),
    ("ntsc", 0, "t0", "above"): (2, 348, -26, 120016),
    ("ntsc", 24, "lo", "below"): (122, 217, -12, 65532),
    ("ntsc", 24, "lo", "above"): (90, 194, 13, 65533),
    ("ntsc", 24, "B", "below"): (3, 113, 21, 96411),
    ("ntsc", 24, "B", "above"): (59, 356, -23, 96416),
    ("ntsc", 24, "t0", "below"): (0, 2, -24, 120000),
    ("ntsc", 24, "t0", "above"): (21, 348, 31, 120001),
    ("ntscp0", -24, "lo", "above"): (37, 230, -13, 65533),
    ("ntscp0", -24, "B", "below"): (25, 266, 23, 96968),
    ("ntscp0", -24, "B", "above"): (4, 39, -25, 96975),
    ("snes", 0, "lo", "below"): (1, 54, 14, 65520),
    ("snes", 0, "t0", "below"): (0, 39, -25, 120000),
    ("nes", 0, "lo", "above"): (0, 22, 9, 65538),
    ("nes", 0, "B", "below"): (13, 227, -15, 114120),
    ("vhslcg", 60, "lo", "above"): (0, 292, 13, 65533),
    ("vhslcg", 60, "B", "below"): (50, 273, -21, 85155),
    ("vhslcg", 60, "B", "above"): (0, 65, 18, 85158),
}
N_FIELDS = 2


def bound_value(name, noise, which):
    return {"lo": LOSKIP_WAVE_MAX, "B": BOUNDS[name][noise], "t0": T0_WAVE_MAX}[which]


DISTANCE = {key: abs(t[3] - bound_value(key[0], key[1], key[2])) for key, t in TUPLES.items()}

# ntsc at noise 0 runs every tuple on all three image families (phase rows, runs of opposite cube corners, the random control); the
# other rows take one family each, in rotation
CASES = {}
for _i, (_key, _t) in enumerate(TUPLES.items()):
    for _fam in (FAMILIES if _key[:2] == ("ntsc", 0) else (FAMILIES[_i % 3],)):
        CASES["%s-noise%d-%s-%s-%s" % (_key + (_fam,))] = dict(name=_key[0], noise=_key[1], bound=_key[2], side=_key[3], enc_hue=_t[0],
                                                             mon_hue=_t[1], sat=_t[2], amp=_t[3], family=_fam, n=N_FIELDS)


# Fused start states: hsync / vsync written into the state before the first call, chosen on the oracle's trace.  From hsync 140 the
# hsync search meets no pulse and walks 8 samples per line until it finds lock again; on the way the decoded windows of field 0 run
# over the line's end into the next line's sync tip, so single windows hold -40 beside white video (110); from (100, 100) the vsync
# search moves as well.  No field-pass of these cases drops out through reads_past_inp (recorded count 0).  (The other start state one
# could wish for -- the field's last line reading the mirrored tail with an amplitude inside (65 532, B] -- is reached from lock: the
# "B-below" cases.)
START_CASES = {
    "ntsc-noise0-B-above-phase-start140": ("ntsc-noise0-B-above-phase", [(140, 0), (140, 0)]),
    "ntsc-noise0-lo-above-phase-start400": ("ntsc-noise0-lo-above-phase", [(400, 0), (100, 100)]),
}
for _cid, (_base, _starts) in START_CASES.items():
    CASES[_cid] = dict(CASES[_base], side="start", starts=_starts)


# sequence and stills carry the sync state from field to field and from pass to pass, so the tuples above (two passes from 0, 0) do
# not keep their amplitude there; these two were searched on the oracle for "every field / every pass holds tier-1 lines AND lines above
# B": (noise, family, encoder hue, monitor hue, saturation), asserted on the trace by the GPU tests' oracle halves
SEQUENCE_TUPLE = (24, "phase", 0, 0, 22)
STILLS_TUPLE = (0, "runs", 0, 47, 33)


def case_bound(cid):
    c = CASES[cid]
    return bound_value(c["name"], c["noise"], c["bound"])


_IMAGES, _WANT = {}, {}


def images(cid):
    """the case's n images in the pixel format, [n, h, w, 4] uint8 (NES: [n, h, w] uint16); built once"""
    if cid not in _IMAGES:
        c = CASES[cid]
        _IMAGES[cid] = np.stack([image(c["name"], c["family"], k) for k in range(c["n"])])
    return _IMAGES[cid]


def run_case(lib, cid, geom=(OUTW, OUTH, OUTFMT), knobs=None):
    c = CASES[cid]
    return run_fields(lib, c["name"], list(images(cid)), c["noise"], c["enc_hue"], c["mon_hue"], c["sat"], starts=c.get("starts"), geom=geom,
                      knobs=knobs)


def expected(cid, geom=(OUTW, OUTH, OUTFMT), scanlines=0):
    """the oracle's results of a case, [field][pass]; computed once per output geometry and left alone"""
    key = (cid, geom, scanlines)
    if key not in _WANT:
        _WANT[key] = run_case(oracle(CASES[cid]["name"]), cid, geom, dict(scanlines=scanlines) if scanlines else None)
    return _WANT[key]


# ---------------------------------------------------------------------------------------------------------------------------
# a model of line_tier_flags (crt_dev.h) and the census of a case's lines
# ---------------------------------------------------------------------------------------------------------------------------
CLASSES = ("tier0", "tier1", "keeplo", "not64")


def line_class(wave0, wave1, loskip_wave_max, reads_tail):
    """tier0: neither flag; tier1: WIDE without KEEPLO; keeplo: above the no-low-cascade bound (a line that reads the mirrored tail
    keeps the any-signal bound); not64: above 120 000"""
    if reads_tail:
        loskip_wave_max = min(loskip_wave_max, LOSKIP_WAVE_MAX)
    a = max(abs(int(wave0)), abs(int(wave1)))
    if a > T0_WAVE_MAX:
        return "not64"
    if a > loskip_wave_max:
        return "keeplo"
    return "tier1" if a > LOSKIP_WAVE_MAX else "tier0"


def census(cid):
    """lines per class over the case's fields and passes, and how many of them read the mirrored tail"""
    c = CASES[cid]
    sd = oracle(c["name"]).sys
    b = BOUNDS[c["name"]][c["noise"]]
    count = dict.fromkeys(CLASSES, 0)
    for per in expected(cid):
        for r in per:
            for row in r["trace"][r["trace"][:, 0] == 1]:
                count[line_class(row[2], row[3], b, int(row[1]) + sd.av_len + 8 > sd.input_size)] += 1
    return tuple(count[k] for k in CLASSES)


def spanning_windows(cid, lo_byte, hi_byte, margin=8):
    """per field and pass: how many decoded windows (pos - margin .. pos + AV_LEN + margin) hold BOTH bytes, and the classes of those
    lines"""
    c = CASES[cid]
    sd = oracle(c["name"]).sys
    b = BOUNDS[c["name"]][c["noise"]]
    res = []
    for per in expected(cid):
        for r in per:
            n, classes = 0, set()
            for row in r["trace"][r["trace"][:, 0] == 1]:
                w = r["inp"][max(int(row[1]) - margin, 0):int(row[1]) + sd.av_len + margin]
                if (w == lo_byte).any() and (w == hi_byte).any():
                    n += 1
                    classes.add(line_class(row[2], row[3], b, int(row[1]) + sd.av_len + 8 > sd.input_size))
            res.append((n, tuple(sorted(classes))))
    return res


def window_bytes(cid):
    """smallest and largest inp[] byte over the decoded windows (pos - 8 .. pos + AV_LEN + 8, inside the field) of the case"""
    sd = oracle(CASES[cid]["name"]).sys
    lo, hi = 127, -128
    for per in expected(cid):
        for r in per:
            for row in r["trace"][r["trace"][:, 0] == 1]:
                w = r["inp"][max(int(row[1]) - 8, 0):int(row[1]) + sd.av_len + 8]
                lo, hi = min(lo, int(w.min())), max(hi, int(w.max()))
    return lo, hi


# ---------------------------------------------------------------------------------------------------------------------------
# recorded per case, asserted exactly by the CPU test: the census (tier0, tier1, keeplo, not64) over 2 fields x 2 passes x 240 lines
# under B(noise, system); the smallest and largest inp[] byte over the decoded windows; its distance to either end of the restated
# signal range.  The 4 KEEPLO lines of the "B-below" cases are the fields' last lines: they read the mirrored tail with an amplitude
# inside (65 532, B], the reads_tail clause of line_tier_flags, reached from lock.
# ---------------------------------------------------------------------------------------------------------------------------
RECORDED = {
    "ntsc-noise0-lo-below-phase": dict(census=(960, 0, 0, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-lo-below-runs": dict(census=(960, 0, 0, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-lo-below-random": dict(census=(960, 0, 0, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-lo-above-phase": dict(census=(486, 472, 2, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-lo-above-runs": dict(census=(486, 472, 2, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-lo-above-random": dict(census=(486, 472, 2, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-B-below-phase": dict(census=(0, 956, 4, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-B-below-runs": dict(census=(0, 956, 4, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-B-below-random": dict(census=(0, 956, 4, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-B-above-phase": dict(census=(0, 484, 476, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-B-above-runs": dict(census=(0, 484, 476, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-B-above-random": dict(census=(0, 484, 476, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-t0-below-phase": dict(census=(0, 42, 918, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-t0-below-runs": dict(census=(0, 42, 918, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-t0-below-random": dict(census=(0, 42, 918, 0), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-t0-above-phase": dict(census=(0, 42, 444, 474), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-t0-above-runs": dict(census=(0, 42, 444, 474), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise0-t0-above-random": dict(census=(0, 42, 444, 474), window=(-40, 110), slack=(0, 0)),
    "ntsc-noise24-lo-below-phase": dict(census=(960, 0, 0, 0), window=(-52, 122), slack=(0, 0)),
    "ntsc-noise24-lo-above-runs": dict(census=(959, 1, 0, 0), window=(-52, 122), slack=(0, 0)),
    "ntsc-noise24-B-below-random": dict(census=(0, 956, 4, 0), window=(-52, 122), slack=(0, 0)),
    "ntsc-noise24-B-above-phase": dict(census=(0, 955, 5, 0), window=(-52, 122), slack=(0, 0)),
    "ntsc-noise24-t0-below-runs": dict(census=(0, 7, 953, 0), window=(-52, 122), slack=(0, 0)),
    "ntsc-noise24-t0-above-random": dict(census=(0, 7, 952, 1), window=(-52, 122), slack=(0, 0)),
    "ntscp0-noise-24-lo-above-phase": dict(census=(958, 2, 0, 0), window=(-52, 121), slack=(0, 0)),
    "ntscp0-noise-24-B-below-runs": dict(census=(2, 954, 4, 0), window=(-52, 121), slack=(0, 0)),
    "ntscp0-noise-24-B-above-random": dict(census=(2, 952, 6, 0), window=(-52, 121), slack=(0, 0)),
    "snes-noise0-lo-below-phase": dict(census=(960, 0, 0, 0), window=(0, 110), slack=(40, 0)),
    "snes-noise0-t0-below-runs": dict(census=(0, 320, 640, 0), window=(0, 110), slack=(40, 0)),
    "nes-noise0-lo-above-random": dict(census=(696, 264, 0, 0), window=(-17, 110), slack=(20, 0)),
    "nes-noise0-B-below-phase": dict(census=(0, 960, 0, 0), window=(-17, 110), slack=(20, 0)),
    "vhslcg-noise60-lo-above-runs": dict(census=(959, 1, 0, 0), window=(-70, 127), slack=(0, 0)),
    "vhslcg-noise60-B-below-random": dict(census=(128, 828, 4, 0), window=(-70, 127), slack=(0, 0)),
    "vhslcg-noise60-B-above-phase": dict(census=(120, 835, 5, 0), window=(-70, 127), slack=(0, 0)),
    # start-state cases: also the fields-passes excluded through reads_past_inp, and per field-pass (field 0 pass 0, 1; field 1 pass
    # 0, 1) the number of decoded windows that hold -40 AND 110 with the classes of their lines
    "ntsc-noise0-B-above-phase-start140": dict(census=(196, 760, 4, 0), window=(-40, 110), slack=(0, 0), excluded=0,
                                               spanning=[(10, ("tier0", "tier1")), (0, ()), (0, ()), (0, ())]),
    "ntsc-noise0-lo-above-phase-start400": dict(census=(833, 126, 1, 0), window=(-40, 110), slack=(0, 0), excluded=0,
                                                spanning=[(10, ("tier0",)), (0, ()), (0, ()), (0, ())]),
}

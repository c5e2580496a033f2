"""Timings of profiles/stills_knobs_timing.txt (python tools/time_stills_knobs.py MODE [NOISE] [N]; CRTHIP_LIBDIR = another build of
the library, e.g. the parent commit's, for the interleaved A/B of the unchanged paths; NTSC 640x480 -> 640x480 BGRA, blend 1,
scanlines 1, the interlaced CLI schedule, N = 4096 stills by default):
  uniform NOISE   one process: the median of crthip_stills at that noise
  fpknobs         one process: the median of the (n, 8) crthip_fieldpass_knobs call (4096 distinct looks, noise 0 .. 48)
  knobs NOISE     crthip_stills_knobs with 4096 distinct (n, 8) looks, every still at that noise, against crthip_stills at the same
                  noise: three interleaved rounds in one process, and the launch counts of crthip_profile_read
  sweep NOISE     ONE image under 4096 looks (image_stride 0) against 4096 copies of the image
  loop            the loop of batch-1 crthip_stills calls the knob call replaces, on 64 looks (every call another look)"""
import os, sys, time, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ntsc-crt_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import crtlib

mode = sys.argv[1]
noise = int(sys.argv[2]) if len(sys.argv) > 2 else 24
n = int(sys.argv[3]) if len(sys.argv) > 3 else (1 if mode == "loop" else 4096)
w, h = 640, 480
LIB = os.environ.get("CRTHIP_LIBDIR", "this")
torch.manual_seed(1)
imgs = torch.randint(0, 256, (min(n, 64), h + 1, w, 4), dtype=torch.uint8, device="cuda:0")
full = imgs.repeat((n + imgs.shape[0] - 1) // imgs.shape[0], 1, 1, 1)[:n]
g = crtlib.CRT(n, w, h, crtlib.FMT_BGRA, "ntsc", device=0)
g.blend = g.scanlines = 1
g.reserve(n)
g.stills_reserve(4)
s = crtlib.Settings(full[:, :h], format=crtlib.FMT_BGRA, as_color=1)


def power_on():
    g.out.zero_()
    g.state.zero_()
    g.state[:, crtlib.ST_RN] = 194


def timed(fn, reps, warm=3):
    ts = []
    for r in range(warm + reps):
        power_on()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record(); b.synchronize()
        if r >= warm:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def looks(count, nz=None):
    """count distinct (n, 8) looks inside tier 0 and the encoder's fast path; nz: every still at that noise"""
    k = np.arange(count)
    rows = np.stack([k % 49, (k * 7) % 801 - 400, 8 + k % 5, k % 81 - 40, 120 + (k * 5) % 121, k % 61 - 30, 60 + (k * 5) % 81, k - count // 2], axis=1)
    if nz is not None:
        rows[:, 0] = nz
    assert len({tuple(r) for r in rows.tolist()}) == count
    return rows


def counts(fn):
    power_on()
    g.profile(True)
    fn()
    c = g.profile_read()
    g.profile(False)
    return c["active"][1], c["decode"][1]


if mode == "uniform":
    med, lo, hi = timed(lambda: g.stills(s, noise), 15)
    print("UNIFORM_STILLS lib=%s n=%d noise=%d median_ms=%.4f min=%.4f max=%.4f stills_per_s=%.0f" % (LIB, n, noise, med, lo, hi, n / med * 1e3))
elif mode == "fpknobs":
    p = g.params(s, 0)
    g._load_field_state(s)
    g.upload_knobs(looks(n), p)
    med, lo, hi = timed(lambda: g.fieldpass_knobs(s, None, params=p), 40, warm=5)
    print("FIELDPASS_KNOBS8 lib=%s n=%d median_ms=%.4f min=%.4f max=%.4f fields_per_s=%.0f" % (LIB, n, med, lo, hi, n / med * 1e3))
elif mode == "knobs":
    p = g.params(s, 0)
    g.upload_knobs(looks(n, noise), p)
    fk = lambda: g.stills_knobs(s, None, params=p)
    fu = lambda: g.stills(s, noise)
    for rnd in range(3):
        mu = timed(fu, 10); mk = timed(fk, 10)
        print("ROUND %d noise=%d uniform median_ms=%.4f (min %.4f max %.4f) knobs median_ms=%.4f (min %.4f max %.4f) ratio=%.4f stills_per_s=%.0f"
              % ((rnd, noise) + mu + mk + (mk[0] / mu[0], n / mk[0] * 1e3)))
    g._load_field_state(s)
    a1, d1 = counts(lambda: g.fieldpass_knobs(s, None, params=p))
    ak, dk = counts(fk)
    au, du = counts(fu)
    print("LAUNCHES noise=%d fieldpass_knobs active=%d decode=%d | stills_knobs active=%d (%.0fx) decode=%d (%.0fx) | stills active=%d decode=%d"
          % (noise, a1, d1, ak, ak / a1, dk, dk / d1, au, du))
elif mode == "sweep":
    p = g.params(s, 0)
    g.upload_knobs(looks(n, noise), p)
    one = crtlib.Settings(full[:1, :h].expand(n, h, w, 4), format=crtlib.FMT_BGRA, as_color=1)
    many = crtlib.Settings(full[:1].repeat(n, 1, 1, 1)[:, :h], format=crtlib.FMT_BGRA, as_color=1)
    assert g._image_stride(one) == 0 and g._has_spare_row(one) and g._has_spare_row(many)
    for rnd in range(3):
        mm = timed(lambda: g.stills_knobs(many, None, params=p), 10); mo = timed(lambda: g.stills_knobs(one, None, params=p), 10)
        print("ROUND %d noise=%d copies median_ms=%.4f (min %.4f max %.4f) one_image median_ms=%.4f (min %.4f max %.4f) ratio=%.4f"
              % ((rnd, noise) + mm + mo + (mo[0] / mm[0],)))
elif mode == "loop":
    rows = looks(64)

    def loop():
        for r in rows:
            g.hue, g.saturation, g.brightness, g.contrast, g.black_point, g.white_point = (int(v) for v in r[1:7])
            s.hue = int(r[7])
            power_on()
            g.stills(s, int(r[0]))
    loop(); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t = time.perf_counter(); loop(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    med = statistics.median(ts)
    print("LOOP batch=%d looks=%d median_s=%.4f stills_per_s=%.0f extrapolated_s_for_4096=%.2f" % (n, len(rows), med, len(rows) * n / med, med * 4096 / len(rows)))
g.close()

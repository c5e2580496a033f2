"""Timings of profiles/hues_timing.txt (python tools/time_hues.py MODE [N]; CRTHIP_LIBDIR = another build of the library, e.g. the
parent commit's, for the interleaved A/B of the unchanged paths; NTSC 640x480, N = 4096 fields by default):
  uniform   one process: the median of crthip_fieldpass
  three     one process: the median of the (n, 3) knob call (4096 distinct (noise, hue) pairs, saturation 10)
  five      one process: the median of the (n, 5) knob call (the same, 4096 distinct (brightness, contrast) pairs inside tier 0)
  seven     one process: the median of the (n, 7) knob call (the same, 4096 distinct (black_point, white_point) pairs)
  eight     (n, 8) with 4096 distinct encoder hues against (n, 7) with the same other knobs, whole call and per kernel
  loop      the loop of batch-1 crthip_fieldpass calls the hue call replaces (N = 1; the encoder hue changes every call), in fields/s"""
import os, sys, time, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ntsc-crt_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import crtlib

mode = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
w, h = 640, 480
torch.manual_seed(1)
imgs = torch.randint(0, 256, (min(n, 64), h + 1, w, 4), dtype=torch.uint8, device="cuda:0")
data = imgs.repeat((n + imgs.shape[0] - 1) // imgs.shape[0], 1, 1, 1)[:n, :h]
g = crtlib.CRT(n, w, h, crtlib.FMT_BGRA, "ntsc", device=0)
g.scanlines = 1
g.reserve(n)
s = crtlib.Settings(data, format=crtlib.FMT_BGRA, as_color=1, field=[k & 1 for k in range(n)], frame=0)
p = g.params(s, 24)
g._load_field_state(s)
LIB = os.environ.get("CRTHIP_LIBDIR", "this")


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def seven_rows():
    k = np.arange(n)
    return np.stack([k % 49, (k * 7) % 801 - 400, np.full(n, 10), k % 81 - 40, 120 + (k * 5) % 121, k % 61 - 30, 60 + (k * 5) % 81], axis=1)


def per_kernel(calls):
    """{tag: {kernel: ms per launch}} with the library's own event pairs; every call twice, interleaved"""
    g.profile(True)
    res = {}
    for rnd in range(2):
        for tag, fn in calls:
            for _ in range(3):
                fn()
            g.profile_read()
            for _ in range(20):
                fn()
            res[tag + str(rnd)] = {k: m / max(c, 1) for k, (m, c) in g.profile_read().items()}
    g.profile(False)
    return res


if mode == "uniform":
    med, lo, hi = timed(lambda: g.fieldpass(s, 24, params=p), 40)
    print("UNIFORM lib=%s n=%d median_ms=%.4f min=%.4f max=%.4f fields_per_s=%.0f" % (LIB, n, med, lo, hi, n / med * 1e3))
elif mode in ("three", "five", "seven"):
    rows = seven_rows()
    g.upload_knobs(rows[:, :{"three": 3, "five": 5, "seven": 7}[mode]], p)
    med, lo, hi = timed(lambda: g.fieldpass_knobs(s, None, params=p), 40)
    print("%s lib=%s n=%d median_ms=%.4f min=%.4f max=%.4f fields_per_s=%.0f" % (mode.upper(), LIB, n, med, lo, hi, n / med * 1e3))
elif mode == "eight":
    seven = seven_rows()
    eight = np.concatenate([seven, (np.arange(n) - n // 2)[:, None]], axis=1)      # n distinct hues, both signs, beyond a turn
    assert len(set(eight[:, 7].tolist())) == n
    r7, l7, e7, le7 = crtlib.knobs_prepare7(p, seven)
    r8, l8, h8, e8, le8, he8 = crtlib.knobs_prepare8(p, eight)
    dev = lambda a: torch.from_numpy(a).to("cuda:0")
    sets = [(dev(r7), dev(l7), None, e7, le7, None), (dev(r8), dev(l8), dev(h8), e8, le8, he8)]
    vp, ref = crtlib.C.c_void_p, crtlib.C.byref

    def call(i):
        recs, levs, hues, env, lenv, henv = sets[i]

        def fn():
            g.knob_recs, g._knob_env = recs, env
            g._check(g.L.crthip_bind_levels(g.ctx, vp(levs.data_ptr()), ref(lenv)), "crthip_bind_levels")
            if hues is not None:
                g._check(g.L.crthip_bind_hues(g.ctx, vp(hues.data_ptr()), ref(henv)), "crthip_bind_hues")
            else:
                g._check(g.L.crthip_bind_hues(g.ctx, None, None), "crthip_bind_hues")
            g.fieldpass_knobs(s, None, params=p)
        return fn
    fa, fb = call(0), call(1)
    for rnd in range(3):
        ma = timed(fa, 30); mb = timed(fb, 30)
        print("ROUND %d seven median_ms=%.4f (min %.4f max %.4f) eight median_ms=%.4f (min %.4f max %.4f) ratio=%.4f"
              % ((rnd,) + ma + mb + (mb[0] / ma[0],)))
    res = per_kernel((("seven", fa), ("eight", fb)))
    for nm in res["seven0"]:
        a0, a1, b0, b1 = (res[t].get(nm, 0.0) for t in ("seven0", "seven1", "eight0", "eight1"))
        if a0 > 0 or b0 > 0:
            print("KERNEL %-10s seven %.4f / %.4f ms  eight %.4f / %.4f ms  ratio %.4f" % (nm, a0, a1, b0, b1, (b0 + b1) / max(a0 + a1, 1e-9)))
elif mode == "loop":
    reps = 512
    ps = []
    for k in range(8):
        s.hue = 45 * k - 160
        ps.append(g.params(s, 24))

    def loop():
        for k in range(reps):
            g.fieldpass(s, 0, params=ps[k & 7])
    loop(); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t = time.perf_counter(); loop(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    med = statistics.median(ts)
    print("LOOP batch=%d calls=%d median_s=%.4f fields_per_s=%.0f" % (n, reps, med, reps * n / med))
g.close()

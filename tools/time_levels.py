"""Timings of profiles/levels_timing.txt (python tools/time_levels.py MODE [N]; CRTHIP_LIBDIR = another build of the library, e.g.
the parent commit's, for the interleaved A/B of the unchanged paths; NTSC 640x480, N = 4096 fields by default):
  uniform   one process: the median of crthip_fieldpass
  three     one process: the median of the (n, 3) knob call (4096 distinct (noise, hue) pairs, saturation 10)
  five      one process: the median of the (n, 5) knob call (the same, 4096 distinct (brightness, contrast) pairs inside tier 0)
  seven     (n, 7) against (n, 5) with the same other knobs, whole call and per kernel: 4096 distinct (black_point, white_point) pairs
            inside the encoder's fast bound (black point -30 .. 30, white point 60 .. 140)
  sixteenth (n, 7) with every 16th field outside the fast bound (white 8192: the whole call on the exact encoder) against all inside
  loop      the loop of batch-1 crthip_fieldpass calls the level call replaces (N = 1), in fields/s"""
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


def five_rows():
    k = np.arange(n)
    return np.stack([k % 49, (k * 7) % 801 - 400, np.full(n, 10), k % 81 - 40, 120 + (k * 5) % 121], axis=1)


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
elif mode in ("three", "five"):
    rows = five_rows()
    g.upload_knobs(rows[:, :3] if mode == "three" else rows, p)
    med, lo, hi = timed(lambda: g.fieldpass_knobs(s, None, params=p), 40)
    print("%s lib=%s n=%d median_ms=%.4f min=%.4f max=%.4f fields_per_s=%.0f" % (mode.upper(), LIB, n, med, lo, hi, n / med * 1e3))
elif mode in ("seven", "sixteenth"):
    five = five_rows()
    k = np.arange(n)
    seven = np.concatenate([five, np.stack([k % 61 - 30, 60 + (k * 5) % 81], axis=1)], axis=1)
    assert len({tuple(r) for r in seven[:, 5:].tolist()}) == min(n, 61 * 81)
    if mode == "sixteenth":
        other = seven.copy()
        other[::16, 6] = 8192                            # WHITE_LEVEL 100: white = 8192, the first value outside the fast bound
        sets = [crtlib.knobs_prepare(p, seven), crtlib.knobs_prepare(p, other)]
        names = ("seven_inside", "seven_one_in_16")
    else:
        # the (n, 5) side at the blob's own levels; the (n, 7) side with a pair of its own per field
        sets = [crtlib.knobs_prepare(p, five), crtlib.knobs_prepare(p, seven)]
        names = ("five", "seven")
    bufs = [torch.from_numpy(r).to("cuda:0") for r, _ in sets]
    levs = [torch.from_numpy(e.levs).to("cuda:0") if hasattr(e, "levs") else None for _, e in sets]

    def call(i):
        def fn():
            g.knob_recs, g._knob_env = bufs[i], sets[i][1]
            if levs[i] is not None:
                g._check(g.L.crthip_bind_levels(g.ctx, crtlib.C.c_void_p(levs[i].data_ptr()), crtlib.C.byref(sets[i][1].lenv)), "crthip_bind_levels")
            else:
                g._check(g.L.crthip_bind_levels(g.ctx, None, None), "crthip_bind_levels")
            g.fieldpass_knobs(s, None, params=p)
        return fn
    fa, fb = call(0), call(1)
    for rnd in range(3):
        ma = timed(fa, 30); mb = timed(fb, 30)
        print("ROUND %d %s median_ms=%.4f (min %.4f max %.4f) %s median_ms=%.4f (min %.4f max %.4f) ratio=%.4f"
              % ((rnd, names[0]) + ma + (names[1],) + mb + (mb[0] / ma[0],)))
    res = per_kernel(((names[0], fa), (names[1], fb)))
    for nm in res[names[0] + "0"]:
        a0, a1, b0, b1 = (res[t][nm] for t in (names[0] + "0", names[0] + "1", names[1] + "0", names[1] + "1"))
        if a0 > 0:
            print("KERNEL %-10s %s %.4f / %.4f ms  %s %.4f / %.4f ms  ratio %.4f" % (nm, names[0], a0, a1, names[1], b0, b1, (b0 + b1) / (a0 + a1)))
elif mode == "loop":
    reps = 512
    ps = []
    for k in range(8):
        g.black_point, g.white_point = k * 5 - 20, 70 + 10 * k
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

"""Timings of profiles/picknobs_timing.txt (python tools/time_picknobs.py MODE [N]; CRTHIP_LIBDIR = another build of the library, e.g.
the parent commit's, for the interleaved A/B of the unchanged paths; NTSC 640x480, N = 4096 fields by default):
  uniform   one process: the median of crthip_fieldpass
  three     one process: the median of the (n, 3) knob call (4096 distinct (noise, hue) pairs, saturation 10)
  five      (n, 5) against (n, 3) with the same other knobs, whole call and per kernel: 4096 distinct (brightness, contrast) pairs inside
            tier 0 (brightness -40 .. 40, contrast 120 .. 240).  CRTHIP_DEC_FLOAT=0 in the environment makes the (n, 3) call run the
            integer stages too: the like-for-like comparison that isolates the per-lane operands
  sixteenth (n, 5) with every 16th field above the contrast bound (contrast 140 000: the 24-bit tier) against all fields inside
  loop      the loop of batch-1 crthip_fieldpass calls the knob call replaces (N = 1), in fields/s"""
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


def triples():
    k = np.arange(n)
    return np.stack([k % 49, (k * 7) % 801 - 400, np.full(n, 10)], axis=1)      # n distinct (noise, hue) pairs, saturation 10


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
elif mode == "three":
    g.upload_knobs(triples(), p)
    med, lo, hi = timed(lambda: g.fieldpass_knobs(s, None, params=p), 40)
    print("THREE lib=%s n=%d median_ms=%.4f min=%.4f max=%.4f fields_per_s=%.0f float_stages=%d" % (LIB, n, med, lo, hi, n / med * 1e3, g.float_stages_used()))
elif mode in ("five", "sixteenth"):
    trip = triples()
    k = np.arange(n)
    five = np.concatenate([trip, np.stack([k % 81 - 40, 120 + (k * 5) % 121], axis=1)], axis=1)
    assert len({tuple(r) for r in five[:, 3:].tolist()}) == n or n > 81 * 121
    recs3, env3 = crtlib.knobs_prepare(p, trip)
    if mode == "sixteenth":
        other = five.copy()
        other[::16, 4] = 140000                          # above the contrast bound: that field's lines take the 24-bit tier
        recs_b, env_b = crtlib.knobs_prepare(p, other)
        recs_a, env_a = crtlib.knobs_prepare(p, five)
        names = ("five_inside", "five_one_in_16")
    else:
        recs_a, env_a = recs3, env3
        recs_b, env_b = crtlib.knobs_prepare(p, five)
        names = ("three", "five")
    bufs = [torch.from_numpy(r).to("cuda:0") for r in (recs_a, recs_b)]
    envs = [env_a, env_b]

    def call(i):
        def fn():
            g.knob_recs, g._knob_env = bufs[i], envs[i]
            g.fieldpass_knobs(s, None, params=p)
        return fn
    fa, fb = call(0), call(1)
    for rnd in range(3):
        ma = timed(fa, 30); fla = g.float_stages_used(); mb = timed(fb, 30); flb = g.float_stages_used()
        print("ROUND %d dec_float_env=%s %s median_ms=%.4f (min %.4f max %.4f, float stages %d) %s median_ms=%.4f (min %.4f max %.4f, float stages %d) ratio=%.4f"
              % ((rnd, os.environ.get("CRTHIP_DEC_FLOAT", "unset"), names[0]) + ma + (fla, names[1]) + mb + (flb, mb[0] / ma[0])))
    res = per_kernel(((names[0], fa), (names[1], fb)))
    for nm in res[names[0] + "0"]:
        a0, a1, b0, b1 = (res[t][nm] for t in (names[0] + "0", names[0] + "1", names[1] + "0", names[1] + "1"))
        if a0 > 0:
            print("KERNEL %-10s %s %.4f / %.4f ms  %s %.4f / %.4f ms  ratio %.4f" % (nm, names[0], a0, a1, names[1], b0, b1, (b0 + b1) / (a0 + a1)))
elif mode == "loop":
    reps = 512
    ps = []
    for k in range(8):
        g.brightness, g.contrast = k * 10 - 40, 120 + 15 * k
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

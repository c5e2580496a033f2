"""Timings of profiles/knobs_timing.txt (python tools/time_knobs.py MODE [N]; CRTHIP_LIBDIR = another build of the library, e.g. the
parent commit's, for the interleaved A/B of the uniform path): mode `uniform` (one process, prints the median of crthip_fieldpass at the headline
configuration), `knobs` / `knobs_sat10` (uniform against knob call, per kernel; saturation 5..15 / 10 throughout), `loop` (batch-1 calls)."""
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


if mode == "uniform":
    med, lo, hi = timed(lambda: g.fieldpass(s, 24, params=p), 40)
    print("UNIFORM lib=%s n=%d median_ms=%.4f min=%.4f max=%.4f fields_per_s=%.0f" % (os.environ.get("CRTHIP_LIBDIR", "this"), n, med, lo, hi, n / med * 1e3))
elif mode in ("knobs", "knobs_sat10"):
    rng = np.random.RandomState(7)
    trip = np.stack([rng.permutation(n) % 49, rng.randint(-400, 401, n), rng.randint(5, 16, n)], axis=1)
    trip[:, 0] = np.arange(n) % 49; trip[:, 1] = (np.arange(n) * 7) % 801 - 400        # 4096 distinct (noise, hue) pairs
    if mode == "knobs_sat10":
        trip[:, 2] = 10            # noise and hue vary, saturation as in the uniform call: the lines stay in the uniform call's decoder tier
    assert len({tuple(r) for r in trip.tolist()}) == n
    g.upload_knobs(trip, p)
    fu = lambda: g.fieldpass(s, 24, params=p)
    fk = lambda: g.fieldpass_knobs(s, None, params=p)
    for rnd in range(3):
        mu = timed(fu, 30); mk = timed(fk, 30)
        print("ROUND %d uniform median_ms=%.4f (min %.4f max %.4f) knobs median_ms=%.4f (min %.4f max %.4f) ratio=%.4f" % ((rnd,) + mu + mk + (mk[0] / mu[0],)))
    g.profile(True)
    res = {}
    for tag, fn in (("uniform", fu), ("knobs", fk), ("uniform2", fu), ("knobs2", fk)):
        for _ in range(3):
            fn()
        g.profile_read()
        for _ in range(20):
            fn()
        res[tag] = {k: m / max(c, 1) for k, (m, c) in g.profile_read().items()}
    g.profile(False)
    for nm in res["uniform"]:
        if res["uniform"][nm] > 0:
            print("KERNEL %-10s uniform %.4f / %.4f ms  knobs %.4f / %.4f ms  ratio %.4f" % (nm, res["uniform"][nm], res["uniform2"][nm], res["knobs"][nm], res["knobs2"][nm],
                  (res["knobs"][nm] + res["knobs2"][nm]) / (res["uniform"][nm] + res["uniform2"][nm])))
elif mode == "loop":
    # the alternative: one call at batch 1 per setting (n here = 1 context of one field, called `reps` times with another noise / hue)
    reps = 512
    ps = []
    for k in range(8):
        g.hue, g.saturation = (k * 37) % 360, 8 + k
        ps.append(g.params(s, 10 + k))
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

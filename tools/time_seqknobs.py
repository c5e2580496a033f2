"""Timings of profiles/seqknobs_timing.txt (python tools/time_seqknobs.py MODE [N] [BLEND]; CRTHIP_LIBDIR = another build of the library,
e.g. the parent commit's, for the interleaved A/B of the uniform path).  NTSC 640x480, N consecutive fields of one set (default 2048;
BLEND = 1: blend on).  Modes:
  uniform     one process, median of crthip_sequence at noise 24 (works with a library that has no knob entry points)
  knobs       crthip_sequence against crthip_sequence_knobs with N distinct (noise, hue) pairs, saturation 10 throughout; per kernel
  knobs_sat   the same with saturations 5..15
  loop        what the knob call replaces: N crthip_fieldpass calls at batch 1, the knobs changed between the calls (default N 256)
  sets        N clips of 16 fields (default 256): crthip_sequence_sets uniform, crthip_sequence_sets_knobs, and a loop of
              crthip_sequence_knobs per clip"""
import ctypes as C
import os, sys, time, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ntsc-crt_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import crtlib

mode = sys.argv[1]
n = int(sys.argv[2]) if len(sys.argv) > 2 else (256 if mode in ("loop", "sets") else 2048)
blend = int(sys.argv[3]) if len(sys.argv) > 3 else 0
w, h = 640, 480
CLIP = 16
torch.manual_seed(1)
imgs = torch.randint(0, 256, (64, h + 1, w, 4), dtype=torch.uint8, device="cuda:0")


def make(count):
    data = imgs.repeat((count + 63) // 64, 1, 1, 1)[:count, :h]
    g = crtlib.CRT(count, w, h, crtlib.FMT_BGRA, "ntsc", device=0)
    g.scanlines = 1
    g.blend = blend
    g.reserve(count)
    s = crtlib.Settings(data, format=crtlib.FMT_BGRA, as_color=1, field=[k & 1 for k in range(count)], frame=[((k + 1) >> 1) & 1 for k in range(count)])
    return g, s


def triples(count, sat_varies):
    k = np.arange(count)
    trip = np.stack([k % 49, (k * 7) % 801 - 400, 5 + (k * 3) % 11 if sat_varies else np.full(count, 10)], axis=1)      # noise 0..48, hue -400..400
    assert len({tuple(r[:2]) for r in trip.tolist()}) == count or count > 49 * 801
    return trip


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)      # (the call synchronises once per sync pass: wall clock)
    return statistics.median(ts), min(ts), max(ts)


def seq_uniform(g, s, p, first=None):
    """crthip_sequence / crthip_sequence_sets with a blob prepared ahead, as the knob wrappers take one (no per-call host work in either)"""
    vp, passes = C.c_void_p, C.c_int(0)
    if first is None:
        rc = g.L.crthip_sequence(g.ctx, C.byref(p), g.n, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()), g.out.stride(0), None,
                                 vp(g.state.data_ptr()), C.byref(passes))
    else:
        rc = g.L.crthip_sequence_sets(g.ctx, C.byref(p), len(first) - 1, (C.c_int * len(first))(*first), vp(s.data.data_ptr()), g._image_stride(s),
                                      vp(g.out.data_ptr()), g.out.stride(0), None, 0, vp(g.state.data_ptr()), C.byref(passes))
    g._check(rc, "crthip_sequence*")
    return passes.value


def reset(g):
    g.state[:, crtlib.ST_HSYNC:crtlib.ST_RN + 1] = torch.tensor([0, 0, 194], dtype=torch.int32, device="cuda:0")


lib = os.environ.get("CRTHIP_LIBDIR", "this")
if mode == "uniform":
    g, s = make(n)
    pu = g.params(s, 24)
    g._load_field_state(s)
    def fu():
        reset(g); return seq_uniform(g, s, pu)
    passes = fu()
    med, lo, hi = timed(fu, 20)
    print("UNIFORM lib=%s n=%d blend=%d passes=%d median_ms=%.4f min=%.4f max=%.4f fields_per_s=%.0f" % (lib, n, blend, passes, med, lo, hi, n / med * 1e3))
elif mode in ("knobs", "knobs_sat"):
    g, s = make(n)
    trip = triples(n, mode == "knobs_sat")
    p, pu = g.params(s, 0), g.params(s, 24)
    g._load_field_state(s)
    g.upload_knobs(trip, p)
    def fu():
        reset(g); return seq_uniform(g, s, pu)
    def fk():
        reset(g); return g.sequence_knobs(s, None, params=p)
    print("PASSES uniform %d knobs %d" % (fu(), fk()))
    for rnd in range(3):
        mu = timed(fu, 15); mk = timed(fk, 15)
        print("ROUND %d uniform median_ms=%.4f (min %.4f max %.4f) knobs median_ms=%.4f (min %.4f max %.4f) ratio=%.4f" % ((rnd,) + mu + mk + (mk[0] / mu[0],)))
    g.profile(True)
    res = {}
    for tag, fn in (("uniform", fu), ("knobs", fk), ("uniform2", fu), ("knobs2", fk)):
        fn()
        g.profile_read()
        for _ in range(5):
            fn()
        res[tag] = {k: (m / 5, c // 5) for k, (m, c) in g.profile_read().items()}
    g.profile(False)
    for nm in res["uniform"]:
        if res["uniform"][nm][0] > 0:
            print("KERNEL %-10s launches/call %d / %d  uniform %.4f / %.4f ms per call  knobs %.4f / %.4f ms per call  ratio %.4f" % (
                  nm, res["uniform"][nm][1], res["knobs"][nm][1], res["uniform"][nm][0], res["uniform2"][nm][0], res["knobs"][nm][0], res["knobs2"][nm][0],
                  (res["knobs"][nm][0] + res["knobs2"][nm][0]) / (res["uniform"][nm][0] + res["uniform2"][nm][0])))
elif mode == "loop":
    # one television set, one crthip_fieldpass at batch 1 per field on the same display, another (noise, hue, saturation) in every call
    g, s = make(1)
    trip = triples(n, True)
    ps = []
    for k in range(n):
        g.hue, g.saturation = int(trip[k, 1]), int(trip[k, 2])
        ps.append(g.params(s, int(trip[k, 0])))
    def loop():
        for k in range(n):
            g.fieldpass(s, 0, params=ps[k])
    loop(); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t = time.perf_counter(); loop(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    print("LOOP batch=1 calls=%d wall_s %s median_s=%.4f fields_per_s=%.0f" % (n, " ".join("%.4f" % t for t in ts), statistics.median(ts), n / statistics.median(ts)))
elif mode == "sets":
    total = n * CLIP
    g, s = make(total)
    s.field = [(k % CLIP) & 1 for k in range(total)]
    s.frame = [(((k % CLIP) + 1) >> 1) & 1 for k in range(total)]
    first = list(range(0, total + 1, CLIP))
    trip = triples(total, True)
    p, pu = g.params(s, 0), g.params(s, 24)
    g._load_field_state(s)
    g.upload_knobs(trip, p)
    def fu():
        reset(g); return seq_uniform(g, s, pu, first)
    def fk():
        reset(g); return g.sequence_sets_knobs(s, None, first, params=p)
    print("PASSES uniform %d knobs %d" % (fu(), fk()))
    for rnd in range(3):
        mu = timed(fu, 10); mk = timed(fk, 10)
        print("ROUND %d sets uniform median_ms=%.4f (min %.4f max %.4f) sets knobs median_ms=%.4f (min %.4f max %.4f) ratio=%.4f fields_per_s=%.0f" % (
              (rnd,) + mu + mk + (mk[0] / mu[0], total / mk[0] * 1e3)))
    # the loop the sets call replaces: one crthip_sequence_knobs per clip on a context of CLIP fields, the clip's records uploaded ahead
    gc, sc = make(CLIP)
    pc = gc.params(sc, 0)
    gc._load_field_state(sc)
    recs = torch.from_numpy(crtlib.knobs_prepare(pc, trip)[0]).to("cuda:0")
    gc.upload_knobs(trip[:CLIP], pc)
    def per_clip():
        for c in range(n):
            gc.knob_recs.copy_(recs[c * CLIP:(c + 1) * CLIP])
            gc._knob_env = crtlib.knobs_prepare(pc, trip[c * CLIP:(c + 1) * CLIP])[1]
            reset(gc)
            sc.data = s.data[c * CLIP:(c + 1) * CLIP]
            gc.sequence_knobs(sc, None, params=pc)
    ml = timed(per_clip, 3, warm=1)
    print("PER-CLIP LOOP clips=%d median_ms=%.4f (min %.4f max %.4f) fields_per_s=%.0f" % (n, ml[0], ml[1], ml[2], total / ml[0] * 1e3))
    gc.close()
g.close()

"""Timings of profiles/sizes_timing.txt (python tools/time_sizes.py MODE [ARG]; CRTHIP_LIBDIR = another build of the library, e.g.
the parent commit's, for the interleaved A/B of the unchanged paths; NTSC -> 640x480 BGRA, noise 24, N = 4096 fields):
  uniform        one process: crthip_fieldpass on 4096 images 640x480, the median and the per-kernel times of crthip_profile_read
  sizes          one process: crthip_fieldpass_sizes on the same 4096 images (4096 equal records), likewise
  knobs3, knobs8 one process: the (n, 3) / (n, 8) crthip_fieldpass_knobs call on them
  stills         one process: crthip_stills on them, blend 1, scanlines 1, the interlaced CLI schedule, noise 0
  mixed          4096 images drawn from 64 distinct sizes between 320x240 and 796x597, packed back to back: ONE
                 crthip_fieldpass_sizes call against the loop of the 64 size-grouped crthip_fieldpass calls (64 fields each) it replaces
  stillsmixed    the same for crthip_stills_sizes against 64 crthip_stills calls (noise 0: the shared clean signal in both)
  run PARENT_DIR [MODE ...]
                 the record: every mode above (or the modes named) in five fresh processes each, `this` and PARENT_DIR (the parent commit's build of
                 libcrthip.so) interleaved for the modes the parent has, one line per process and the summary behind them"""
import os, sys, time, statistics, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ntsc-crt_amd"), os.path.join(ROOT, "tests")]

mode = sys.argv[1]
N, W, H, NOISE = 4096, 640, 480, 24
LIB = "parent" if os.environ.get("CRTHIP_LIBDIR") else "this"
OLD_MODES = ("uniform", "knobs3", "knobs8", "stills")        # what the parent commit's library has
NEW_MODES = ("sizes", "mixed", "stillsmixed")

if mode == "run":
    parent = os.path.abspath(sys.argv[2])
    lines = []
    only = sys.argv[3:]
    if only:
        OLD_MODES = tuple(m for m in OLD_MODES if m in only)
        NEW_MODES = tuple(m for m in NEW_MODES if m in only)

    def child(m, libdir):
        env = dict(os.environ)
        env.pop("CRTHIP_LIBDIR", None)
        if libdir:
            env["CRTHIP_LIBDIR"] = libdir
        r = subprocess.run([sys.executable, os.path.abspath(__file__), m], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit("time_sizes.py %s failed (%d):\n%s" % (m, r.returncode, r.stderr[-2000:]))
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("T ")]
        for ln in out:
            print(ln, flush=True)
        lines.extend(out)
    for rnd in range(5):
        for m in OLD_MODES:
            child(m, None)
            child(m, parent)
        for m in NEW_MODES:
            child(m, None)

    def field(ln, key):
        return float([t for t in ln.split() if t.startswith(key + "=")][0].split("=")[1])

    def med(m, lib, key="median_ms"):
        v = [field(ln, key) for ln in lines if ln.split()[1] == m and ("lib=" + lib) in ln]
        return statistics.median(v), min(v), max(v)
    print("\nSUMMARY (median of the five processes' medians [smallest .. largest]; ms)")
    for m in OLD_MODES:
        t, p = med(m, "this"), med(m, "parent")
        inside = p[1] <= t[0] <= p[2]
        print("  %-8s this %.4f [%.4f .. %.4f]   parent %.4f [%.4f .. %.4f]   this / parent %.4f   this's median %s the parent's own spread"
              % ((m,) + t + p + (t[0] / p[0], "INSIDE" if inside else "below" if t[0] < p[1] else "ABOVE")))
    if only:
        sys.exit(0)
    u, z = med("uniform", "this"), med("sizes", "this")
    print("  sizes call, 4096 equal 640x480 images: %.4f [%.4f .. %.4f] against the uniform call's %.4f: ratio %.4f" % (z + (u[0], z[0] / u[0])))
    for k in ("template", "active", "noise", "sync", "decode"):
        print("    per kernel %-8s uniform %.4f   sizes %.4f" % (k, med("uniform", "this", "k_" + k)[0], med("sizes", "this", "k_" + k)[0]))
    for m, what in (("mixed", "fieldpass"), ("stillsmixed", "stills")):
        one, loop = med(m, "this"), med(m, "this", "loop_ms")
        print("  %s, 4096 images of 64 sizes: ONE sizes call %.4f [%.4f .. %.4f]   the 64 grouped calls %.4f [%.4f .. %.4f]   loop / one %.2f   %.0f fields/s"
              % ((what,) + one + loop + (loop[0] / one[0], N / one[0] * 1e3)))
    sys.exit(0)

import numpy as np
import torch
import crtlib

torch.manual_seed(1)


def timed(fn, reset, reps, warm=3):
    ts = []
    for r in range(warm + reps):
        reset()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record(); b.synchronize()
        if r >= warm:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def power_on(g):
    g.out.zero_()
    g.state.zero_()
    g.state[:, crtlib.ST_RN] = 194


def per_kernel(g, fn):
    power_on(g)
    g.profile(True)
    fn()
    c = g.profile_read()
    g.profile(False)
    return " ".join("k_%s=%.4f" % (k, c[k][0]) for k in crtlib.K_NAMES)


def report(m, t, extra=""):
    print("T %s lib=%s n=%d median_ms=%.4f min=%.4f max=%.4f fields_per_s=%.0f %s" % ((m, LIB, N) + t + (N / t[0] * 1e3, extra)), flush=True)


if mode in OLD_MODES + ("sizes",):
    imgs = torch.randint(0, 256, (64, H + 1, W, 4), dtype=torch.uint8, device="cuda:0")
    full = imgs.repeat(N // 64, 1, 1, 1)
    g = crtlib.CRT(N, W, H, crtlib.FMT_BGRA, "ntsc", device=0)
    g.scanlines = 1
    g.reserve(N)
    s = crtlib.Settings(full[:, :H], format=crtlib.FMT_BGRA, as_color=1)
    if mode == "uniform":
        fn = lambda: g.fieldpass(s, NOISE)
    elif mode == "sizes":
        sz = crtlib.Settings(None, format=crtlib.FMT_BGRA, as_color=1, spare_row=True)
        p = g.sizes_params(sz, NOISE)
        g._load_field_state(sz)
        stride = (H + 1) * W * 4
        g.upload_sizes((full.reshape(-1), np.stack([np.full(N, W), np.full(N, H), np.arange(N) * stride], axis=1)), p)
        fn = lambda: g.fieldpass_sizes(None, NOISE, params=p, settings=sz)
    elif mode in ("knobs3", "knobs8"):
        k = np.arange(N)
        rows = np.stack([k % 49, (k * 7) % 801 - 400, 8 + k % 5, k % 81 - 40, 120 + (k * 5) % 121, k % 61 - 30, 60 + (k * 5) % 81, k - N // 2], axis=1)
        p = g.params(s, 0)
        g._load_field_state(s)
        g.upload_knobs(rows if mode == "knobs8" else rows[:, :3], p)
        fn = lambda: g.fieldpass_knobs(s, None, params=p)
    else:
        g.blend = 1
        g.stills_reserve(4)
        fn = lambda: g.stills(s, 0)
    t = timed(fn, lambda: power_on(g), 15 if mode == "stills" else 40, warm=5)
    report(mode, t, per_kernel(g, fn))
    g.close()
else:
    # 64 distinct sizes, 64 images of each, group after group in the one buffer: a group is also one [64, h, w, 4] tensor
    stills = mode == "stillsmixed"
    dims = [(320 + (i % 8) * 68, 240 + (i // 8) * 51) for i in range(64)]
    sizes, off = [], 0
    for w, h in dims:
        for _ in range(64):
            sizes.append((w, h, off))
            off += w * h * 4
    buf = torch.randint(0, 256, (off,), dtype=torch.uint8, device="cuda:0")
    sizes = np.array(sizes, dtype=np.int64)
    g = crtlib.CRT(N, W, H, crtlib.FMT_BGRA, "ntsc", device=0)
    g.scanlines = 1
    g.blend = 1 if stills else 0
    g.reserve(N)
    noise = 0 if stills else NOISE
    sz = crtlib.Settings(None, format=crtlib.FMT_BGRA, as_color=1, spare_row=False)
    p = g.sizes_params(sz, noise)
    g._load_field_state(sz)
    g.upload_sizes((buf, sizes), p)
    if stills:
        g.stills_reserve(4)
        fn = lambda: g.stills_sizes(None, noise, params=p, settings=sz)
    else:
        fn = lambda: g.fieldpass_sizes(None, noise, params=p, settings=sz)
    t = timed(fn, lambda: power_on(g), 10 if stills else 20)
    want = g.out.clone()
    # the grouped path: one CRT per size (its output = the group's slice of the big batch's), one call each
    groups = []
    for i, (w, h) in enumerate(dims):
        c = crtlib.CRT(64, W, H, crtlib.FMT_BGRA, "ntsc", device=0, out=g.out[64 * i:64 * (i + 1)])
        c.scanlines, c.blend = 1, g.blend
        c.reserve(64)
        if stills:
            c.stills_reserve(4)
        data = buf[int(sizes[64 * i, 2]):int(sizes[64 * i, 2]) + 64 * w * h * 4].view(64, h, w, 4)
        groups.append((c, crtlib.Settings(data, format=crtlib.FMT_BGRA, as_color=1, spare_row=False)))

    def reset_groups():
        power_on(g)
        for c, _ in groups:
            c.state.zero_()
            c.state[:, crtlib.ST_RN] = 194

    def loop():
        for c, s in groups:
            if stills:
                c.stills(s, noise)
            else:
                c.fieldpass(s, noise)
    ts = []
    for r in range(2 + 5):
        reset_groups()
        torch.cuda.synchronize()
        t0 = time.perf_counter(); loop(); torch.cuda.synchronize(); t1 = time.perf_counter()
        if r >= 2:
            ts.append((t1 - t0) * 1e3)
    same = bool(torch.equal(g.out, want))
    lp = (statistics.median(ts), min(ts), max(ts))
    report(mode, t, "loop_ms=%.4f loop_min=%.4f loop_max=%.4f loop_equals_one_call=%s" % (lp + (same,)))
    assert same, "the grouped calls and the one sizes call differ"
    for c, _ in groups:
        c.close()
    g.close()

#!/usr/bin/env python3
"""crthip_stills against the loop of crthip_fieldpass calls doing the same work, in one process (profiles/stills_timing.txt).

    python tools/time_stills.py [--n 4096] [--runs 7] [--loop-only]

Workload: n stills 640x480 BGRA in and out, blend 1, scanlines 1 (the reference's `ntsc -o 640 480 NOISE 0`): (a) interlaced, noise
24; (b) interlaced, noise 0; (c) progressive, noise 0.  Events on the stream around the call, one warm-up, the median of --runs;
the loop is timed twice (before and after the stills call) so that the file shows the spread between repeated timings of the same
thing.  --loop-only: the loop alone (what a build without crthip_stills can run)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# CRTHIP_BINDING_DIR: the crtlib.py that belongs to the library CRTHIP_LIBDIR names (timing the loop on another build)
sys.path.insert(0, os.environ.get("CRTHIP_BINDING_DIR") or os.path.join(ROOT, "ntsc-crt_amd"))
CLI = {True: [(0, 0), (1, 0), (1, 1), (0, 1), (0, 1), (1, 1), (1, 0), (0, 0)], False: [(0, 0)] * 4}     # crt_main.c:241-255


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--loop-only", action="store_true")
    a = ap.parse_args()
    import torch
    import crtlib
    n, w, h = a.n, 640, 480
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    imgs = torch.randint(0, 256, (n, h + 1, w, 4), dtype=torch.uint8, device="cuda:0", generator=gen)
    g = crtlib.CRT(n, w, h, crtlib.FMT_BGRA, "ntsc", device=0)
    g.blend = g.scanlines = 1
    s = crtlib.Settings(imgs[:, :h], format=crtlib.FMT_BGRA)
    g.reserve()
    have_stills = hasattr(g, "stills") and not a.loop_only
    if have_stills:
        g.stills_reserve(4)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def power_on():
        g.out.zero_()
        g.state.zero_()
        g.state[:, crtlib.ST_RN] = 194

    def loop(noise, interlaced):
        p = g.params(s, noise)
        for field, frame in CLI[interlaced]:
            g.state[:, crtlib.ST_FIELD] = field
            g.state[:, crtlib.ST_FRAME] = frame
            g.fieldpass(s, noise, params=p)

    def timed(fn, *args):
        ms = []
        for r in range(a.runs + 1):
            power_on()
            torch.cuda.synchronize()
            ev[0].record()
            fn(*args)
            ev[1].record()
            torch.cuda.synchronize()
            if r:
                ms.append(ev[0].elapsed_time(ev[1]))
        return statistics.median(ms), min(ms), max(ms)

    print("n = %d stills 640x480 BGRA, blend 1, scanlines 1; median (min .. max) of %d runs, ms per call" % (n, a.runs))
    for name, noise, interlaced in (("(a) interlaced, noise 24", 24, True), ("(b) interlaced, noise 0", 0, True), ("(c) progressive, noise 0", 0, False)):
        l1 = timed(loop, noise, interlaced)
        print("%-26s loop of fieldpass calls  %8.2f (%.2f .. %.2f)   %.0f stills/s" % ((name,) + l1 + (n / l1[0] * 1e3,)))
        if have_stills:
            st = timed(lambda: g.stills(s, noise, interlaced=interlaced))
            l2 = timed(loop, noise, interlaced)
            print("%-26s crthip_stills            %8.2f (%.2f .. %.2f)   %.0f stills/s   %+.1f %% against the loops' mean" %
                  ((name,) + st + (n / st[0] * 1e3, 100.0 * (st[0] / ((l1[0] + l2[0]) / 2) - 1))))
            print("%-26s loop again               %8.2f (%.2f .. %.2f)   loop-to-loop spread %.1f %%" % ((name,) + l2 + (100.0 * abs(l1[0] - l2[0]) / l1[0],)))
            lay = (C.c_int * 4)()
            fs = C.c_size_t(0)
            g.L.crthip_signal_layout_query(C.byref(g.params(s, noise)), n, 0, lay, C.byref(fs))
            distinct = len(set(CLI[interlaced])) if noise == 0 else 0
            print("%-26s shared-signal workspace  %d distinct x %d fields x %d bytes = %.2f GB" % (name, distinct, n, fs.value, distinct * n * fs.value / 1e9))
    g.close()


if __name__ == "__main__":
    main()

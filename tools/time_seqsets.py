#!/usr/bin/env python3
"""crthip_sequence_sets against the best a caller of the parent tree can do: a loop of crthip_sequence calls, one per set.

  tools/time_seqsets.py ab --parent DIR [--parent-commit ID] [--procs 5] [--out profiles/seqsets_timing.txt]
      DIR = the parent commit exported with `git archive` and built there (its ntsc-crt_amd/lib/libcrthip.so).  Runs 2 x procs fresh
      processes, alternating parent / this tree, and writes every sample, the process medians and the acceptance comparison to --out.
  tools/time_seqsets.py child --tree DIR --role parent|new
      one process: imports DIR's crtlib (and so DIR's library), prints one JSON line.
  tools/time_seqsets.py trace --sets N
      one crthip_sequence_sets call sequence of the 16-field blend workload with N sets (to be run under rocprofv3 --kernel-trace).

Timing: 3 warm-up calls, 12 timed calls, each between two device synchronisations on the host clock (the states are put back
before the first synchronisation, outside the clock); per process the median.  All calls go through the C ABI with a prebuilt
crthip_params, so no Python work per set is on the clock beyond one ctypes call.
Workloads (640x480 BGRA in and out, noise 24, scanlines 1, every set interlaced from its field 0, every set its own incoming
hsync / vsync / rn): 256 sets x 16 fields and 64 sets x 64 fields, each with blend 0, blend 1 and blend 1 + fade.
  parent:  loop1 = one crthip_sequence per set on one context;  loop3 = the sets dealt round robin over 3 contexts on 3 streams
  new:     sets = one crthip_sequence_sets;  fieldpass = crthip_fieldpass over the same 4096 fields as independent fields (what the
           kernels cost without sequence semantics);  and for information one set of 512 fields with blend 1: crthip_sequence_sets
           with n_sets = 1 (one fold launch) and this tree's crthip_sequence (one fold launch per field)."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, NOISE = 640, 480, 24
WARMUP, CALLS = 3, 12
WORKLOADS = [(256, 16), (64, 64)]
VARIANTS = [("blend0", 0, "keep"), ("blend1", 1, "keep"), ("blend1fade", 1, "fade")]


def _timed(torch, prep, fn):
    out = []
    for i in range(WARMUP + CALLS):
        prep()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARMUP:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


class _Bench:
    def __init__(self, tree):
        sys.path.insert(0, os.path.join(tree, "ntsc-crt_amd"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import numpy as np
        import torch
        import crtlib
        import crtref as R
        assert os.path.dirname(os.path.abspath(crtlib.__file__)) == os.path.join(os.path.abspath(tree), "ntsc-crt_amd")
        self.np, self.torch, self.crtlib, self.R = np, torch, crtlib, R
        self.base = torch.from_numpy(np.stack([R.synth_image(W, H, 4, 11 + k) for k in range(8)])).to("cuda:0")
        self.init = torch.from_numpy(R.lcg_bytes(W * H * 4, 5).reshape(H, W, 4).copy()).to("cuda:0")

    def images(self, n):
        full = self.torch.empty((n, H + 1, W, 4), dtype=self.torch.uint8, device="cuda:0")
        full[:, :H] = self.base.repeat((n + 7) // 8, 1, 1, 1)[:n]
        full[:, H] = full[:, H - 1]
        return full[:, :H]

    def context(self, n, n_sets, per, blend, mode, imgs):
        """a CRT over n fields with the field inputs and every set's incoming state loaded -> (crt, settings, params, state0)"""
        crtlib = self.crtlib
        g = crtlib.CRT(n, W, H, crtlib.FMT_BGRA, "ntsc", device=0)
        g.scanlines, g.blend = 1, blend
        if mode != "keep":
            g.phosphor = mode
        g.reserve(n)
        s = crtlib.Settings(imgs, format=crtlib.FMT_BGRA, field=[(k % per) & 1 for k in range(n)],
                            frame=[(((k % per) + 1) >> 1) & 1 for k in range(n)])
        g._load_field_state(s)
        p = g.params(s, NOISE)
        firsts = self.torch.arange(0, n, per, device="cuda:0")
        sets = self.torch.arange(n_sets, device="cuda:0", dtype=self.torch.int32)
        g.state[firsts, crtlib.ST_HSYNC] = (sets % 5) * 9 - 18
        g.state[firsts, crtlib.ST_VSYNC] = sets % 3
        g.state[firsts, crtlib.ST_RN] = 194 + 7919 * sets
        return g, s, p, g.state.clone()


def child(tree, role):
    b = _Bench(tree)
    torch, crtlib = b.torch, b.crtlib
    vp = C.c_void_p
    res = {"tree": tree, "role": role, "samples_ms": {}}
    jobs = [(ns, per, v) for ns, per in WORKLOADS for v in VARIANTS]
    if role == "new":
        jobs.append((1, 512, VARIANTS[1]))
    for n_sets, per, (vname, blend, mode) in jobs:
        n = n_sets * per
        key = "%dx%d/%s" % (n_sets, per, vname)
        imgs = b.images(n)
        g, s, p, st0 = b.context(n, n_sets, per, blend, mode, imgs)
        istride, ostride = g._image_stride(s), g.out.stride(0)
        img0, out0, stp0 = s.data.data_ptr(), g.out.data_ptr(), g.state.data_ptr()

        def reset():
            g.state.copy_(st0)

        def seq_call(ctx, lo, cnt):
            rc = g.L.crthip_sequence(ctx, C.byref(p), cnt, vp(img0 + lo * istride), istride, vp(out0 + lo * ostride), ostride,
                                     vp(b.init.data_ptr()), vp(stp0 + lo * 4 * crtlib.STATE_INTS), None)
            assert rc == 0, rc
        if role == "parent":
            res["samples_ms"][key + "/loop1"] = _timed(torch, reset, lambda: [seq_call(g.ctx, k * per, per) for k in range(n_sets)])
            side = []
            for _ in range(3):
                c = crtlib.CRT(1, W, H, crtlib.FMT_BGRA, "ntsc", device=0)
                c.reserve(per)
                st = torch.cuda.Stream()
                c.use_stream(st)
                side.append((c, st))
            res["samples_ms"][key + "/loop3"] = _timed(torch, reset, lambda: [seq_call(side[k % 3][0].ctx, k * per, per) for k in range(n_sets)])
            for c, _st in side:
                c.close()
        else:
            first = (C.c_int * (n_sets + 1))(*range(0, n + 1, per))

            def sets_call():
                rc = g.L.crthip_sequence_sets(g.ctx, C.byref(p), n_sets, first, vp(img0), istride, vp(out0), ostride,
                                              vp(b.init.data_ptr()), 0, vp(stp0), None)
                assert rc == 0, rc
            res["samples_ms"][key + "/sets"] = _timed(torch, reset, sets_call)
            if n_sets == 1:
                res["samples_ms"][key + "/sequence"] = _timed(torch, reset, lambda: seq_call(g.ctx, 0, n))
            else:
                res["samples_ms"][key + "/fieldpass"] = _timed(torch, reset, lambda: g.fieldpass(s, NOISE, params=p))
        g.close()
        del imgs, g
        torch.cuda.empty_cache()
    print(json.dumps(res))


def trace(n_sets):
    b = _Bench(ROOT)
    per = 16
    n = n_sets * per
    g, s, p, st0 = b.context(n, n_sets, per, 1, "keep", b.images(n))
    for _ in range(2):
        g.state.copy_(st0)
        passes = g.sequence_sets(s, NOISE, list(range(0, n + 1, per)), out_init=b.init)
        g.synchronize()
    print("trace: %d sets x %d fields, blend 1: %d sync passes per call, 2 calls" % (n_sets, per, passes))
    g.close()


def ab(parent, parent_commit, procs, out_path):
    me = os.path.abspath(__file__)
    cmds = {"parent": [sys.executable, me, "child", "--tree", parent, "--role", "parent"],
            "new": [sys.executable, me, "child", "--tree", ROOT, "--role", "new"]}
    runs = {"parent": [], "new": []}
    for i in range(procs):
        for label in ("parent", "new"):
            r = subprocess.run(cmds[label], capture_output=True, text=True, timeout=1100)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-3000:])
                raise SystemExit("child %s failed with %d" % (label, r.returncode))
            runs[label].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print("process %d %s done" % (i, label), flush=True)
    lines = ["# tools/time_seqsets.py: crthip_sequence_sets against a loop of crthip_sequence calls on the parent tree",
             "# parent commit: %s (exported with git archive, built in place)" % parent_commit,
             "# commands (alternated, %d processes each):" % procs,
             "#   python tools/time_seqsets.py child --tree PARENT_EXPORT --role parent",
             "#   python tools/time_seqsets.py child --tree . --role new",
             "# %d warm-up calls, %d timed calls per process, device-synchronised host clock, milliseconds" % (WARMUP, CALLS), ""]
    for label in ("parent", "new"):
        for i, run in enumerate(runs[label]):
            for key, v in sorted(run["samples_ms"].items()):
                lines.append("%s proc %d %-28s %s" % (label, i, key, " ".join("%.4f" % x for x in v)))
    lines.append("")

    def meds(label, key):
        return [statistics.median(run["samples_ms"][key]) for run in runs[label]]
    for label in ("parent", "new"):
        for key in sorted(runs[label][0]["samples_ms"]):
            m = meds(label, key)
            lines.append("process medians %-6s %-28s min %.4f  median %.4f  max %.4f" % (label, key, min(m), statistics.median(m), max(m)))
    lines.append("")
    ok = True
    for n_sets, per in WORKLOADS:
        for vname, _b, _m in VARIANTS:
            key = "%dx%d/%s" % (n_sets, per, vname)
            new, fp = meds("new", key + "/sets"), meds("new", key + "/fieldpass")
            for loop in ("loop1", "loop3"):
                old = meds("parent", key + "/" + loop)
                good = max(new) < min(old)
                ok = ok and good
                lines.append("%-22s sets slowest %.4f  <  parent %s fastest %.4f : %s   (median ratio %.2fx)" % (
                    key, max(new), loop, min(old), "yes" if good else "NO", statistics.median(old) / statistics.median(new)))
            lines.append("%-22s sets / fieldpass over the same fields = %.2f  (%.4f / %.4f ms)" % (
                key, statistics.median(new) / statistics.median(fp), statistics.median(new), statistics.median(fp)))
    k1 = "1x512/blend1"
    lines.append("%-22s n_sets = 1: %.4f ms, crthip_sequence (one fold launch per field): %.4f ms" % (
        k1, statistics.median(meds("new", k1 + "/sets")), statistics.median(meds("new", k1 + "/sequence"))))
    lines.append("acceptance (every workload, both loops): %s" % ("met" if ok else "NOT met"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ab", "child", "trace"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--role", default="new", choices=["parent", "new"])
    ap.add_argument("--sets", type=int, default=256)
    ap.add_argument("--parent", help="the parent commit exported with git archive and built in place (ab)")
    ap.add_argument("--parent-commit", default="unknown")
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqsets_timing.txt"))
    a = ap.parse_args()
    if a.what == "child":
        child(a.tree, a.role)
    elif a.what == "trace":
        trace(a.sets)
    else:
        ab(a.parent, a.parent_commit, a.procs, a.out)

#!/usr/bin/env python3
"""Cost of the phosphor display modes (CRTHIP_F_PHOSPHOR_FADE / _CLEAR) against the parent tree's keep mode.

  tools/time_phosphor.py ab --parent DIR [--parent-commit ID] [--procs 5] [--out profiles/phosphor_timing.txt]
      DIR = the parent commit exported with `git archive` and built there (its ntsc-crt_amd/lib/libcrthip.so).  Runs 2 x procs fresh
      processes, alternating parent / this tree, and writes every sample, the medians and the three bounds to --out.
  tools/time_phosphor.py child --tree DIR --modes keep,fade,clear
      one process: imports DIR's crtlib (and so DIR's library), prints one JSON line.

Timing: 3 warm-up calls, then >= 10 timed calls, each between two device synchronisations on the host clock; the median is reported.
Workloads (all 640x480 BGRA input and output, noise 24, scanlines 1, interlaced parities):
  seq       crthip_sequence, n = 2048, blend 0
  seqblend  crthip_sequence, n = 512, blend 1
  fp        crthip_fieldpass, n = 4096 (BASELINE configs[1]), blend 0; fpblend: the same with blend 1
and, in the same process as fp, a device-to-device copy_ of B bytes, B = the bytes of the rows no field of the batch writes (counted
from the batch's line table, which a stage-level crthip_sync gives) -- all rows for fpblend."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, NOISE = 640, 480, 24
WARMUP, CALLS = 3, 12


def _timed(torch, fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(CALLS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def child(tree, modes):
    sys.path.insert(0, os.path.join(tree, "ntsc-crt_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import crtlib
    import crtref as R
    assert os.path.dirname(os.path.abspath(crtlib.__file__)) == os.path.join(os.path.abspath(tree), "ntsc-crt_amd")
    res = {"tree": tree, "samples_ms": {}}
    base = torch.from_numpy(np.stack([R.synth_image(W, H, 4, 11 + k) for k in range(8)])).to("cuda:0")

    def images(n):
        full = torch.empty((n, H + 1, W, 4), dtype=torch.uint8, device="cuda:0")
        full[:, :H] = base.repeat((n + 7) // 8, 1, 1, 1)[:n]
        full[:, H] = full[:, H - 1]
        return full[:, :H]

    def settings(imgs, n):
        return crtlib.Settings(imgs, format=crtlib.FMT_BGRA, field=[k & 1 for k in range(n)], frame=[((k + 1) >> 1) & 1 for k in range(n)])

    for work, n, blend in (("seq", 2048, 0), ("seqblend", 512, 1)):
        imgs = images(n)
        init = torch.from_numpy(R.lcg_bytes(W * H * 4, 5).reshape(H, W, 4).copy()).to("cuda:0")
        for mode in modes:
            g = crtlib.CRT(n, W, H, crtlib.FMT_BGRA, "ntsc", device=0)
            g.scanlines, g.blend = 1, blend
            if mode != "keep":
                g.phosphor = mode
            s = settings(imgs, n)
            st0 = g.state.clone()

            def call():
                g.state.copy_(st0)
                g.sequence(s, NOISE, out_init=init)
            res["samples_ms"]["%s/%s" % (work, mode)] = _timed(torch, call)
            g.close()
            torch.cuda.empty_cache()
        del imgs
    n = 4096
    imgs = images(n)
    for work, blend in (("fp", 0), ("fpblend", 1)):
        for mode in modes:
            g = crtlib.CRT(n, W, H, crtlib.FMT_BGRA, "ntsc", device=0)
            g.scanlines, g.blend = 1, blend
            if mode != "keep":
                g.phosphor = mode
            g.reserve(n)
            s = settings(imgs, n)
            g._load_field_state(s)
            p = g.params(s, NOISE)
            res["samples_ms"]["%s/%s" % (work, mode)] = _timed(torch, lambda: g.fieldpass(s, NOISE, params=p))
            if mode == modes[-1] and blend == 0 and "fade" in modes:
                # the unowned rows of this batch: the line table of a stage-level pass over the same fields and states
                g.phosphor = "keep"
                g.modulate(s)
                g.demodulate(NOISE)
                g.synchronize()
                lt = g.line_table.cpu().numpy()
                own = np.zeros((n, H), dtype=bool)
                for k in range(n):
                    for beg, nr in zip(lt[k, :, 3], lt[k, :, 4] & 0xffff):
                        own[k, beg:min(beg + nr, H)] = True
                res["unowned_rows"] = int((~own).sum())
                g._analog = g._inp = None
            g.close()
            torch.cuda.empty_cache()
    del imgs
    torch.cuda.empty_cache()
    if "unowned_rows" in res:
        for key, nbytes in (("copy_unowned", res["unowned_rows"] * W * 4), ("copy_all", n * H * W * 4)):
            a = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
            b = torch.empty_like(a)
            res["samples_ms"][key] = _timed(torch, lambda: b.copy_(a))
            res[key + "_bytes"] = nbytes
            del a, b
    print(json.dumps(res))


def ab(parent, parent_commit, procs, out_path):
    cmd_p = [sys.executable, os.path.abspath(__file__), "child", "--tree", parent, "--modes", "keep"]
    cmd_n = [sys.executable, os.path.abspath(__file__), "child", "--tree", ROOT, "--modes", "keep,fade,clear"]
    runs = {"parent": [], "new": []}
    for i in range(procs):
        for label, cmd in (("parent", cmd_p), ("new", cmd_n)):
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-3000:])
                raise SystemExit("child %s failed with %d" % (label, r.returncode))
            runs[label].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print("process %d %s done" % (i, label), flush=True)

    def pooled(label, key):
        return [x for run in runs[label] for x in run["samples_ms"][key]]

    def med(label, key):
        return statistics.median(pooled(label, key))

    lines = ["# tools/time_phosphor.py: phosphor display modes against the parent tree's keep mode",
             "# parent commit: %s (exported with git archive, built in place)" % parent_commit,
             "# this tree: the change on top of that commit",
             "# commands (alternated, %d processes each):" % procs,
             "#   python tools/time_phosphor.py child --tree PARENT_EXPORT --modes keep",
             "#   python tools/time_phosphor.py child --tree . --modes keep,fade,clear",
             "# %d warm-up calls, %d timed calls per process, device-synchronised host clock, milliseconds" % (WARMUP, CALLS), ""]
    for label in ("parent", "new"):
        for i, run in enumerate(runs[label]):
            for key, v in sorted(run["samples_ms"].items()):
                lines.append("%s proc %d %-16s %s" % (label, i, key, " ".join("%.4f" % x for x in v)))
    lines.append("")
    keys = sorted(runs["new"][0]["samples_ms"])
    for key in sorted(runs["parent"][0]["samples_ms"]):
        lines.append("median parent %-16s %.4f" % (key, med("parent", key)))
    for key in keys:
        lines.append("median new    %-16s %.4f" % (key, med("new", key)))
    unowned = runs["new"][0]["unowned_rows"]
    lines.append("unowned rows of the fp batch (4096 fields x 480 rows): %d = %d bytes (B)" % (unowned, runs["new"][0]["copy_unowned_bytes"]))
    lines.append("")
    ok = True
    for work in ("seq", "seqblend"):
        base = med("parent", work + "/keep")
        for mode in ("fade", "clear"):
            r = med("new", "%s/%s" % (work, mode)) / base
            good = r <= 1.05 or mode == "clear"
            ok = ok and good
            lines.append("%-9s %-5s / parent keep = %.4f  (bound 1.05%s)%s" % (work, mode, r, "" if mode == "fade" else ", reported",
                                                                               "" if good else "  EXCEEDED"))
    for work, copy_key in (("fp", "copy_unowned"), ("fpblend", "copy_all")):
        base = med("parent", work + "/keep")
        cp = med("new", copy_key)
        for mode in ("fade", "clear"):
            extra = med("new", "%s/%s" % (work, mode)) - base
            r = extra / cp
            good = r <= 1.3 or work == "fpblend"
            ok = ok and good
            lines.append("%-9s %-5s extra = %.4f ms, copy_ of %s = %.4f ms, ratio %.3f  (bound 1.3%s)%s" % (
                work, mode, extra, copy_key, cp, r, "" if work == "fp" else ", reported", "" if good else "  EXCEEDED"))
    lines.append("all bounds met: %s" % ok)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ab", "child"])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--modes", default="keep,fade,clear")
    ap.add_argument("--parent", help="the parent commit exported with git archive and built in place (ab)")
    ap.add_argument("--parent-commit", default="unknown")
    ap.add_argument("--procs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phosphor_timing.txt"))
    a = ap.parse_args()
    if a.what == "child":
        child(a.tree, a.modes.split(","))
    else:
        ab(a.parent, a.parent_commit, a.procs, a.out)

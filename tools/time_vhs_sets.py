#!/usr/bin/env python3
"""crthip_sequence_sets with CRTHIP_F_VHS_SET_STREAMS (the stock VHS build, one rand() stream per set) against the best a caller of
the parent tree can do -- a loop of crthip_sequence calls, one per clip -- and the untouched paths against the parent tree.

  tools/time_vhs_sets.py ab --parent DIR [--parent-commit ID] [--procs 3] [--out profiles/vhs_sets_timing.txt]
      DIR = the parent commit exported with `git archive` and built there (its ntsc-crt_amd/lib/libcrthip.so).  Runs 2 x procs fresh
      processes, alternating parent / this tree, then one traced process for the chain kernel's own time; every process is a step
      with a time limit of its own and the first one that fails ends the run.  Writes every sample, the process medians, the ratios
      and both process-to-process spreads to --out.
  tools/time_vhs_sets.py child --tree DIR --role parent|new
      one process: imports DIR's crtlib (and so DIR's library), prints one JSON line.
  tools/time_vhs_sets.py trace
      two crthip_sequence_sets calls per workload (blend 0), to be run under rocprofv3 --kernel-trace --stats.

Timing: 3 warm-up calls, 9 timed calls, each between two device synchronisations on the host clock (states and generator
histories are put back before the first synchronisation, outside the clock); per process the median.  All calls go through the C ABI
with a prebuilt crthip_params.  640x480 BGRA in and out, noise 12, scanlines 1, every clip interlaced from its field 0 with its own
seed and incoming vsync.
  clips:   256 clips x 16 fields and 64 x 64 fields, blend 0 and 1
           parent: loop = crthip_vhs_bind_history + crthip_sequence per clip on one context;  new: sets = one crthip_sequence_sets
  untouched (both trees): seq_vhs = crthip_sequence, stock VHS, one clip of 64 fields;  sets_vhslcg = crthip_sequence_sets on vhslcg,
           256 x 16;  fieldpass_vhs = crthip_fieldpass, stock VHS, 1024 fields"""
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, NOISE = 640, 480, 12
WARMUP, CALLS = 3, 9
WORKLOADS = [(256, 16), (64, 64)]
VARIANTS = [("blend0", 0), ("blend1", 1)]
F_VHS_SET_STREAMS = 0x20000
CHILD_LIMIT_S, TRACE_LIMIT_S = 900, 600


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

    def context(self, name, n, n_sets, per, blend, imgs, flags=0):
        """a CRT over n fields with the field inputs, every clip's incoming state and seed loaded -> (crt, settings, params, reset)"""
        crtlib, torch = self.crtlib, self.torch
        g = crtlib.CRT(n, W, H, crtlib.FMT_BGRA, name, device=0)
        g.scanlines, g.blend = 1, blend
        g.reserve(n)
        s = crtlib.Settings(imgs, format=crtlib.FMT_BGRA, field=[(k % per) & 1 for k in range(n)],
                            frame=[(((k % per) + 1) >> 1) & 1 for k in range(n)])
        g._load_field_state(s)
        p = g.params(s, NOISE)
        p.flags |= flags                                   # (nothing of the blob is derived from this flag)
        firsts = torch.arange(0, n, per, device="cuda:0")
        sets = torch.arange(n_sets, device="cuda:0", dtype=torch.int32)
        g.state[firsts, crtlib.ST_VSYNC] = sets % 3
        g.state[firsts, crtlib.ST_RN] = 194 + 7919 * sets
        if g.vhs_hist is not None:
            g.srand([1000 + (k // per) if k % per == 0 else 1 for k in range(n)])
        st0 = g.state.clone()
        h0 = g.vhs_hist.clone() if g.vhs_hist is not None else None

        def reset():
            g.state.copy_(st0)
            if h0 is not None:
                g.vhs_hist.copy_(h0)
        return g, s, p, reset


def child(tree, role):
    b = _Bench(tree)
    torch, crtlib = b.torch, b.crtlib
    vp = C.c_void_p
    res = {"tree": tree, "role": role, "samples_ms": {}}
    for n_sets, per in WORKLOADS:
        n = n_sets * per
        imgs = b.images(n)
        for vname, blend in VARIANTS:
            key = "%dx%d/%s" % (n_sets, per, vname)
            g, s, p, reset = b.context("vhs", n, n_sets, per, blend, imgs, F_VHS_SET_STREAMS if role == "new" else 0)
            istride, ostride = g._image_stride(s), g.out.stride(0)
            img0, out0, stp0, h0 = s.data.data_ptr(), g.out.data_ptr(), g.state.data_ptr(), g.vhs_hist.data_ptr()
            if role == "parent":
                def loop():
                    for k in range(n_sets):
                        lo = k * per
                        rc = g.L.crthip_vhs_bind_history(g.ctx, vp(h0 + lo * 128))
                        rc = rc or g.L.crthip_sequence(g.ctx, C.byref(p), per, vp(img0 + lo * istride), istride, vp(out0 + lo * ostride), ostride,
                                                       vp(b.init.data_ptr()), vp(stp0 + lo * 4 * crtlib.STATE_INTS), None)
                        assert rc == 0, rc
                res["samples_ms"][key + "/loop"] = _timed(torch, reset, loop)
            else:
                first = (C.c_int * (n_sets + 1))(*range(0, n + 1, per))

                def sets_call():
                    rc = g.L.crthip_sequence_sets(g.ctx, C.byref(p), n_sets, first, vp(img0), istride, vp(out0), ostride,
                                                  vp(b.init.data_ptr()), 0, vp(stp0), None)
                    assert rc == 0, g.L.crthip_error_string(g.ctx)
                res["samples_ms"][key + "/sets"] = _timed(torch, reset, sets_call)
            g.close()
            del g
        del imgs
        torch.cuda.empty_cache()
    # the untouched paths, the same calls on both trees
    imgs = b.images(64)
    g, s, p, reset = b.context("vhs", 64, 1, 64, 0, imgs)
    res["samples_ms"]["untouched/seq_vhs"] = _timed(torch, reset, lambda: g.sequence(s, NOISE, out_init=b.init))
    g.close()
    imgs = b.images(4096)
    g, s, p, reset = b.context("vhslcg", 4096, 256, 16, 0, imgs)
    first = list(range(0, 4097, 16))
    res["samples_ms"]["untouched/sets_vhslcg"] = _timed(torch, reset, lambda: g.sequence_sets(s, NOISE, first, out_init=b.init))
    g.close()
    g, s, p, reset = b.context("vhs", 1024, 1024, 1, 0, imgs[:1024])
    res["samples_ms"]["untouched/fieldpass_vhs"] = _timed(torch, reset, lambda: g.fieldpass(s, NOISE, params=p))
    g.close()
    print(json.dumps(res))


def trace():
    b = _Bench(ROOT)
    for n_sets, per in WORKLOADS:
        n = n_sets * per
        g, s, p, reset = b.context("vhs", n, n_sets, per, 0, b.images(n))
        for _ in range(2):
            reset()
            passes = g.sequence_sets(s, NOISE, list(range(0, n + 1, per)), out_init=b.init, vhs_streams=True)
            g.synchronize()
        print("trace: %d sets x %d fields: %d sync passes per call, 2 calls" % (n_sets, per, passes))
        g.close()
        b.torch.cuda.empty_cache()


def _chain_times(procs_env):
    """one traced process -> [(grid as 'calls of k_vhs_chain', average ns)] from rocprofv3's kernel trace"""
    me = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory(prefix="vhs_sets_trace") as tmp:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, me, "trace"],
                           capture_output=True, text=True, timeout=TRACE_LIMIT_S, env=procs_env)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-3000:])
            raise SystemExit("the traced process failed with %d" % r.returncode)
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "k_vhs_chain" in row.get("Kernel_Name", ""):
                        rows.append((int(row["Grid_Size_X"]) // max(1, int(row["Workgroup_Size_X"])),
                                     (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6))
        if not rows:
            raise SystemExit("no k_vhs_chain launch in the kernel trace")
        return rows


def ab(parent, parent_commit, procs, out_path):
    me = os.path.abspath(__file__)
    cmds = {"parent": [sys.executable, me, "child", "--tree", parent, "--role", "parent"],
            "new": [sys.executable, me, "child", "--tree", ROOT, "--role", "new"]}
    runs = {"parent": [], "new": []}
    for i in range(procs):
        for label in ("parent", "new"):
            r = subprocess.run(cmds[label], capture_output=True, text=True, timeout=CHILD_LIMIT_S)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-3000:])
                raise SystemExit("child %s failed with %d: nothing more is started" % (label, r.returncode))
            runs[label].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print("process %d %s done" % (i, label), flush=True)
    chain = _chain_times(dict(os.environ))
    lines = ["# tools/time_vhs_sets.py: crthip_sequence_sets with CRTHIP_F_VHS_SET_STREAMS against a loop of crthip_sequence calls on the parent tree",
             "# parent commit: %s (exported with git archive, built in place)" % parent_commit,
             "# commands (alternated, %d fresh processes each, then one traced process):" % procs,
             "#   python tools/time_vhs_sets.py child --tree PARENT_EXPORT --role parent",
             "#   python tools/time_vhs_sets.py child --tree . --role new",
             "#   rocprofv3 --kernel-trace -- python tools/time_vhs_sets.py trace",
             "# 640x480 BGRA, stock VHS build, noise %d; %d warm-up calls, %d timed calls per process, device-synchronised host clock, milliseconds"
             % (NOISE, WARMUP, CALLS), ""]
    for label in ("parent", "new"):
        for i, run in enumerate(runs[label]):
            for key, v in sorted(run["samples_ms"].items()):
                lines.append("%s proc %d %-26s %s" % (label, i, key, " ".join("%.4f" % x for x in v)))
    lines.append("")

    def meds(label, key):
        return [statistics.median(run["samples_ms"][key]) for run in runs[label]]
    for label in ("parent", "new"):
        for key in sorted(runs[label][0]["samples_ms"]):
            m = meds(label, key)
            lines.append("process medians %-6s %-26s min %.4f  median %.4f  max %.4f" % (label, key, min(m), statistics.median(m), max(m)))
    lines.append("")
    lines.append("1. the new call against the loop it replaces (median of the process medians)")
    for n_sets, per in WORKLOADS:
        for vname, _b in VARIANTS:
            key = "%dx%d/%s" % (n_sets, per, vname)
            new, old = meds("new", key + "/sets"), meds("parent", key + "/loop")
            lines.append("%-14s sets %.4f ms (slowest %.4f)   parent loop %.4f ms (fastest %.4f)   ratio %.2fx" % (
                key, statistics.median(new), max(new), statistics.median(old), min(old), statistics.median(old) / statistics.median(new)))
    for n_sets, per in WORKLOADS:
        t = [ms for grid, ms in chain if grid == n_sets]
        if t:
            lines.append("k_vhs_chain<SETS> alone, %d workgroups x %d fields (kernel trace, %d launches): %s ms = %.4f ms per field of the longest set"
                         % (n_sets, per, len(t), " ".join("%.4f" % x for x in t), statistics.median(t) / per))
    lines.append("")
    lines.append("2. the untouched paths against the parent commit: unchanged = this tree's median inside the parent's own process-to-process spread")
    for key in ("untouched/seq_vhs", "untouched/sets_vhslcg", "untouched/fieldpass_vhs"):
        new, old = meds("new", key), meds("parent", key)
        inside = min(old) <= statistics.median(new) <= max(old)
        lines.append("%-26s parent spread [%.4f, %.4f] median %.4f   this tree spread [%.4f, %.4f] median %.4f : %s" % (
            key, min(old), max(old), statistics.median(old), min(new), max(new), statistics.median(new),
            "inside" if inside else ("OUTSIDE (faster)" if statistics.median(new) < min(old) else "OUTSIDE (slower)")))
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
    ap.add_argument("--parent", help="the parent commit exported with git archive and built in place (ab)")
    ap.add_argument("--parent-commit", default="unknown")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vhs_sets_timing.txt"))
    a = ap.parse_args()
    if a.what == "child":
        child(a.tree, a.role)
    elif a.what == "trace":
        trace()
    else:
        ab(a.parent, a.parent_commit, a.procs, a.out)

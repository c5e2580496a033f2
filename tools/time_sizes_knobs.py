"""The record of profiles/sizes_knobs_timing.txt (python tools/time_sizes_knobs.py MODE [ARG ...]; NTSC -> 640x480 BGRA, N = 4096 fields):
  resources PARENT_LIB [THIS_LIB]
                 no GPU: the kernel descriptors' metadata (llvm-readelf --notes on the gfx950 code objects inside libcrthip.so) of the
                 parent commit's build and of this one -- every existing kernel unchanged?, and every SZ + KN / LV / HU instantiation
                 of k_active beside its SZ twin and its per-lane knob twin
  one            one process: ONE crthip_fieldpass_sizes_knobs call on 4096 images of 64 sizes (tools/time_sizes.py's) with 4096
                 distinct (n, 8) looks; the median, the per-kernel times, and beside it crthip_fieldpass_sizes on the same images at
                 the looks' largest noise (no knobs)
  grouped        one process: the loop of 64 size-grouped crthip_fieldpass_knobs calls (64 fields each) the one call replaces, and
                 whether their pictures are byte-identical to the one call's
  batch1         one process: the loop of batch-1 crthip_fieldpass calls on a sample of 64 fields (one context per field, the field's
                 own size and eight values), extrapolated to 4096
  fieldpass, knobs3, knobs5, knobs7, knobs8, sizes, stills, stills_knobs, stills_sizes
                 one process each: the paths this change leaves alone, on 4096 images 640x480 (CRTHIP_LIBDIR = another build of the
                 library, e.g. the parent commit's)
  run PARENT_DIR [PROCESSES [MODE ...]]
                 every mode above in PROCESSES (default 3) fresh processes each, `this` and PARENT_DIR interleaved for the untouched
                 paths, one line per process and the summary behind them"""
import os, sys, time, statistics, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ntsc-crt_amd"), os.path.join(ROOT, "tests")]

mode = sys.argv[1]
N, W, H, NOISE = 4096, 640, 480, 24
LIB = "parent" if os.environ.get("CRTHIP_LIBDIR") else "this"
OLD_MODES = ("fieldpass", "knobs3", "knobs5", "knobs7", "knobs8", "sizes", "stills", "stills_knobs", "stills_sizes")
NEW_MODES = ("one", "grouped", "batch1")

if mode == "resources":
    import re, struct, tempfile

    def kernels(path):
        """{demangled name: (vgpr, sgpr, agpr, lds, scratch)} over the gfx950 code objects bundled into the library"""
        data = open(path, "rb").read()
        magic, out, at = b"__CLANG_OFFLOAD_BUNDLE__", {}, 0
        while True:
            at = data.find(magic, at)
            if at < 0:
                break
            n, o = struct.unpack_from("<Q", data, at + 24)[0], at + 32
            for _ in range(n):
                off, size, ts = struct.unpack_from("<QQQ", data, o)
                triple = data[o + 24:o + 24 + ts]
                o += 24 + ts
                if b"gfx950" not in triple or size == 0:
                    continue
                with tempfile.NamedTemporaryFile(suffix=".co") as f:
                    f.write(data[at + off:at + off + size])
                    f.flush()
                    notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
                for blk in notes.split("  - .agpr_count:")[1:]:
                    get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                    name = re.search(r"\.name:\s+(\S+)", blk).group(1).strip("'")
                    out[name] = (get("vgpr_count"), get("sgpr_count"), int(blk.split()[0]), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
            at += len(magic)
        names = list(out)
        dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return {d: out[m] for m, d in zip(names, dem)}

    def waves(vgpr, lds):
        return min(4 * min(8, 512 // ((vgpr + 7) // 8 * 8)), (160 * 1024) // lds if lds else 32)

    parent = kernels(sys.argv[2])
    this = kernels(sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "ntsc-crt_amd", "lib", "libcrthip.so"))
    changed = [k for k in parent if k not in this or this[k] != parent[k]]
    added = [k for k in this if k not in parent]
    print("    kernels in the parent's library              %d" % len(parent))
    print("    of them with ANY of the five values changed  %d" % len(changed))
    for k in changed[:20]:
        print("        %s: %s -> %s" % (k, parent[k], this.get(k)))
    print("    kernels added                                %d" % len(added))
    others = [k for k in added if not re.search(r"k_active<.*, true>\(", k)]
    print("    of them NOT k_active<..., SZ = true>          %d" % len(others))
    pat = re.compile(r"k_active<(Sys\w+), (true|false), (true|false), (true|false), true, (\d+), (\d+), (\d+), (true|false), (true|false), (true|false), (true|false)>")
    tab = {}
    for k, v in this.items():
        m = pat.search(k)
        if m:
            g = m.groups()
            tab[(g[0],) + tuple(int(x == "true") if x in ("true", "false") else int(x) for x in g[1:])] = v
    b = lambda x: int(bool(x))
    for system in sys.argv[4:] or ["SysNTSC"]:
        print("\nsystem   noise fast in4 act kn lv hu | SZ+knobs: vgpr sgpr lds waves/CU | SZ twin: vgpr sgpr lds waves/CU | per-lane knob twin: vgpr sgpr lds waves/CU")
        low = []
        for key in sorted(tab):
            s, nz, fa, i4, act, ot, ol, kn, lv, hu, szf = key
            if s != system or not szf or not (kn or lv or hu):
                continue
            new, sz, pl = tab[key], tab.get((s, nz, fa, i4, act, ot, ol, 0, 0, 0, 1)), tab.get((s, nz, fa, i4, act, ot, ol, kn, lv, hu, 0))
            cell = lambda v: "%4d %4d %6d %3d" % (v[0], v[1], v[3], waves(v[0], v[3])) if v else "   (no such instantiation)"
            print("%-8s %d     %d    %d   %2d  %d  %d  %d  |   %s   |   %s   |   %s" % (s, nz, fa, i4, act, kn, lv, hu, cell(new), cell(sz), cell(pl)))
            assert sz and new[3] == sz[3] and new[4] == 0, "LDS of the SZ twin, no scratch"
            if pl and waves(new[0], new[3]) < min(waves(sz[0], sz[3]), waves(pl[0], pl[3])):
                low.append(key)
        print("instantiations with fewer waves per CU than BOTH twins: %s" % (low or "none"))
    sys.exit(0)

if mode == "run":
    parent = os.path.abspath(sys.argv[2])
    procs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    only = sys.argv[4:]
    if only:
        OLD_MODES = tuple(m for m in OLD_MODES if m in only)
        NEW_MODES = tuple(m for m in NEW_MODES if m in only)
    lines = []

    def child(m, libdir):
        env = dict(os.environ)
        env.pop("CRTHIP_LIBDIR", None)
        if libdir:
            env["CRTHIP_LIBDIR"] = libdir
        r = subprocess.run([sys.executable, os.path.abspath(__file__), m], env=env, capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            sys.exit("time_sizes_knobs.py %s failed (%d):\n%s" % (m, r.returncode, r.stderr[-2000:]))
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("T ")]
        for ln in out:
            print(ln, flush=True)
        lines.extend(out)
    for rnd in range(procs):
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
    print("\nSUMMARY (median of the %d processes' medians [smallest .. largest]; ms; one process at a time on one MI355X)" % procs)
    for m in OLD_MODES:
        t, p = med(m, "this"), med(m, "parent")
        inside = p[1] <= t[0] <= p[2]
        print("  %-12s this %.4f [%.4f .. %.4f]   parent %.4f [%.4f .. %.4f]   this / parent %.4f   this's median %s the parent's own spread"
              % ((m,) + t + p + (t[0] / p[0], "INSIDE" if inside else "below" if t[0] < p[1] else "ABOVE")))
    if "one" in NEW_MODES:
        one, plain = med("one", "this"), med("one", "this", "sizes_ms")
        print("  ONE sizes_knobs call %.4f [%.4f .. %.4f]   fieldpass_sizes without knobs %.4f [%.4f .. %.4f]   ratio %.3f   %.0f fields/s"
              % (one + plain + (one[0] / plain[0], N / one[0] * 1e3)))
        print("  k_active alone: SZ + KN + LV + HU %.4f   its SZ twin (fieldpass_sizes) %.4f   ratio %.3f"
              % (med("one", "this", "k_active")[0], med("one", "this", "sizes_k_active")[0], med("one", "this", "k_active")[0] / med("one", "this", "sizes_k_active")[0]))
        if "grouped" in NEW_MODES:
            lp = med("grouped", "this", "loop_ms")
            print("  the 64 grouped fieldpass_knobs calls %.4f [%.4f .. %.4f]   loop / one %.2f" % (lp + (lp[0] / one[0],)))
        if "batch1" in NEW_MODES:
            b1 = med("batch1", "this", "extrapolated_ms")
            print("  the batch-1 loop, 64 fields extrapolated to %d: %.1f [%.1f .. %.1f]   loop / one %.0f   %.0f fields/s"
                  % ((N,) + b1 + (b1[0] / one[0], N / b1[0] * 1e3)))
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


def per_kernel(g, fn, prefix="k_"):
    power_on(g)
    g.profile(True)
    fn()
    c = g.profile_read()
    g.profile(False)
    return " ".join("%s%s=%.4f" % (prefix, k, c[k][0]) for k in crtlib.K_NAMES)


def report(m, t, extra=""):
    print("T %s lib=%s n=%d median_ms=%.4f min=%.4f max=%.4f fields_per_s=%.0f %s" % ((m, LIB, N) + t + (N / t[0] * 1e3, extra)), flush=True)


def looks(n):
    """n distinct (n, 8) looks inside the encoder's fast envelope: noise 0 .. 48, every knob moving at its own period"""
    k = np.arange(n)
    return np.stack([k % 49, (k * 7) % 801 - 400, 8 + k % 5, k % 81 - 40, 120 + (k * 5) % 121, k % 61 - 30, 60 + (k * 5) % 81, k - n // 2], axis=1).astype(np.int32)


def new_crt(n, out=None, blend=0):
    g = crtlib.CRT(n, W, H, crtlib.FMT_BGRA, "ntsc", device=0, out=out)
    g.scanlines = 1
    g.blend = blend
    g.reserve(n)
    return g


if mode in OLD_MODES:
    imgs = torch.randint(0, 256, (64, H + 1, W, 4), dtype=torch.uint8, device="cuda:0")
    full = imgs.repeat(N // 64, 1, 1, 1)
    stills = mode.startswith("stills")
    g = new_crt(N, blend=1 if stills else 0)
    s = crtlib.Settings(full[:, :H], format=crtlib.FMT_BGRA, as_color=1)
    rows = looks(N)
    if stills:
        g.stills_reserve(4)
    if mode == "fieldpass":
        fn = lambda: g.fieldpass(s, NOISE)
    elif mode in ("sizes", "stills_sizes"):
        sz = crtlib.Settings(None, format=crtlib.FMT_BGRA, as_color=1, spare_row=True)
        p = g.sizes_params(sz, 0 if stills else NOISE)
        g._load_field_state(sz)
        g.upload_sizes((full.reshape(-1), np.stack([np.full(N, W), np.full(N, H), np.arange(N) * (H + 1) * W * 4], axis=1)), p)
        fn = (lambda: g.stills_sizes(None, 0, params=p, settings=sz)) if stills else (lambda: g.fieldpass_sizes(None, NOISE, params=p, settings=sz))
    elif mode.startswith("knobs") or mode == "stills_knobs":
        p = g.params(s, 0)
        g._load_field_state(s)
        if mode == "stills_knobs":
            rows[:, 0] = 0                                           # every still clean: the shared signal, as in `stills`
            g.upload_knobs(rows, p)
            fn = lambda: g.stills_knobs(s, None, params=p)
        else:
            g.upload_knobs(rows[:, :int(mode[5:])], p)
            fn = lambda: g.fieldpass_knobs(s, None, params=p)
    else:
        fn = lambda: g.stills(s, 0)
    t = timed(fn, lambda: power_on(g), 10 if stills else 30, warm=4)
    report(mode, t, per_kernel(g, fn))
    g.close()
    sys.exit(0)

# the mixed batch of tools/time_sizes.py: 64 distinct sizes, 64 images of each, group after group in the one buffer
dims = [(320 + (i % 8) * 68, 240 + (i // 8) * 51) for i in range(64)]
sizes, off = [], 0
for w, h in dims:
    for _ in range(64):
        sizes.append((w, h, off))
        off += w * h * 4
buf = torch.randint(0, 256, (off,), dtype=torch.uint8, device="cuda:0")
sizes = np.array(sizes, dtype=np.int64)
rows = looks(N)
sz = crtlib.Settings(None, format=crtlib.FMT_BGRA, as_color=1, spare_row=False)


def one_call(g):
    p = g.sizes_params(sz, 0)
    g._load_field_state(sz)
    g.upload_sizes((buf, sizes), p)
    g.upload_knobs(rows, p)
    return lambda: g.fieldpass_sizes_knobs(None, None, params=p, settings=sz)


if mode == "one":
    g = new_crt(N)
    fn = one_call(g)
    t = timed(fn, lambda: power_on(g), 20)
    pk = per_kernel(g, fn)
    # the same images through crthip_fieldpass_sizes: no knobs, the looks' largest noise everywhere
    p2 = g.sizes_params(sz, int(rows[:, 0].max()))
    fn2 = lambda: g.fieldpass_sizes(None, 0, params=p2, settings=sz)
    t2 = timed(fn2, lambda: power_on(g), 20)
    report(mode, t, "%s sizes_ms=%.4f sizes_min=%.4f sizes_max=%.4f %s" % ((pk,) + t2 + (per_kernel(g, fn2, "sizes_k_"),)))
    g.close()
elif mode == "grouped":
    g = new_crt(N)
    fn = one_call(g)
    power_on(g)
    fn()
    torch.cuda.synchronize()
    want = g.out.clone()
    groups = []
    for i, (w, h) in enumerate(dims):
        c = new_crt(64, out=g.out[64 * i:64 * (i + 1)])
        data = buf[int(sizes[64 * i, 2]):int(sizes[64 * i, 2]) + 64 * w * h * 4].view(64, h, w, 4)
        s = crtlib.Settings(data, format=crtlib.FMT_BGRA, as_color=1, spare_row=False)
        p = c.params(s, 0)
        c._load_field_state(s)
        c.upload_knobs(rows[64 * i:64 * (i + 1)], p)
        groups.append((c, s, p))

    def reset_groups():
        g.out.zero_()
        for c, _, _ in groups:
            c.state.zero_()
            c.state[:, crtlib.ST_RN] = 194
    ts = []
    for r in range(2 + 5):
        reset_groups()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c, s, p in groups:
            c.fieldpass_knobs(s, None, params=p)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if r >= 2:
            ts.append((t1 - t0) * 1e3)
    same = bool(torch.equal(g.out, want))
    lp = (statistics.median(ts), min(ts), max(ts))
    report(mode, lp, "loop_ms=%.4f loop_min=%.4f loop_max=%.4f loop_equals_one_call=%s" % (lp + (same,)))
    assert same, "the grouped knob calls and the one sizes_knobs call differ"
    for c, _, _ in groups:
        c.close()
    g.close()
elif mode == "batch1":
    # every 64th field: one of each size, its own look -- one context per field, everything set up beforehand; the loop is the calls
    sample = list(range(0, N, 64))
    ctxs = []
    for k in sample:
        w, h, o = (int(v) for v in sizes[k])
        c = new_crt(1)
        r = rows[k]
        c.hue, c.saturation, c.brightness, c.contrast, c.black_point, c.white_point = (int(v) for v in r[1:7])
        s = crtlib.Settings(buf[o:o + w * h * 4].view(1, h, w, 4), format=crtlib.FMT_BGRA, as_color=1, hue=int(r[7]), spare_row=False)
        ctxs.append((c, s, int(r[0])))
    ts = []
    for rep in range(2 + 5):
        for c, _, _ in ctxs:
            power_on(c)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c, s, nz in ctxs:
            c.fieldpass(s, nz)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if rep >= 2:
            ts.append((t1 - t0) * 1e3)
    lp = (statistics.median(ts), min(ts), max(ts))
    print("T batch1 lib=%s n=%d median_ms=%.4f min=%.4f max=%.4f sample=%d extrapolated_ms=%.2f fields_per_s=%.0f"
          % ((LIB, N) + lp + (len(sample), lp[0] * N / len(sample), len(sample) / lp[0] * 1e3)), flush=True)
    for c, _, _ in ctxs:
        c.close()

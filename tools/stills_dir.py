#!/usr/bin/env python3
"""Finished stills for a folder of images: what the reference's `ntsc` program (crt_main.c) writes for every file, in batches.

    python tools/stills_dir.py [--one-call [--looks FILE]] [-m|f|p|r] OUTW OUTH NOISE HUE IN_DIR OUT_DIR

The flags are `ntsc`'s (crt_main.c:95-110): m monochrome, f start at the odd field, p progressive, r raw (no scaling); o is accepted
and ignored (existing files are overwritten), a (analog dumps) is not available.  Every P6 .ppm of IN_DIR is read; files of equal
size form a batch (the parameters are uniform per batch) that goes through ONE crthip_stills call (CRT.stills: at noise 0 every
distinct field / frame of the schedule is encoded once for the batch); OUT_DIR/<name>.ppm is byte-identical to `ntsc`'s output.

--one-call: the files are NOT grouped by size; the whole folder (MAX_BATCH files at a time) goes through one crthip_stills_sizes call
(CRT.stills_sizes: every still with its own w and h), with byte-identical output files.  Not with r: raw images are refused there
(the signal rectangle then depends on the image size).  The default stays the grouped path.

--one-call --looks FILE: every picture with its own look -- FILE holds one line per picture, the file name and eight integers (noise,
mon_hue, saturation, brightness, contrast, black_point, white_point, hue), which replace NOISE, HUE and crt_init's defaults for that
picture; the folder goes through one crthip_stills_sizes_knobs call (CRT.stills_sizes_knobs).  A file that gives every picture
NOISE, HUE and the defaults (default_look) writes what --one-call alone writes.

PPM reading and writing are numpy: ppm_read24 / ppm_write24 (ppm_rw.c) restated.  The pixels travel as RGB24 in both directions
(CRTHIP_FMT_RGB): the encoder reads the same r, g, b whatever the byte order, and the colour bytes of the decoder's blended BGRA
words (crt_core.c:584-609) are what it writes into an RGB picture -- three quarters of the memory of crt_main.c's BGRA."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ntsc-crt_amd"))

MAX_BATCH = 1024                                        # stills per call


def read_ppm(path):
    """ppm_read24: three header lines (lines starting with '#' skipped, at most 63 bytes each), then binary RGB; values are scaled
    to 8 bits by (x * 255 + maxc / 2) / maxc.  Returns [h, w, 3] uint8."""
    with open(path, "rb") as f:
        header = []
        while len(header) < 3:
            line = f.readline(63)
            if not line:
                raise ValueError("%s: invalid ppm [no data]" % path)
            if line[:1] == b"#":
                continue
            header.append(line)
        if header[0][:2] != b"P6":
            raise ValueError("%s: invalid ppm [not P6]" % path)
        dims = header[1].split()
        if len(dims) < 2:
            raise ValueError("%s: invalid ppm [no dim]" % path)
        w, h = int(dims[0]), int(dims[1])
        tok = header[2].split()
        maxc = int(tok[0]) if tok else 0
        if maxc > 0xff or maxc <= 0:
            raise ValueError("%s: invalid ppm [maxval %d]" % (path, maxc))
        raw = f.read(w * h * 3)
    if len(raw) < w * h * 3:
        raise ValueError("%s: early eof" % path)
    px = np.frombuffer(raw, dtype=np.uint8).reshape(h, w, 3)
    if maxc != 0xff:
        px = ((px.astype(np.int32) * 255 + maxc // 2) // maxc).astype(np.uint8)
    return px


def write_ppm(path, rgb):
    """ppm_write24"""
    h, w = rgb.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb).tobytes())


def parse_flags(arg):
    opt = dict(docolor=1, field=0, progressive=0, raw=0)
    for ch in arg.lstrip("-"):
        if ch == "m":
            opt["docolor"] = 0
        elif ch == "f":
            opt["field"] = 1
        elif ch == "p":
            opt["progressive"] = 1
        elif ch == "r":
            opt["raw"] = 1
        elif ch == "o":
            pass
        else:
            raise SystemExit("Unrecognized flag '%s'" % ch)
    return opt


def convert_batch(crtlib, torch, imgs, outw, outh, noise, hue, opt):
    """imgs: [n, h, w, 3] uint8 RGB -> [n, outh, outw, 3] uint8 RGB"""
    n, h, w = imgs.shape[:3]
    crt = crtlib.CRT(n, outw, outh, crtlib.FMT_RGB, "ntsc", device=0)
    crt.blend = crt.scanlines = 1                                   # crt_main.c:235-236
    data = torch.from_numpy(np.ascontiguousarray(imgs)).to(crt.dev)
    s = crtlib.Settings(data, format=crtlib.FMT_RGB, raw=opt["raw"], as_color=opt["docolor"], hue=hue, spare_row=False)
    crt.stills(s, noise, interlaced=not opt["progressive"], first_field=opt["field"], frames=4)
    crt.synchronize()
    out = crt.out.cpu().numpy()
    crt.close()
    return out


def convert_mixed(crtlib, torch, imgs, outw, outh, noise, hue, opt):
    """imgs: a list of n [h_k, w_k, 3] uint8 RGB images of any sizes -> [n, outh, outw, 3] uint8 RGB, in ONE stills_sizes call"""
    crt = crtlib.CRT(len(imgs), outw, outh, crtlib.FMT_RGB, "ntsc", device=0)
    crt.blend = crt.scanlines = 1                                   # crt_main.c:235-236
    s = crtlib.Settings(None, format=crtlib.FMT_RGB, raw=0, as_color=opt["docolor"], hue=hue, spare_row=False)
    data = [torch.from_numpy(np.array(px)).to(crt.dev) for px in imgs]        # (a copy: read_ppm's arrays are read-only views)
    crt.stills_sizes(data, noise, interlaced=not opt["progressive"], first_field=opt["field"], frames=4, settings=s)
    crt.synchronize()
    out = crt.out.cpu().numpy()
    crt.close()
    return out


LOOK_NAMES = ("noise", "mon_hue", "saturation", "brightness", "contrast", "black_point", "white_point", "hue")


def default_look(noise, hue):
    """the look the command line gives every picture: NOISE and HUE beside crt_init's defaults (crt_core.c:263-289)"""
    return (noise, 0, 10, 0, 180, 0, 100, hue)


def parse_looks(path, names):
    """--looks FILE: one line per picture -- the file name and eight integers, LOOK_NAMES in this order; empty lines and lines
    starting with '#' are skipped.  Returns an (n, 8) int32 array in the order of ``names``; a picture without a line, a line for
    no picture, a name given twice or a malformed line is an error.  Noise below 0 becomes 0 and the hue is reduced by C's % 360,
    as the command line's are."""
    looks = {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if len(tok) != 1 + len(LOOK_NAMES):
                raise SystemExit("%s:%d: a file name and %d integers are needed (%s)" % (path, ln, len(LOOK_NAMES), " ".join(LOOK_NAMES)))
            try:
                vals = [int(t) for t in tok[1:]]
            except ValueError:
                raise SystemExit("%s:%d: not an integer" % (path, ln))
            if tok[0] in looks:
                raise SystemExit("%s:%d: %s has a look already" % (path, ln, tok[0]))
            vals[0] = max(vals[0], 0)
            vals[7] = int(np.fmod(vals[7], 360))
            looks[tok[0]] = vals
    missing = [n for n in names if n not in looks]
    extra = sorted(set(looks) - set(names))
    if missing or extra:
        raise SystemExit("%s: no look for %s; no picture for %s" % (path, ", ".join(missing) or "-", ", ".join(extra) or "-"))
    return np.array([looks[n] for n in names], dtype=np.int32).reshape(len(names), len(LOOK_NAMES))


def convert_mixed_looks(crtlib, torch, imgs, looks, outw, outh, opt):
    """convert_mixed with row k of ``looks`` ((n, 8), LOOK_NAMES) as picture k's look, in ONE stills_sizes_knobs call"""
    crt = crtlib.CRT(len(imgs), outw, outh, crtlib.FMT_RGB, "ntsc", device=0)
    crt.blend = crt.scanlines = 1                                   # crt_main.c:235-236
    s = crtlib.Settings(None, format=crtlib.FMT_RGB, raw=0, as_color=opt["docolor"], hue=0, spare_row=False)
    data = [torch.from_numpy(np.array(px)).to(crt.dev) for px in imgs]
    crt.stills_sizes_knobs(data, looks, interlaced=not opt["progressive"], first_field=opt["field"], frames=4, settings=s)
    crt.synchronize()
    out = crt.out.cpu().numpy()
    crt.close()
    return out


def main(argv):
    args = argv[1:]
    one_call = "--one-call" in args
    if one_call:
        args.remove("--one-call")
    looks_file = None
    if "--looks" in args:
        i = args.index("--looks")
        if i + 1 >= len(args):
            raise SystemExit(__doc__)
        looks_file = args[i + 1]
        del args[i:i + 2]
        if not one_call:
            raise SystemExit("--looks goes with --one-call")
    opt = parse_flags(args.pop(0)) if args and args[0].startswith("-") else parse_flags("")
    if len(args) != 6:
        raise SystemExit(__doc__)
    outw, outh, noise, hue = (int(a) for a in args[:4])
    noise = max(noise, 0)                                            # crt_main.c:187
    hue = int(np.fmod(hue, 360))                                     # C's %: the sign of the dividend
    in_dir, out_dir = args[4], args[5]
    import torch
    import crtlib
    names = sorted(f for f in os.listdir(in_dir) if f.lower().endswith(".ppm"))
    if one_call and opt["raw"]:
        raise SystemExit("--one-call: raw images (r) keep the grouped path")
    by_size = {}
    for name in names:
        px = read_ppm(os.path.join(in_dir, name))
        by_size.setdefault(px.shape[:2], []).append((name, px))
    os.makedirs(out_dir, exist_ok=True)
    done = 0
    if one_call:
        files = [(name, px) for _, group in sorted(by_size.items()) for name, px in group]
        looks = parse_looks(looks_file, [name for name, _ in files]) if looks_file else None
        for lo in range(0, len(files), MAX_BATCH):
            part = files[lo:lo + MAX_BATCH]
            if looks is not None:
                out = convert_mixed_looks(crtlib, torch, [px for _, px in part], looks[lo:lo + MAX_BATCH], outw, outh, opt)
            else:
                out = convert_mixed(crtlib, torch, [px for _, px in part], outw, outh, noise, hue, opt)
            for (name, _), pic in zip(part, out):
                write_ppm(os.path.join(out_dir, os.path.splitext(name)[0] + ".ppm"), pic)
            done += len(part)
            print("mixed sizes: %d stills in one call" % len(part))
        print("done: %d files" % done)
        return 0
    for (h, w), files in sorted(by_size.items()):
        for lo in range(0, len(files), MAX_BATCH):
            part = files[lo:lo + MAX_BATCH]
            out = convert_batch(crtlib, torch, np.stack([px for _, px in part]), outw, outh, noise, hue, opt)
            for (name, _), pic in zip(part, out):
                write_ppm(os.path.join(out_dir, os.path.splitext(name)[0] + ".ppm"), pic)
            done += len(part)
            print("%d x %d: %d stills" % (w, h, len(part)))
    print("done: %d files" % done)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

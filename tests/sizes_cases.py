"""The inputs of tests/test_sizes_cpu.py and tests/test_gpu_sizes.py (TEST INFRASTRUCTURE ONLY; numpy and the CPU checkers, no GPU,
no tests): batches whose fields differ in IMAGE SIZE (crthip_fieldpass_sizes, crthip_stills_sizes).

The contract is "a mixed-size call equals n calls at batch 1", so the checker's loop (checker_fields) runs one CRT per image: batch 1,
the image's own w and h, the image followed by its spare row -- its own bytes where the case sets CRTHIP_F_IMAGE_SPARE_ROW (the
reference reads row h for odd fields with h <= desth, crt_ntsc.c:263), a copy of row h - 1 where it does not (what the kernels read
then).  A checker is crtref.Oracle or crtref.RefLib; both go through the same function.

Every case is tiny (5..8 fields, 64x48 pictures) and holds the smallest shapes at which the size-dependent code can go wrong:
waves that straddle fields (every n >= 2: desth is 236 for NTSC, a wave is 64 rows), widths below / at / above destw in one batch,
every width at which the encoder takes another path (1, 3, 4, 7, 8, 15, 16, 17; 1279 and 1280 together), heights 1, 2, desth - 1,
desth, desth + 1 and beyond 2 * desth, odd and even fields with and without the spare row, and every way of laying the images out."""
import numpy as np

import crtref as R

OUTW, OUTH = 64, 48
DESTW, DESTH = 753, 236          # standard NTSC (crt_ntsc.c:132-133); asserted against crthip_params_finalize in test_sizes_cpu.py

# packing: how the images lie in the one buffer.  "packed" = back to back in field order, no slack (4-byte formats: every image is a
# multiple of 4 bytes); "descending" = back to back in REVERSE field order; "shared" = the last field names field 0's image;
# "odd" = 3-byte formats with a 1-byte gap in front (every offset odd or even as it falls); "mod8" = 4-byte formats, 4 bytes of
# slack in front of every second image so that offsets = 4 mod 8 occur
CASES = {
    # widths below, at and above destw in one batch; a wave (64 rows) straddles every field boundary
    "scale": dict(name="ntsc", fmt=R.FMT_BGRA, noise=24, spare=True, pack="packed",
                  sizes=[(96, 60), (753, 7), (1000, 9), (40, 30), (754, 5), (752, 3)]),
    # every width at which a path switches; 4-byte pixels, so widths below 4 send the whole batch down the bytewise path
    "narrow": dict(name="ntsc", fmt=R.FMT_RGBA, noise=12, spare=False, pack="packed",
                   sizes=[(1, 8), (3, 5), (4, 6), (7, 3), (8, 8), (15, 2), (16, 4), (17, 7)]),
    # ... and from 4 on, so the cooperative tiles run them (w_min >= 4)
    "tiles": dict(name="ntsc", fmt=R.FMT_ARGB, noise=12, spare=True, pack="mod8",
                  sizes=[(4, 6), (7, 3), (8, 8), (15, 2), (16, 4), (17, 7), (33, 5)]),
    # 1279 and 1280 in one batch (the narrow image tile), and a batch of wide images only (the wide tile)
    "wide_mixed": dict(name="ntsc", fmt=R.FMT_BGRA, noise=0, spare=False, pack="descending",
                       sizes=[(1279, 4), (1280, 3), (640, 8), (1281, 2), (2000, 1)]),
    "wide_only": dict(name="ntsc", fmt=R.FMT_ABGR, noise=24, spare=True, pack="packed",
                      sizes=[(1280, 3), (1311, 2), (1920, 4), (1281, 5), (2561, 1)]),
    # heights around desth, odd and even fields, with the spare row (row h is read) and without (row h - 1)
    "heights_spare": dict(name="ntsc", fmt=R.FMT_BGRA, noise=24, spare=True, pack="packed",
                          sizes=[(8, 1), (5, 2), (6, DESTH - 1), (4, DESTH), (9, DESTH + 1), (4, 2 * DESTH + 29), (12, 1)]),
    "heights_tight": dict(name="ntsc", fmt=R.FMT_BGRA, noise=24, spare=False, pack="shared",
                          sizes=[(8, 1), (5, 2), (6, DESTH - 1), (4, DESTH), (9, DESTH + 1), (4, 2 * DESTH + 29), (8, 1)]),
    # 3-byte formats at odd offsets
    "rgb_odd": dict(name="ntsc", fmt=R.FMT_RGB, noise=24, spare=False, pack="odd",
                    sizes=[(5, 3), (33, 7), (1, 1), (754, 2), (16, 9)]),
    "bgr_spare": dict(name="ntsc", fmt=R.FMT_BGR, noise=0, spare=True, pack="odd",
                      sizes=[(7, 5), (2, 240), (100, 3), (3, 3), (1300, 2)]),
    # one case per system and build
    "vhs": dict(name="vhs", fmt=R.FMT_BGRA, noise=12, spare=True, pack="packed", seeds=[3, 14, 25, 36, 47],
                sizes=[(64, 48), (17, 9), (300, 5), (8, 100), (96, 240)]),
    "vhslcg": dict(name="vhslcg", fmt=R.FMT_BGRA, noise=24, spare=True, pack="packed",
                   sizes=[(64, 48), (17, 9), (300, 5), (8, 100), (96, 240)]),
    "snes": dict(name="snes", fmt=R.FMT_RGBA, noise=24, spare=True, pack="packed",
                 sizes=[(256, 22), (17, 9), (300, 5), (8, 100), (512, 3)]),
    "temp": dict(name="temp", fmt=R.FMT_BGRA, noise=24, spare=True, pack="descending",
                 sizes=[(64, 48), (17, 9), (300, 5), (8, 100), (900, 2)]),
    "nesrgb": dict(name="nesrgb", fmt=R.FMT_BGRA, noise=24, spare=True, pack="packed",
                   sizes=[(256, 24), (17, 9), (300, 5), (8, 250), (700, 3)]),
    "pv1k": dict(name="pv1k", fmt=R.FMT_BGRA, noise=12, spare=True, pack="packed",
                 sizes=[(64, 48), (17, 9), (300, 5), (8, 100), (1290, 2)]),
    "ntscp0": dict(name="ntscp0", fmt=R.FMT_BGRA, noise=24, spare=True, pack="mod8",
                   sizes=[(64, 48), (17, 9), (300, 5), (8, 100), (96, 240)]),
    "bloom": dict(name="ntscbloom", fmt=R.FMT_BGRA, noise=24, spare=True, pack="packed",
                  sizes=[(64, 48), (17, 9), (637, 5), (8, 100), (96, 240)]),
    "fir7": dict(name="ntscfir7", fmt=R.FMT_BGRA, noise=24, spare=True, pack="packed",
                 sizes=[(64, 48), (17, 9), (300, 5), (8, 100)]),
    # finished stills (crthip_stills_sizes): the CLI's accumulate loop, blend = scanlines = 1; noise 0 = the shared clean signal
    "stills0": dict(name="ntsc", fmt=R.FMT_BGRA, noise=0, spare=True, pack="packed", crt_knobs=dict(blend=1),
                    sizes=[(64, 48), (17, 9), (300, 5), (8, 100), (96, 240)]),
    "stills12": dict(name="ntsc", fmt=R.FMT_BGRA, noise=12, spare=True, pack="packed", crt_knobs=dict(blend=1),
                     sizes=[(64, 48), (17, 9), (300, 5), (8, 100), (96, 240)]),
    # enough fields for two overlap chunks (crthip_set_overlap: 256 fields per chunk at least): 520 fields over 8 distinct
    # (size, image, parity) combinations -- field k is field k % 8 again, so the checkers run 8 CRTs
    "many": dict(name="ntsc", fmt=R.FMT_BGRA, noise=24, spare=True, pack="packed", distinct=8,
                 sizes=[[(64, 48), (17, 9), (300, 5), (8, 100), (96, 240), (4, 4), (760, 2), (31, 31)][k % 8] for k in range(520)]),
}
STEPS = 2


def bpp(case):
    return R.bpp4fmt(CASES[case]["fmt"])


def parity(k):
    """(field, frame) of field k before the first pass: the recipe of the parity tests"""
    return k & 1, (k >> 1) & 1


def dot_crawl(name, k):
    return (2 * k + 1) % 6 if name.startswith(("pv1k", "temp")) else (k + 1) % 3


def image(case, k):
    """image k of a case WITH the row behind it: (h + 1, w, bpp).  Rows 0 .. h - 1 are the image; row h is the spare row -- bytes
    of its own where the case has the flag, a copy of row h - 1 where it has not (there it exists for the checkers only)."""
    c = CASES[case]
    w, h = c["sizes"][k]
    k %= c.get("distinct", len(c["sizes"]))
    img = R.synth_image(w, h + 1, bpp(case), 4242 + 31 * k + 1000 * sorted(CASES).index(case), "random" if k % 3 else "bars")
    if not c["spare"]:
        img[h] = img[h - 1]
    return img


def layout(case):
    """(buffer, sizes): the one uint8 buffer a sizes call reads and the (n, 3) int64 array of (w, h, byte offset).  No byte of slack
    behind the last image: the buffer ends where the furthest image (and its spare row, where the case has one) ends."""
    c = CASES[case]
    n, b = len(c["sizes"]), bpp(case)
    spare = 1 if c["spare"] else 0
    order = list(range(n))
    if c["pack"] == "descending":
        order.reverse()
    stored = order[:-1] if c["pack"] == "shared" else order
    off, offs, chunks = 0, {}, []
    for i, k in enumerate(stored):
        gap = 0
        if c["pack"] == "odd":
            gap = 1 if i % 2 == 0 else 0
        elif c["pack"] == "mod8":
            gap = (4 - off) % 8 if i % 2 == 0 else 0
        if gap:
            chunks.append(np.full(gap, 0xA5, dtype=np.uint8))
            off += gap
        w, h = c["sizes"][k]
        data = image(case, k)[:h + spare].reshape(-1)
        offs[k] = off
        chunks.append(data)
        off += data.size
    if c["pack"] == "shared":
        assert c["sizes"][n - 1] == c["sizes"][0]
        offs[n - 1] = offs[0]
    sizes = np.array([(c["sizes"][k][0], c["sizes"][k][1], offs[k]) for k in range(n)], dtype=np.int64)
    return np.concatenate(chunks), sizes


def field_image(case, k):
    """what field k reads: its own image, or -- "shared" -- field 0's for the last field"""
    c = CASES[case]
    return image(case, 0 if c["pack"] == "shared" and k == len(c["sizes"]) - 1 else k)


def checker_fields(lib, case, steps=STEPS, schedule=None):
    """The loop a sizes call must equal: per field ONE CRT of `lib` (crtref.Oracle or crtref.RefLib) at batch 1 with the field's own
    w and h, `steps` field-passes with the interlaced parities of the parity tests -- or, `schedule` = [(field, frame, aux), ...], the
    passes of a stills call (blend and scanlines as the case's crt_knobs say).  Returns per field a list of per-pass dicts: inp, out,
    hsync, vsync, rn, ccf and -- the oracle only -- undefined (crtref.reads_past_inp)."""
    c = CASES[case]
    name = c["name"]
    is_orc = isinstance(lib, R.Oracle)
    dc = lib.system in R.DOT_CRAWL_SYSTEMS
    prog = lib.system in R.PROGRESSIVE_SYSTEMS
    res = []
    for k, (w, h) in enumerate(c["sizes"]):
        if k >= c.get("distinct", len(c["sizes"])):
            res.append(res[k % c["distinct"]])         # the same size, image and parities again (distinct is a multiple of 4)
            continue
        crt = lib.new_crt(OUTW, OUTH, R.FMT_BGRA)
        crt.set("scanlines", 1)
        for a, v in c.get("crt_knobs", {}).items():
            crt.set(a, v)
        img = field_image(case, k)
        crt.settings(img, format=c["fmt"], w=w, h=h)
        if not prog:
            crt.sset("raw", 0)
            crt.sset("as_color", 1)
        field, frame = parity(k)
        aux = dot_crawl(name, k) if dc else 0
        if "seeds" in c:
            lib.srand(c["seeds"][k])
        per = []
        for step in range(len(schedule) if schedule else steps):
            if schedule:
                field, frame, aux = schedule[step][0] & 1, schedule[step][1] & 1, schedule[step][2]
            if not prog:
                crt.sset("field", field)
                crt.sset("frame", frame)
            if dc:
                crt.sset("dot_crawl_offset", aux)
            crt.analog[:] = 0                          # batch semantics: every field-pass starts from a crt_init-clean analog[]
            if prog:
                crt.sset("field_initialized", 0)
            crt.modulate()
            hs_before = crt.get("hsync")
            if is_orc:
                crt.demodulate(c["noise"], trace=True)
            else:
                crt.demodulate(c["noise"])
            d = dict(inp=crt.inp.copy(), out=crt.out.copy(), hsync=crt.get("hsync"), vsync=crt.get("vsync"), rn=crt.get("rn"),
                     ccf=crt.ccf.copy())
            if is_orc:
                d["undefined"] = R.reads_past_inp(lib, crt.trace, crt.get("vsync"), hs_before)
            per.append(d)
            field ^= 1
            if step % 2 == 0:
                frame ^= 1
        res.append(per)
    return res

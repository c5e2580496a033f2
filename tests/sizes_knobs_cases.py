"""The inputs of tests/test_sizes_knobs_cpu.py and tests/test_gpu_sizes_knobs.py (TEST INFRASTRUCTURE ONLY; numpy and the CPU checkers,
no GPU, no tests): batches whose fields differ in IMAGE SIZE and in LOOK (crthip_fieldpass_sizes_knobs, crthip_stills_sizes_knobs).

A case takes its sizes, images, packing, format and system from a case of tests/sizes_cases.py (`base`) and adds one look per field:
rows of (noise, mon_hue, saturation[, brightness, contrast[, black_point, white_point[, hue]]]) -- the widths CRT.upload_knobs takes --
from the hue / level / picture-knob case modules.  The contract is "the call equals n calls of crthip_fieldpass at batch 1, each with
field k's size, image and eight values", so the checker's loop (checker_fields) runs one CRT per image with that image's w and h and
its row: struct CRT's hue / saturation / brightness / contrast / black_point / white_point, NTSC_SETTINGS.hue, crt_demodulate(noise_k).
A checker is crtref.Oracle or crtref.RefLib; both go through the same function.

Every case is tiny (5..8 fields, 64x48 pictures; `many`: 520 fields of 8 distinct ones for two overlap chunks).  desth is 236 and a
wave is 64 rows, so every n >= 2 has waves starting mid-batch."""
import numpy as np

import crtref as R
import hues_cases as HU
import knobs_cases as KC
import levels_cases as LV
import picknobs_cases as PK
import sizes_cases as SC

OUTW, OUTH = SC.OUTW, SC.OUTH
STEPS = 2
CRT_KNOBS = ("hue", "saturation", "brightness", "contrast", "black_point", "white_point")      # row[1:7], struct CRT's names
DEFAULTS = (0, 0, 10, 0, 180, 0, 100, 0)               # crt_init's look: what a row narrower than 8 leaves alone


def _n(base):
    return len(SC.CASES[base]["sizes"])


def _cycle(rows, n):
    return [tuple(int(v) for v in rows[k % len(rows)]) for k in range(n)]


def with_noise(rows, noise):
    ns = [noise] * len(rows) if isinstance(noise, int) else list(noise)
    assert len(ns) == len(rows)
    return [(int(z),) + tuple(r[1:]) for z, r in zip(ns, rows)]


COMBINED = HU.BATCHES["combined"]                      # the eight values at once: hues 405, -90, 33, -123, 180, 359, a clean field
HUES = [HU.D7 + (h,) for h in HU.HUES_A + HU.HUES_B]   # 0, +-1, 33, 90, 180, 359, +-360, 405, -90, -123


def _outside_bound(n):
    """n rows (n, 8), ONE field on the first value outside the encoder's fast-path bound -- |white| = 8192 in one batch, |ire_base| =
    8192 in the other (LV.bound_batches) -- so the whole call takes the exact SZ + LV instantiation"""
    out = {}
    for which in ("white+", "ire-"):
        rows = list(LV.bound_batches("ntsc")[which])
        rows += [LV.at("ntsc", noise=30, sat=12)] * (n - len(rows))
        out[which] = [tuple(int(v) for v in r) + (h,) for r, h in zip(rows, (0, -123, 405, 33, 359, -45, 77))]
    return out


CASES = {
    # widths on every path switch with (n, 8) looks: below 4 (bytewise), from 4 on (narrow tile), 1279 and 1280 together, wide only
    "narrow8": dict(base="narrow", rows=_cycle(COMBINED + HUES[:2], _n("narrow"))),
    "tiles8": dict(base="tiles", rows=_cycle(HUES[5:] + COMBINED[:1], _n("tiles"))),
    "wide_mixed8": dict(base="wide_mixed", rows=_cycle(COMBINED[1:], _n("wide_mixed"))),
    "wide_only8": dict(base="wide_only", rows=_cycle(COMBINED, _n("wide_only"))),
    "scale8": dict(base="scale", rows=_cycle(COMBINED, _n("scale"))),
    # one field just outside the fast-path level bound
    "bound_white": dict(base="scale", rows=_outside_bound(_n("scale"))["white+"]),
    "bound_ire": dict(base="tiles", rows=_outside_bound(_n("tiles"))["ire-"]),
    # hues including negatives and +-360, 3-byte pixels at odd offsets
    "hues": dict(base="rgb_odd", rows=_cycle(HUES[6:] + HUES[1:3], _n("rgb_odd"))),
    # noise 0 everywhere: no KN instantiation (and, as stills, the shared clean signal)
    "clean8": dict(base="heights_spare", rows=with_noise(_cycle(COMBINED, _n("heights_spare")), 0)),
    "clean3": dict(base="scale", rows=with_noise(_cycle(KC.SMALL_TRIPLES, _n("scale")), 0)),
    # one noisy field among clean ones
    "one_noisy": dict(base="scale", rows=with_noise(_cycle(COMBINED, _n("scale")), [0, 0, 24, 0, 0, 0])),
    # the record widths
    "rows3": dict(base="scale", rows=_cycle(KC.SMALL_TRIPLES, _n("scale"))),
    "rows5": dict(base="heights_tight", rows=_cycle(PK.ALL_FIVE, _n("heights_tight"))),
    "rows7": dict(base="bgr_spare", rows=_cycle(LV.COMBINED, _n("bgr_spare"))),
    # hues bound, levels not: p->white and p->ire_base apply (rows keep black point 0 and white point 100)
    "hue_only": dict(base="scale", rows=_cycle(HU.BATCHES["straddle"], _n("scale")), hue_only=True),
    "hue_only_clean": dict(base="scale", rows=with_noise(_cycle(HU.BATCHES["straddle"], _n("scale")), 0), hue_only=True),
    # every field names ONE image, under n looks (a contact sheet)
    "one_image": dict(base="scale", rows=_cycle(COMBINED, _n("scale")), one_image=True),
    # one case per system and build
    "vhs": dict(base="vhs", rows=_cycle(HU.per_system("vhs", 5), _n("vhs"))),
    "vhslcg": dict(base="vhslcg", rows=_cycle(HU.per_system("vhslcg", 5), _n("vhslcg"))),
    "snes": dict(base="snes", rows=_cycle(HU.per_system("snes", 5), _n("snes"))),
    "temp": dict(base="temp", rows=_cycle(HU.per_system("temp", 5), _n("temp"))),
    "nesrgb": dict(base="nesrgb", rows=_cycle(HU.per_system("nesrgb", 5), _n("nesrgb"))),
    "ntscp0": dict(base="ntscp0", rows=_cycle(HU.per_system("ntscp0", 5), _n("ntscp0"))),
    "bloom": dict(base="bloom", rows=_cycle([(24, 0, 10), (0, 17, 14), (30, -20, 12), (24, 350, 40), (60, 77, 13)], _n("bloom"))),
    "fir7": dict(base="fir7", rows=_cycle(LV.STRADDLE, _n("fir7"))),
    # finished stills (blend = scanlines = 1, SC.CASES["stills0"]): every still clean = the shared signal; one noisy still = per pass
    "stills_clean": dict(base="stills0", rows=with_noise(_cycle(COMBINED, _n("stills0")), 0)),
    "stills_one_noisy": dict(base="stills0", rows=with_noise(_cycle(COMBINED, _n("stills0")), [0, 24, 0, 0, 0])),
    # two overlap chunks: 520 fields, field k is field k % 8 again (size, image, parity AND look)
    "many": dict(base="many", rows=_cycle(COMBINED + HUES[9:11], _n("many"))),
}


def base(case):
    return SC.CASES[CASES[case]["base"]]


def rows8(case):
    """the case's rows widened to the eight values with crt_init's defaults"""
    return [tuple(r) + DEFAULTS[len(r):] for r in CASES[case]["rows"]]


def noise_max(case):
    return max(r[0] for r in CASES[case]["rows"])


def layout(case):
    """(buffer, sizes) as SC.layout; `one_image`: the buffer is field 0's image alone and every field names it"""
    c = CASES[case]
    if not c.get("one_image"):
        return SC.layout(c["base"])
    b = base(case)
    w, h = b["sizes"][0]
    data = SC.image(c["base"], 0)[:h + (1 if b["spare"] else 0)].reshape(-1)
    return data.copy(), np.array([(w, h, 0)] * len(c["rows"]), dtype=np.int64)


def field_size(case, k):
    return base(case)["sizes"][0 if CASES[case].get("one_image") else k]


def field_image(case, k):
    return SC.image(CASES[case]["base"], 0) if CASES[case].get("one_image") else SC.field_image(CASES[case]["base"], k)


def checker_fields(lib, case, steps=STEPS, schedule=None):
    """The loop the call must equal: per field ONE CRT of `lib` at batch 1 with the field's own w, h, image and look; `steps`
    field-passes with the interlaced parities of the parity tests, or the passes of `schedule` = [(field, frame, aux), ...].  Returns
    per field a list of per-pass dicts: inp, out, hsync, vsync, rn, ccf and -- the oracle only -- undefined (crtref.reads_past_inp)."""
    c, b = CASES[case], base(case)
    name = b["name"]
    is_orc = isinstance(lib, R.Oracle)
    dc = lib.system in R.DOT_CRAWL_SYSTEMS
    prog = lib.system in R.PROGRESSIVE_SYSTEMS
    distinct = b.get("distinct", len(c["rows"]))
    res = []
    for k, row in enumerate(rows8(case)):
        if k >= distinct:
            assert row == rows8(case)[k % distinct]
            res.append(res[k % distinct])
            continue
        w, h = field_size(case, k)
        crt = lib.new_crt(OUTW, OUTH, R.FMT_BGRA)
        crt.set("scanlines", 1)
        for a, v in b.get("crt_knobs", {}).items():
            crt.set(a, v)
        for a, v in zip(CRT_KNOBS, row[1:7]):
            crt.set(a, v)
        crt.settings(field_image(case, k), format=b["fmt"], w=w, h=h)
        if not prog:
            crt.sset("raw", 0)
            crt.sset("as_color", 1)
        field, frame = SC.parity(k)
        aux = SC.dot_crawl(name, k) if dc else 0
        if "seeds" in b:
            lib.srand(b["seeds"][k])
        per = []
        for step in range(len(schedule) if schedule else steps):
            if schedule:
                field, frame, aux = schedule[step][0] & 1, schedule[step][1] & 1, schedule[step][2]
            if not prog:
                crt.sset("field", field)
                crt.sset("frame", frame)
            if dc:
                crt.sset("dot_crawl_offset", aux)
            crt.sset("hue", row[7])
            crt.analog[:] = 0                          # batch semantics: every field-pass starts from a crt_init-clean analog[]
            if prog:
                crt.sset("field_initialized", 0)
            crt.modulate()
            hs_before = crt.get("hsync")
            if is_orc:
                crt.demodulate(row[0], trace=True)
            else:
                crt.demodulate(row[0])
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

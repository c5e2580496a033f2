"""Cases of tests/test_gpu_fence.py (and their CPU-side checks in tests/test_fence_cpu.py): every entry point on fenced buffers
(tests/fence.py) with loose strides and offset bases.  A case is a dict; `expected(case)` runs the oracle ONCE per case (cached) on
the case's own inputs, which depend on nothing but the case -- never on the fill seed of a run.

Geometry of a case:
  img = (stride, base_off, spare_row): stride "tight", "row" (tight + one row) or tight + that many bytes; base_off bytes from the
        allocation's aligned start; spare_row True = a DEFINED row h behind every image (CRTHIP_F_IMAGE_SPARE_ROW), False = whatever
        lies there is poison and must not be read
  out = (extra stride bytes, base_off)
"""
import numpy as np

import crtref as R
from test_phosphor_cpu import display_step_np

OUT_SEED, ANALOG_SEED, SPARE_SEED, INIT_SEED = 4242, 9191, 606, 5
FILL_SEEDS = (20261019, 77003)                # the two runs of every case: everything OUTSIDE the payloads


def C(id, kind="fieldpass", name="ntsc", w=64, h=48, ifmt=R.FMT_BGRA, outw=33, outh=241, ofmt=R.FMT_BGRA, noise=24, n=3,
      skw=None, knobs=None, shape=1, layout=1, tile=0, lpw=0, exact=False, mode="keep", img=("tight", 0, False), out=(0, 0),
      set_first=None, init="none", triples=None, overlap=0, sched=None, vhs_streams=False):
    return dict(id=id, kind=kind, name=name, w=w, h=h, ifmt=ifmt, outw=outw, outh=outh, ofmt=ofmt, noise=noise, n=n,
                skw=dict(skw or {}), knobs=dict(knobs or {}), shape=shape, layout=layout, tile=tile, lpw=lpw, exact=exact, mode=mode,
                img=img, out=out, set_first=set_first, init=init, triples=triples, overlap=overlap, sched=sched, vhs_streams=vhs_streams)


F4 = (R.FMT_ARGB, R.FMT_RGBA, R.FMT_ABGR, R.FMT_BGRA)
IMG4 = [("tight", 0, False), ("row", 4, True), (4, 8, False), (4100, 12, False)]
IMG3 = [("tight", 1, False), ("row", 2, True), (3, 3, False), (4100, 1, False)]
OUT4 = [(0, 0), (4, 4), (4096 + 20, 8), (4, 12)]
OUT3 = [(0, 1), (1, 2), (3, 3), (4096 + 20, 1)]


def _img(fmt, i):
    return (IMG4 if fmt in F4 else IMG3)[i % 4]


def _out(fmt, i):
    return (OUT4 if fmt in F4 else OUT3)[i % 4]


def _cases():
    cs = []
    # ---- strides and bases, all of them, on the lane-shape field-pass (4-byte and 3-byte pixels on both sides) ----
    for i in range(4):
        for j in range(4):
            if (i + j) % 2 == 0:
                cs.append(C("lane-bgra-img%d-out%d" % (i, j), w=17, h=7, img=IMG4[i], out=OUT4[j], knobs=dict(scanlines=j & 1)))
            else:
                cs.append(C("lane-rgb-img%d-out%d" % (i, j), w=17, h=7, ifmt=R.FMT_RGB, outw=101, outh=77, ofmt=R.FMT_RGB,
                            img=IMG3[i], out=OUT3[j], knobs=dict(blend=j & 1)))
    # ---- encoder: widths x heights x formats; stage-level modulate and the fused field-pass in both shapes and layouts ----
    enc = [(1, 1, R.FMT_BGRA), (3, 7, R.FMT_ARGB), (4, 48, R.FMT_BGRA), (5, 7, R.FMT_ARGB), (17, 1, R.FMT_RGB), (64, 48, R.FMT_RGB),
           (1281, 7, R.FMT_BGRA), (1281, 48, R.FMT_ARGB), (5, 48, R.FMT_BGRA), (3, 1, R.FMT_RGB), (4, 7, R.FMT_ARGB), (1, 48, R.FMT_RGB)]
    for i, (w, h, fmt) in enumerate(enc):
        tag = "%dx%d-%s" % (w, h, {R.FMT_BGRA: "bgra", R.FMT_ARGB: "argb", R.FMT_RGB: "rgb"}[fmt])
        cs.append(C("enc-stage-" + tag, kind="stage", w=w, h=h, ifmt=fmt, img=_img(fmt, i), out=_out(R.FMT_BGRA, i + 1)))
        cs.append(C("enc-lane-" + tag, w=w, h=h, ifmt=fmt, img=_img(fmt, i + 1), out=_out(R.FMT_BGRA, i + 2), layout=i & 1))
        cs.append(C("enc-row-" + tag, w=w, h=h, ifmt=fmt, shape=2, img=_img(fmt, i + 2), out=_out(R.FMT_BGRA, i + 3), layout=1 - (i & 1)))
    for tile in (0, 32):
        cs.append(C("enc-tile%d-64x48" % tile, tile=tile, img=IMG4[2], out=OUT4[1]))
        cs.append(C("enc-tile%d-1281x7" % tile, w=1281, h=7, tile=tile, img=IMG4[3], out=OUT4[2]))
    # raw images on an odd field with h <= desth: the reference reads row h (crt_ntsc.c:263)
    for kind in ("stage", "fieldpass"):
        cs.append(C("raw-spare-row-" + kind, kind=kind, w=20, h=7, skw=dict(raw=1), img=("row", 4, True), out=OUT4[1]))
        cs.append(C("raw-poison-row-" + kind, kind=kind, w=20, h=7, skw=dict(raw=1), img=(4, 8, False), out=OUT4[3]))
        cs.append(C("raw-poison-row-rgb-" + kind, kind=kind, w=5, h=7, ifmt=R.FMT_RGB, skw=dict(raw=1), img=(3, 1, False), out=OUT4[0]))
    cs.append(C("nes-u16-stage", kind="stage", name="nes", w=256, h=240, img=(2, 2, False), out=OUT4[1], noise=12))
    cs.append(C("nes-u16-fused", name="nes", w=256, h=240, img=(2, 6, False), out=OUT4[2], noise=12))
    cs.append(C("pv1k-stage", kind="stage", name="pv1k", outw=64, outh=48, img=IMG4[2], out=OUT4[1], noise=12))
    cs.append(C("pv1k-fused", name="pv1k", outw=64, outh=48, img=IMG4[1], out=OUT4[3], noise=12))
    # ---- decoders: pictures ----
    pics = [(1, 1, R.FMT_RGB, {}), (1, 1, R.FMT_BGRA, {}), (3, 17, R.FMT_RGB, {}), (3, 17, R.FMT_BGRA, {}), (5, 240, R.FMT_RGB, {}),
            (5, 240, R.FMT_BGRA, {}), (33, 241, R.FMT_BGRA, {}), (101, 77, R.FMT_RGB, {}), (64, 120, R.FMT_ABGR, dict(v_fac=30))]
    for i, (ow, oh, fmt, kn) in enumerate(pics):
        tag = "%dx%d-%s" % (ow, oh, "rgb" if fmt == R.FMT_RGB else "4b")
        for shape, combos in ((1, ((0, 0), (1, 1))), (2, ((0, 1), (1, 0)))):
            for j, (blend, scan) in enumerate(combos):
                cs.append(C("dec-%s-%s-b%ds%d" % ("lane" if shape == 1 else "row", tag, blend, scan), kind="stage" if (i + j) % 3 == 0 else "fieldpass",
                            outw=ow, outh=oh, ofmt=fmt, shape=shape, knobs=dict(kn, blend=blend, scanlines=scan),
                            img=IMG4[(i + j) % 4], out=_out(fmt, i + j + shape)))
    for ow, oh in ((1650, 120), (1921, 241)):
        for lpw in (8, 16):
            # (no blend: crt_decode_wide_ok sends blended pictures to the lane decoder; tests/test_gpu_fence.py asserts the path taken)
            cs.append(C("dec-wide-%dx%d-lpw%d" % (ow, oh, lpw), outw=ow, outh=oh, lpw=lpw, n=2, knobs=dict(scanlines=int(lpw == 16)),
                        out=OUT4[1 + (lpw == 16)], img=IMG4[1]))
    cs.append(C("dec-lane-1650x120-blend", outw=1650, outh=120, lpw=16, n=2, knobs=dict(blend=1), out=OUT4[3], img=IMG4[2]))
    cs.append(C("dec-bloom-33x241-bgra", name="ntscbloom", out=OUT4[2], knobs=dict(blend=1)))
    cs.append(C("dec-bloom-101x77-rgb", name="ntscbloom", outw=101, outh=77, ofmt=R.FMT_RGB, out=OUT3[2], knobs=dict(scanlines=1)))
    cs.append(C("dec-exact-33x241", exact=True, out=OUT4[3], img=IMG4[3]))
    # ---- display and sequence kernels ----
    disp = [(3, 17, R.FMT_RGB), (33, 241, R.FMT_BGRA), (101, 77, R.FMT_RGB)]
    for i, (ow, oh, fmt) in enumerate(disp):
        for mode in ("fade", "clear"):
            for blend in (0, 1):
                cs.append(C("phos-%s-b%d-%dx%d" % (mode, blend, ow, oh), outw=ow, outh=oh, ofmt=fmt, mode=mode, knobs=dict(blend=blend),
                            out=_out(fmt, i + blend + (mode == "fade")), img=IMG4[(i + blend) % 4]))
    for i, mode in enumerate(("keep", "fade", "clear")):
        for blend in (0, 1):
            cs.append(C("seq-%s-b%d" % (mode, blend), kind="sequence", mode=mode, knobs=dict(blend=blend, v_fac=30), init="loose",
                        out=OUT4[(i + blend) % 4], img=IMG4[(i + 2 * blend) % 4]))
    ragged = [0, 1, 4, 5]
    for tag, ow, oh, fmt in (("pitch303", 101, 77, R.FMT_RGB), ("pitch132", 33, 241, R.FMT_BGRA)):
        for init in ("shared", "loose"):
            cs.append(C("sets-%s-%s" % (tag, init), kind="sets", outw=ow, outh=oh, ofmt=fmt, n=5, set_first=ragged, init=init,
                        knobs=dict(blend=1, scanlines=1, v_fac=240), mode="fade" if init == "shared" else "keep",
                        out=_out(fmt, 2 if init == "shared" else 3), img=IMG4[2]))
    cs.append(C("sets-3x2049-per-field", kind="sets", outw=3, outh=2049, ofmt=R.FMT_RGB, n=5, set_first=ragged, init="loose",
                knobs=dict(blend=1), out=OUT3[2], img=IMG4[1]))
    cs.append(C("sets-noblend-clear", kind="sets", n=5, set_first=ragged, init="shared", mode="clear", out=OUT4[1], img=IMG4[3]))
    cs.append(C("stills", kind="stills", knobs=dict(blend=1, scanlines=1), sched=[(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], noise=0,
                out=OUT4[2], img=IMG4[2]))
    trip = [(24, 0, 10), (0, 17, 14), (12, -20, 6)]
    cs.append(C("fieldpass-knobs", kind="fieldpass", triples=trip, out=OUT4[1], img=IMG4[1]))
    cs.append(C("sequence-knobs", kind="sequence", triples=trip, init="loose", out=OUT4[3], img=IMG4[2]))
    cs.append(C("vhs-fieldpass", name="vhs", noise=12, out=OUT4[1], img=IMG4[2], shape=0))
    cs.append(C("vhs-sets-streams", kind="sets", name="vhs", noise=12, n=5, set_first=ragged, init="loose", vhs_streams=True,
                out=OUT4[2], img=IMG4[1], shape=0))
    # the chunk loop offsets d_out by first * ostride: 512 fields is the smallest batch the library still cuts in two
    cs.append(C("overlap-chunks", w=1, h=1, outw=3, outh=17, ofmt=R.FMT_RGB, n=512, overlap=2, out=OUT3[1], img=(4, 4, False)))
    return cs


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)
VHS_SEEDS = [7, 1001, 424242, 5, 99]


def case(id):
    return CASES[CASE_IDS.index(id)]


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def is_nes(c):
    return R.SYSTEMS[c["name"]][0] == R.SYS_NES


def in_bpp(c):
    return 2 if is_nes(c) else R.bpp4fmt(c["ifmt"])


def image_row_bytes(c):
    return c["w"] * in_bpp(c)


def picture_row_bytes(c):
    return c["outw"] * R.bpp4fmt(c["ofmt"])


def image_layout(c):
    """(payload bytes, stride bytes, base_off, spare_row): the payload includes the defined spare row where there is one"""
    stride, base, spare = c["img"]
    row = image_row_bytes(c)
    tight = row * c["h"]
    payload = tight + (row if spare else 0)
    st = tight if stride == "tight" else tight + row if stride == "row" else tight + int(stride)
    if spare and st < payload:
        st = payload
    return payload, st, base, spare


def picture_layout(c):
    extra, base = c["out"]
    tight = picture_row_bytes(c) * c["outh"]
    return tight, tight + extra, base


def sets_of(c):
    sf = c["set_first"] or [0, c["n"]]
    return list(zip(sf[:-1], sf[1:]))


# ---- inputs (functions of the case alone) ---------------------------------------------------------------------------------------
def images(c):
    """[n, h (+1 with a spare row), w, bpp] uint8, or [n, h (+1), w] uint16 PPU pixels; the spare row is DEFINED and differs from
    row h - 1 (so a kernel that reads the wrong one of the two is caught)"""
    spare = c["img"][2]
    out = []
    for k in range(c["n"]):
        if is_nes(c):
            im = R.synth_ppu(c["w"], c["h"], 31 + k)
            extra = R.synth_ppu(c["w"], 1, SPARE_SEED + k)
        else:
            bpp = R.bpp4fmt(c["ifmt"])
            im = R.synth_image(c["w"], c["h"], bpp, 777 + 13 * (k % 7), "random" if k % 2 == 0 else "bars")
            extra = R.synth_image(c["w"], 1, bpp, SPARE_SEED + k)
        out.append(np.concatenate([im, extra], axis=0) if spare else im)
    return np.stack(out)


def oracle_image(c, imgs, k):
    """what the oracle is handed for field k: h + 1 rows -- the defined spare row, or (no spare row) row h - 1 again, which is what
    the library reads in place of the reference's row h (CRTHIP_F_IMAGE_SPARE_ROW)"""
    im = imgs[k]
    return im if c["img"][2] else np.concatenate([im, im[-1:]], axis=0)


def parity(k):
    return k & 1, (k >> 1) & 1


def dot_crawl(c, k):
    return (2 * k + 1) % 6 if c["name"].startswith("pv1k") else k % 3


def out_prefill(c):
    """the pictures d_out holds before the call, [n, outh * pitch]"""
    size = picture_layout(c)[0]
    return R.lcg_bytes(c["n"] * size, OUT_SEED).reshape(c["n"], size)


def analog_prefill(c, input_size):
    return R.lcg_bytes(c["n"] * input_size, ANALOG_SEED).view(np.int8).reshape(c["n"], input_size)


def init_pictures(c):
    """None, [1, bytes] (one picture shared by all sets / the single set) or [n_sets, bytes]"""
    size = picture_layout(c)[0]
    if c["init"] == "none":
        return None
    ns = 1 if (c["init"] == "shared" or c["kind"] == "sequence") else len(sets_of(c))
    return np.stack([R.lcg_bytes(size, INIT_SEED + 11 * s) for s in range(ns)])


def field_noise(c, k):
    return c["triples"][k][0] if c["triples"] else c["noise"]


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
def _new_crt(orc, c, out=None):
    crt = orc.new_crt(c["outw"], c["outh"], c["ofmt"], out)
    for key, v in c["knobs"].items():
        crt.set(key, v)
    return crt


def _settings(orc, c, crt, imgs, k, par, aux=None):
    im = oracle_image(c, imgs, k)
    if is_nes(c):
        crt.settings(im, w=c["w"], h=c["h"], dot_crawl_offset=dot_crawl(c, k) if aux is None else aux, hue=0)
        return
    crt.settings(im, format=c["ifmt"], w=c["w"], h=c["h"], field=par[0], frame=par[1], **dict(dict(as_color=1), **c["skw"]))
    if orc.system in R.DOT_CRAWL_SYSTEMS:
        crt.sset("dot_crawl_offset", dot_crawl(c, k) if aux is None else aux)


def _knobs_of_field(c, crt, k):
    if c["triples"]:
        crt.set("hue", c["triples"][k][1])
        crt.set("saturation", c["triples"][k][2])


def _demodulate(orc, c, crt, k, res):
    hs = crt.get("hsync")
    crt.demodulate(field_noise(c, k), trace=True)
    if R.reads_past_inp(orc, crt.trace, crt.get("vsync"), hs):
        res["excluded"].append(k)


_EXPECTED = {}


def expected(c):
    """dict: out [n, bytes]; state [n, 3] (hsync, vsync, rn); ccf [n, vper, ccs] (independent fields only); analog / inp [n, input_size]
    (kind "stage"; inp also for the fused kinds: crthip_fieldpass_signal); trace [n][lines, 9] (the oracle's line table); excluded: fields whose demodulate reads past inp[] in the REFERENCE (undefined there) -- must stay empty"""
    if c["id"] in _EXPECTED:
        return _EXPECTED[c["id"]]
    orc = R.Oracle(c["name"])
    imgs = images(c)
    n = c["n"]
    res = dict(out=[], state=[], ccf=[], analog=[], inp=[], trace=[], excluded=[], input_size=orc.input_size)
    vhs_rand = c["name"] == "vhs"
    if c["kind"] in ("fieldpass", "stage", "stills"):
        pre = out_prefill(c)
        apre = analog_prefill(c, orc.input_size) if c["kind"] == "stage" else None
        for k in range(n):
            crt = _new_crt(orc, c, pre[k].copy())
            if apre is not None:
                crt.analog[:] = apre[k]
            if vhs_rand:
                orc.srand(VHS_SEEDS[k % 5])
            passes = c["sched"] if c["kind"] == "stills" else [parity(k) + (None,)]
            for (fld, frm, aux) in passes:
                if c["mode"] != "keep":
                    crt.out[:] = display_step_np(crt.out, c["ofmt"], c["mode"])
                _settings(orc, c, crt, imgs, k, (fld, frm), aux)
                _knobs_of_field(c, crt, k)
                if c["kind"] != "stage":
                    crt.analog[:] = 0                      # the fused path starts every field from a crt_init-clean analog[]
                    if is_nes(c):
                        crt.sset("field_initialized", 0)
                crt.modulate()
                if c["kind"] == "stage":
                    res["analog"].append(crt.analog.copy())
                _demodulate(orc, c, crt, k, res)
            res["inp"].append(crt.inp.copy())
            res["trace"].append(crt.trace.copy())          # (of the last pass: what the line table holds after the call)
            res["out"].append(crt.out.copy())
            res["state"].append((crt.get("hsync"), crt.get("vsync"), crt.get("rn")))
            res["ccf"].append(crt.ccf.copy())
    else:
        init = init_pictures(c)
        for s, (lo, hi) in enumerate(sets_of(c)):
            crt = _new_crt(orc, c)
            if init is not None:
                crt.out[:] = init[s if init.shape[0] > 1 else 0]
            if vhs_rand:
                orc.srand(VHS_SEEDS[s % 5])
            for k in range(lo, hi):
                if c["mode"] != "keep":
                    crt.out[:] = display_step_np(crt.out, c["ofmt"], c["mode"])
                _settings(orc, c, crt, imgs, k, parity(k - lo))
                _knobs_of_field(c, crt, k)
                crt.modulate()
                _demodulate(orc, c, crt, k, res)
                res["out"].append(crt.out.copy())
                res["state"].append((crt.get("hsync"), crt.get("vsync"), crt.get("rn")))
    res["out"] = np.stack(res["out"])
    res["state"] = np.array(res["state"], dtype=np.int64)
    _EXPECTED[c["id"]] = res
    return res

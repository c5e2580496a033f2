"""Shared by tests/test_knobs_cpu.py and tests/test_gpu_knobs.py: the knob triples (noise, monitor hue, saturation) of the
crthip_fieldpass_knobs tests, their images, and the expected values -- the oracle run once per field with that field's knobs."""
import ctypes as C

import numpy as np

import crtref as R

SMALL = dict(w=64, h=48, outw=160, outh=120)
FULL = dict(w=640, h=480, outw=640, outh=480)

# six fields, six triples: noise 0 inside a noisy batch; saturation 900 / 40 / 13 / -70 and the hues test_gpu_parity.py's cases use
# to put lines into the exact tier, tier 1 and either side of tier 0's chroma bound -- the lines of one wavefront carry different tiers
SMALL_TRIPLES = [(24, 0, 10), (0, 17, 14), (30, -20, 900), (24, 350, 40), (110, 77, 13), (60, 725, -70)]


def drawn_triples(n, seed, noise_max=60, sat_lo=-20, sat_hi=45):
    """n triples from a fixed seed: every field another one (noise 0 .. noise_max, hue -400 .. 400, saturation sat_lo .. sat_hi)"""
    rng = np.random.RandomState(seed)
    t = np.stack([rng.randint(0, noise_max + 1, n), rng.randint(-400, 401, n), rng.randint(sat_lo, sat_hi + 1, n)], axis=1)
    t[n // 2, 0] = 0                                   # a clean field in the middle of the batch
    assert len({tuple(r) for r in t.tolist()}) == n
    return [tuple(int(v) for v in r) for r in t]


_IMAGES = {}


def image(geo, k, distinct=None):
    j = k if distinct is None else k % distinct
    key = (geo["w"], geo["h"], j)
    if key not in _IMAGES:
        _IMAGES[key] = R.synth_image(geo["w"], geo["h"], 4, 777 + 13 * j, "random" if j % 2 == 0 else "bars")
    return _IMAGES[key]


def ppu_image(k, distinct=None):
    j = k if distinct is None else k % distinct
    if ("ppu", j) not in _IMAGES:
        _IMAGES[("ppu", j)] = R.synth_ppu(256, 240, 900 + j)
    return _IMAGES[("ppu", j)]


def parity(k):
    return k & 1, (k >> 1) & 1


def dot_crawl(name, k):
    return (2 * k + 1) % 6 if name.startswith(("pv1k", "temp")) else (k + 1) % 3


def oracle_fields(name, geo, triples, steps=1, crt_knobs=None, seeds=None, distinct=None, fields=None):
    """Field k of a batch as n = 1 calls of the reference would give it: its own crt.hue, crt.saturation and noise (crt_main.c:351-391),
    `steps` field-passes in a row on its own CRT with the interlaced parities of the parity tests.  Returns, per field, a list of
    per-step dicts (inp, out, hsync, vsync, rn, ccf, trace, undefined).  seeds: the rand()-noise VHS build, one generator per field.
    fields: only these field indices (the others come back as None)."""
    libc = C.CDLL(None)
    orc = R.Oracle(name)
    nes = orc.system == R.SYS_NES
    dc = orc.system in R.DOT_CRAWL_SYSTEMS
    out = []
    for k, (noise, hue, sat) in enumerate(triples):
        if fields is not None and k not in fields:
            out.append(None)
            continue
        c = orc.new_crt(geo["outw"], geo["outh"], R.FMT_BGRA)
        c.set("scanlines", 1)
        for a, v in (crt_knobs or {}).items():
            c.set(a, v)
        c.set("hue", hue)
        c.set("saturation", sat)
        field, frame = parity(k)
        if nes:
            ppu = ppu_image(k, distinct)
            c.settings(np.concatenate([ppu, ppu[-1:]], axis=0), w=256, h=240, dot_crawl_offset=dot_crawl(name, k), hue=0)
        else:
            img = image(geo, k, distinct)
            c.settings(np.concatenate([img, img[-1:]], axis=0), format=R.FMT_BGRA, w=geo["w"], h=geo["h"], as_color=1)
            if orc.system not in R.PROGRESSIVE_SYSTEMS:
                c.sset("field", field)
                c.sset("frame", frame)
            if dc:
                c.sset("dot_crawl_offset", dot_crawl(name, k))
        if seeds is not None:
            libc.srand(seeds[k])
        per = []
        for step in range(steps):
            c.analog[:] = 0                            # batch semantics: every field-pass starts from a crt_init-clean analog[]
            if orc.system in R.PROGRESSIVE_SYSTEMS:
                c.sset("field_initialized", 0)
            c.modulate()
            hs_before = c.get("hsync")
            c.demodulate(noise, trace=True)
            per.append(dict(inp=c.inp.copy(), out=c.out.copy(), hsync=c.get("hsync"), vsync=c.get("vsync"), rn=c.get("rn"),
                            ccf=c.ccf.copy(), trace=c.trace.copy(),
                            undefined=R.reads_past_inp(orc, c.trace, c.get("vsync"), hs_before)))
            if not nes and orc.system not in R.PROGRESSIVE_SYSTEMS:
                field ^= 1
                if step % 2 == 0:
                    frame ^= 1
                c.sset("field", field)
                c.sset("frame", frame)
        out.append(per)
    return out

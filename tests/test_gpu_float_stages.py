"""The float filter stages of k_decode on the GPU: every case runs with the switch on and off (CRTHIP_DEC_FLOAT, read
when a context is created: fresh contexts), both runs against the CPU oracle -- out, hsync, vsync, rn, ccf, bit for bit -- and
against each other.  Shapes: one or two fields of a 64x48 image to a 64x48 picture.  A line is AV_LEN samples whatever the picture, so
the bias drift runs its full course and rounding ties occur about a hundred times per field; one field is four waves."""
import os

import numpy as np
import pytest

import crtref as R

pytestmark = pytest.mark.gpu

W, H = 64, 48
HS0 = [0, 3, 30, 60, 140, 300, 500, 700, 880, 892, 905, 909]      # the start states of test_wild_sync_states_against_the_oracle
VS0 = [0, 4, 9, 100, 180, 250, 255, 258, 261]


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def _case(name="ntsc", n=2, noise=24, knobs=None, skw=None, wild=False, steps=2, floats=1):
    """floats: what crthip_float_stages_used must say with the switch on"""
    return dict(name=name, n=n, noise=noise, knobs=knobs or {}, skw=skw or {}, wild=wild, steps=steps, floats=floats)


CASES = {
    # from lock, both field parities (fields 0 and 1 of the batch, swapped in the second pass)
    "ntsc-noise0": _case(noise=0),
    "ntsc-noise24": _case(noise=24),
    # wild sync states under heavy noise: burst amplitudes all over the place, so waves of tiers 2 / 3 (the other launch) and
    # float waves decode lines of the same fields
    "ntsc-wild-noise150": _case(n=12, noise=150, wild=True, steps=3),
    # between the two carrier envelopes (65 532 < |wave| <= 120 000): tier 1 of the integer stages
    "ntsc-saturation17": _case(knobs=dict(saturation=17)),
    "ntsc-saturation19-noise60": _case(noise=60, knobs=dict(saturation=19)),
    "nes": _case(name="nes"),                                   # default saturation: tier 1 by its burst level
    "snes": _case(name="snes"),
    "ntscp0": _case(name="ntscp0"),                             # the other coefficient set
    "ntscbloom": _case(name="ntscbloom"),
    "hue+": _case(knobs=dict(hue=17), skw=dict(hue=350)),
    "hue-": _case(knobs=dict(hue=-40), skw=dict(hue=30)),
    "brightness-300": _case(knobs=dict(brightness=-300)),
    # the envelope's edge: |bright| = |brightness - black level (7)| = 2600 = T0_BRIGHT_MAX
    "brightness+edge": _case(knobs=dict(brightness=2607, contrast=20)),
    "brightness-edge": _case(knobs=dict(brightness=-2593, contrast=400)),
    # verdict no (5 samples per chroma cycle): the integer stages, whatever the switch says
    "pv1k-verdict-no": _case(name="pv1k", floats=0),
    # beyond the edge the batch is tier 2: no float stages either
    "brightness-beyond": _case(knobs=dict(brightness=2608, contrast=20), floats=0),
}


def _images(case):
    n, nes = case["n"], case["name"] == "nes"
    uniq = min(n, 6)
    if nes:
        base = np.stack([R.synth_ppu(256, 240, 8100 + k) for k in range(uniq)]).astype(np.int16)
    else:
        base = np.stack([R.synth_image(W, H, 4, 8100 + k, "bars" if k % 3 == 1 else "random") for k in range(uniq)])
    return base, uniq


def _start(case, k):
    return (HS0[(k * 5 + 1) % len(HS0)], VS0[(k * 2) % len(VS0)]) if case["wild"] and k % 4 != 0 else (0, 0)


_ORACLE = {}


def _oracle(cid):
    """per step, per field: (out, hsync, vsync, rn, ccf), or None from the pass on in which the reference reads past inp[] + 16
    (crtref.reads_past_inp: undefined there).  Computed once per case and left alone."""
    if cid in _ORACLE:
        return _ORACLE[cid]
    case = CASES[cid]
    name, n, nes = case["name"], case["n"], case["name"] == "nes"
    base, uniq = _images(case)
    orc = R.Oracle(name)
    res = [[None] * n for _ in range(case["steps"])]
    for k in range(n):
        c = orc.new_crt(W, H, R.FMT_BGRA)
        c.set("scanlines", 1)
        for kk, v in case["knobs"].items():
            c.set(kk, v)
        hs, vs = _start(case, k)
        c.set("hsync", hs)
        c.set("vsync", vs)
        pad = np.concatenate([base[k % uniq], base[k % uniq][-1:]])
        field = k & 1
        for step in range(case["steps"]):
            if nes:
                c.settings(pad.astype(np.uint16), w=256, h=240, dot_crawl_offset=(k + step) % 3, hue=case["skw"].get("hue", 0))
                c.sset("field_initialized", 0)
            else:
                c.settings(pad, format=R.FMT_BGRA, w=W, h=H, as_color=1, field=field ^ (step & 1), frame=0, **case["skw"])
                if orc.system in R.DOT_CRAWL_SYSTEMS:
                    c.sset("dot_crawl_offset", (k + step) % 3)
            c.analog[:] = 0                                    # batch semantics: every field-pass starts from a clean analog[]
            c.modulate()
            hs_before = c.get("hsync")
            c.demodulate(case["noise"], trace=True)
            if R.reads_past_inp(orc, c.trace, c.get("vsync"), hs_before):
                break
            res[step][k] = (c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn"), np.array(c.ccf).copy(), orc.vper, orc.ccs)
    _ORACLE[cid] = res
    return res


def _context(crtlib, case, dec_float):
    saved = os.environ.get("CRTHIP_DEC_FLOAT")
    os.environ["CRTHIP_DEC_FLOAT"] = "1" if dec_float else "0"
    try:
        g = crtlib.CRT(case["n"], W, H, crtlib.FMT_BGRA, case["name"], device=0)
    finally:
        if saved is None:
            del os.environ["CRTHIP_DEC_FLOAT"]
        else:
            os.environ["CRTHIP_DEC_FLOAT"] = saved
    g.set_shape(1)                                             # lane-per-scanline: the shape whose kernel this is about
    g.scanlines = 1
    for k, v in case["knobs"].items():
        setattr(g, k, v)
    return g


def _settings(crtlib, case, data, step):
    n, name = case["n"], case["name"]
    if name == "nes":
        return crtlib.Settings(data, hue=case["skw"].get("hue", 0), dot_crawl_offset=[(k + step) % 3 for k in range(n)])
    kw = dict(format=crtlib.FMT_BGRA, field=[(k & 1) ^ (step & 1) for k in range(n)], frame=0, **case["skw"])
    if R.Oracle(name).system in R.DOT_CRAWL_SYSTEMS:
        kw["dot_crawl_offset"] = [(k + step) % 3 for k in range(n)]
    return crtlib.Settings(data, **kw)


def _device_images(case):
    import torch
    base, uniq = _images(case)
    imgs = torch.from_numpy(np.concatenate([base, base[:, -1:]], axis=1)).to("cuda:0")     # + the spare row
    reps = (case["n"] + uniq - 1) // uniq
    rep = imgs.repeat(reps, *([1] * (imgs.dim() - 1)))
    return rep[:case["n"], :base.shape[1]]


def _gpu(crtlib, case, dec_float):
    import torch
    n = case["n"]
    g = _context(crtlib, case, dec_float)
    data = _device_images(case)
    g.state[:, crtlib.ST_HSYNC] = torch.tensor([_start(case, k)[0] for k in range(n)], dtype=torch.int32, device="cuda:0")
    g.state[:, crtlib.ST_VSYNC] = torch.tensor([_start(case, k)[1] for k in range(n)], dtype=torch.int32, device="cuda:0")
    per, used = [], []
    for step in range(case["steps"]):
        g.fieldpass(_settings(crtlib, case, data, step), case["noise"])
        g.synchronize()
        used.append(g.float_stages_used())
        per.append((g.out.cpu().numpy().copy(), g.state.cpu().numpy().copy()))
    g.close()
    return per, used


def _compare(crtlib, cid, per, what):
    case = CASES[cid]
    want = _oracle(cid)
    excluded = set()
    for step in range(case["steps"]):
        out, st = per[step]
        for k in range(case["n"]):
            if want[step][k] is None:
                excluded.add(k)
                continue
            o_out, o_hs, o_vs, o_rn, o_ccf, vper, ccs = want[step][k]
            w = "%s %s step %d field %d" % (cid, what, step, k)
            assert (int(st[k][crtlib.ST_HSYNC]), int(st[k][crtlib.ST_VSYNC]), int(st[k][crtlib.ST_RN])) == (o_hs, o_vs, o_rn), w
            np.testing.assert_array_equal(st[k][crtlib.ST_CCF:crtlib.ST_CCF + 25].reshape(5, 5)[:vper, :ccs], o_ccf, err_msg=w + " ccf")
            np.testing.assert_array_equal(out[k].reshape(-1), o_out, err_msg=w + " out")
    return excluded


@pytest.mark.parametrize("cid", sorted(CASES))
def test_float_and_integer_stages_equal_the_oracle_and_each_other(crtlib, cid):
    case = CASES[cid]
    on, used_on = _gpu(crtlib, case, True)
    off, used_off = _gpu(crtlib, case, False)
    assert used_on == [case["floats"]] * case["steps"], "float stages with the switch on: %s" % used_on
    assert used_off == [0] * case["steps"], "float stages with the switch off: %s" % used_off
    excluded = _compare(crtlib, cid, on, "float")
    assert _compare(crtlib, cid, off, "integer") == excluded
    if not case["wild"]:
        assert not excluded, "a case from lock must exclude nothing (reads_past_inp): %s" % sorted(excluded)
    else:
        assert 2 * len(excluded) < case["n"], "fewer than half the fields may drop out: %s" % sorted(excluded)
    for step in range(case["steps"]):
        # the two runs against each other (but for the fields whose reference run is undefined: what lies behind inp[] is nobody's result)
        keep = [k for k in range(case["n"]) if k not in excluded]
        np.testing.assert_array_equal(on[step][0][keep], off[step][0][keep], err_msg="%s step %d: out, float against integer" % (cid, step))
        np.testing.assert_array_equal(on[step][1][keep], off[step][1][keep], err_msg="%s step %d: state, float against integer" % (cid, step))


def test_float_stages_bgr_output_and_wider_picture(crtlib):
    """the 3-byte instantiation of the float kernel, and a picture wider than one pixel tile with an odd width (101 x 77)"""
    import torch
    base = np.stack([R.synth_image(W, H, 4, 8200 + k, "random") for k in range(2)])
    imgs = torch.from_numpy(np.concatenate([base, base[:, -1:]], axis=1)).to("cuda:0")
    got = {}
    for dec_float in (1, 0):
        saved = os.environ.get("CRTHIP_DEC_FLOAT")
        os.environ["CRTHIP_DEC_FLOAT"] = str(dec_float)
        try:
            g = crtlib.CRT(2, 101, 77, crtlib.FMT_RGB, "ntsc", device=0)
        finally:
            if saved is None:
                del os.environ["CRTHIP_DEC_FLOAT"]
            else:
                os.environ["CRTHIP_DEC_FLOAT"] = saved
        g.set_shape(1)
        g.fieldpass(crtlib.Settings(imgs[:, :H], format=crtlib.FMT_BGRA, field=[0, 1], frame=0), 24)
        g.synchronize()
        assert g.float_stages_used() == dec_float
        got[dec_float] = g.out.cpu().numpy().copy()
        g.close()
    orc = R.Oracle("ntsc")
    for k in range(2):
        c = orc.new_crt(101, 77, R.FMT_RGB)
        c.settings(np.concatenate([base[k], base[k][-1:]]), format=R.FMT_BGRA, w=W, h=H, as_color=1, field=k, frame=0)
        c.modulate()
        c.demodulate(24)
        np.testing.assert_array_equal(got[1][k].reshape(-1), c.out, err_msg="float, field %d" % k)
        np.testing.assert_array_equal(got[0][k].reshape(-1), c.out, err_msg="integer, field %d" % k)


def test_float_stages_in_a_captured_graph(crtlib):
    """one graph-captured field-pass with the float stages, replayed twice, against the oracle"""
    import torch
    cid = "ntsc-noise24"
    case = CASES[cid]
    n = case["n"]
    g = _context(crtlib, case, True)
    g.reserve(n)
    side = torch.cuda.Stream()
    g.use_stream(side)
    data = _device_images(case)
    s0 = _settings(crtlib, case, data, 0)
    g._load_field_state(s0)
    torch.cuda.synchronize()
    state0 = g.state.clone()
    p0 = g.params(s0, case["noise"])
    g.fieldpass(s0, case["noise"], params=p0)                  # eager once: the cached tables exist before the capture
    g.synchronize()
    eager = g.out.clone()
    g.state.copy_(state0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.fieldpass(s0, case["noise"], params=p0)
    assert g.float_stages_used() == 1
    want = _oracle(cid)[0]
    for _ in range(2):
        g.state.copy_(state0)
        g.out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g.out, eager)
        out, st = g.out.cpu().numpy(), g.state.cpu().numpy()
        for k in range(n):
            np.testing.assert_array_equal(out[k].reshape(-1), want[k][0], err_msg="replayed field %d" % k)
            assert (int(st[k][crtlib.ST_HSYNC]), int(st[k][crtlib.ST_VSYNC]), int(st[k][crtlib.ST_RN])) == want[k][1:4]
    del graph
    g.close()

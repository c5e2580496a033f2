"""Decoder tier 1 and k_decode's float stages at the edge of the fused path's envelope: the cases of tests/envelope_cases.py --
encoder-made fields whose largest carrier amplitude lies within one |saturation| of 65 532, of B(noise, system) or of 120 000 -- bit
for bit against the CPU oracle (which tests/test_envelope_cpu.py pins to the real reference on the same cases): the noisy signal of
fieldpass_signal, picture, hsync, vsync, rn, ccf, tolerance 0, nothing left out; and against the reference's own bytes where
oracle/_ref holds the build.  Every shape is a 64 x 48 picture (or a 64-high one wide enough for the wide-run decoder), two fields."""
import os

import numpy as np
import pytest

import crtref as R
import envelope_cases as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def _device_images(imgs):
    """[n, h, w, ...] inside an allocation with one more row per image (the reference reads row h)"""
    import torch
    if imgs.dtype == np.uint16:
        imgs = imgs.view(np.int16)
    full = torch.from_numpy(np.concatenate([imgs, imgs[:, -1:]], axis=1)).to("cuda:0")
    return full[:, :imgs.shape[1]]


def _settings(crtlib, name, enc_hue, data, n, step, first=0):
    dco = [V.E.dco_of(name, first + k, step) for k in range(n)]
    if V.E.is_nes(name):
        return crtlib.Settings(data, hue=enc_hue, dot_crawl_offset=dco)
    return crtlib.Settings(data, format=V.OUTFMT, as_color=1, field=[V.E.field_of(first + k, step) for k in range(n)],
                           frame=[V.E.frame_of(first + k) for k in range(n)], hue=enc_hue, dot_crawl_offset=dco)


def _context(crtlib, name, n, geom, dec_float=None, shape=1, exact=0, layout=1, wide_lpw=0, **knobs):
    saved = os.environ.get("CRTHIP_DEC_FLOAT")
    if dec_float is not None:
        os.environ["CRTHIP_DEC_FLOAT"] = "1" if dec_float else "0"          # read when a context is created
    try:
        g = crtlib.CRT(n, geom[0], geom[1], geom[2], name, device=0)
    finally:
        if dec_float is not None:
            if saved is None:
                del os.environ["CRTHIP_DEC_FLOAT"]
            else:
                os.environ["CRTHIP_DEC_FLOAT"] = saved
    g.set_shape(shape)
    g.set_exact(exact)
    g.set_signal_layout(layout)
    g.set_wide_lpw(wide_lpw)
    for k, v in knobs.items():
        setattr(g, k, v)
    return g


GEOM = (V.OUTW, V.OUTH, V.OUTFMT)


def _run(crtlib, cid, geom=GEOM, system=None, **kw):
    """-> per pass (signal in the reference's layout, state, out), and float_stages_used per pass"""
    c = V.CASES[cid]
    name = system or c["name"]
    g = _context(crtlib, name, c["n"], geom, hue=c["mon_hue"], saturation=c["sat"], **kw)
    data = _device_images(V.images(cid))
    if c.get("starts"):                                       # a fused start state: written into the state before the first call
        import torch
        g.state[:, crtlib.ST_HSYNC] = torch.tensor([st[0] for st in c["starts"]], dtype=torch.int32, device="cuda:0")
        g.state[:, crtlib.ST_VSYNC] = torch.tensor([st[1] for st in c["starts"]], dtype=torch.int32, device="cuda:0")
    per, used = [], []
    for step in range(V.STEPS):
        g.fieldpass(_settings(crtlib, name, c["enc_hue"], data, c["n"], step), c["noise"])
        g.synchronize()
        used.append(g.float_stages_used())
        sig, _ = g.fieldpass_signal()
        per.append((sig.cpu().numpy()[:, :g.input_size].copy(), g.state.cpu().numpy().copy(), g.out.cpu().numpy().copy()))
    g.close()
    return per, used


def _check_field(crtlib, name, sig, st, out, o, what):
    orc = V.oracle(name)
    assert not o["undefined"], what + "no case excludes anything (reads_past_inp)"
    np.testing.assert_array_equal(sig, o["inp"], err_msg=what + "inp")
    assert (int(st[crtlib.ST_HSYNC]), int(st[crtlib.ST_VSYNC]), int(st[crtlib.ST_RN])) == (o["hsync"], o["vsync"], o["rn"]), what + "state"
    np.testing.assert_array_equal(st[crtlib.ST_CCF:crtlib.ST_CCF + 25].reshape(5, 5)[:orc.vper, :orc.ccs], o["ccf"], err_msg=what + "ccf")
    np.testing.assert_array_equal(out.reshape(-1), o["out"], err_msg=what + "out")


def _check(crtlib, cid, per, want, what):
    c = V.CASES[cid]
    for k in range(c["n"]):
        for step in range(V.STEPS):
            sig, st, out = per[step]
            _check_field(crtlib, c["name"], sig[k], st[k], out[k], want[k][step], "%s %s field %d pass %d: " % (cid, what, k, step))


_REF = {}


def _reference(cid):
    """the real reference's own results, where its build travels with the tree"""
    if cid not in _REF:
        name = V.CASES[cid]["name"]
        _REF[cid] = V.run_case(R.RefLib(name), cid) if R.have_ref(name) else None
    return _REF[cid]


def _floats_expected(crtlib, cid):
    """the library's own host-side verdict for the case's parameters (ntsc, ntscp0, snes, nes: yes -- test_gpu_float_stages.py)"""
    c = V.CASES[cid]
    img = V.images(cid)
    p = crtlib.make_params(c["name"], w=int(img.shape[2]), h=int(img.shape[1]), outw=V.OUTW, outh=V.OUTH, out_format=V.OUTFMT,
                           mon_hue=c["mon_hue"], saturation=c["sat"], noise=c["noise"], hue=c["enc_hue"])
    verdict = int(crtlib.float_stages(p)[0] == 1)
    assert verdict == 1 or c["name"] == "vhslcg"
    return verdict


@pytest.mark.parametrize("cid", sorted(V.CASES))
def test_envelope_cases_float_and_integer_stages(crtlib, cid):
    """fieldpass, lane per scanline, CRTHIP_DEC_FLOAT on and off on fresh contexts: both equal the oracle (and the reference) and
    each other, and the float kernel is the one that ran"""
    on, used_on = _run(crtlib, cid, dec_float=True)
    off, used_off = _run(crtlib, cid, dec_float=False)
    assert used_on == [_floats_expected(crtlib, cid)] * V.STEPS, "float stages with the switch on: %s" % used_on
    assert used_off == [0] * V.STEPS, "float stages with the switch off: %s" % used_off
    want = V.expected(cid)
    _check(crtlib, cid, on, want, "float")
    _check(crtlib, cid, off, want, "integer")
    if _reference(cid) is not None:
        _check(crtlib, cid, on, _reference(cid), "float against the reference")
    for step in range(V.STEPS):
        for a, b, f in zip(on[step], off[step], ("signal", "state", "out")):
            np.testing.assert_array_equal(a, b, err_msg="%s pass %d: %s, float against integer" % (cid, step, f))


VARIANTS = {"shape2": dict(shape=2), "exact1": dict(exact=1), "exact2": dict(exact=2), "flat": dict(layout=0)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("cid", sorted(V.CASES))
def test_envelope_cases_dispatch_variants(crtlib, cid, variant):
    """the scanline-parallel shape; the exact kernels everywhere and the 24-bit tier without the 64-bit-mad tiers (tier 1 lines then
    go to tier 2); the reference's flat signal layout"""
    per, _ = _run(crtlib, cid, **VARIANTS[variant])
    _check(crtlib, cid, per, V.expected(cid), variant)


# one case per bound and side of it (ntsc, the hostile images), and the tier-1-only fields of the other systems
PINNED = ["ntsc-noise0-lo-above-phase", "ntsc-noise0-B-below-runs", "ntsc-noise0-B-above-phase", "ntsc-noise0-t0-below-runs",
          "ntsc-noise0-t0-above-phase", "ntsc-noise24-lo-above-runs", "ntsc-noise24-B-above-phase", "vhslcg-noise60-B-above-phase"]


@pytest.mark.parametrize("cid", PINNED)
def test_envelope_cases_three_byte_output(crtlib, cid):
    geom = (V.OUTW, V.OUTH, R.FMT_RGB)
    per, _ = _run(crtlib, cid, geom=geom)
    _check(crtlib, cid, per, V.expected(cid, geom), "rgb")


@pytest.mark.parametrize("lpw", [8, 16])
@pytest.mark.parametrize("cid", PINNED[:5])
def test_envelope_cases_wide_run_decoder(crtlib, cid, lpw):
    """a picture 1700 wide takes the wide-run decoder for its tier-0 / 1 waves (both instantiations pinned): the lane decoder's float
    stages must not have run"""
    geom = (1700, V.OUTH, V.OUTFMT)
    per, used = _run(crtlib, cid, geom=geom, wide_lpw=lpw, dec_float=True)
    assert used == [0] * V.STEPS, "the wide-run decoder was not taken: float stages %s" % used
    _check(crtlib, cid, per, V.expected(cid, geom), "wide lpw %d" % lpw)


_BLOOM = {}


@pytest.mark.parametrize("cid", ["ntsc-noise0-B-below-random", "ntsc-noise0-lo-above-random", "ntsc-noise24-B-above-phase"])
def test_envelope_tuples_on_the_bloom_build(crtlib, cid):
    """ntscbloom: the bloom decoder has no tier 1, its lines above 65 532 go to tier 2.  Same tuple and images; the burst, hence the
    amplitude, is the plain build's."""
    c = V.CASES[cid]
    if cid not in _BLOOM:
        _BLOOM[cid] = V.run_fields(V.oracle("ntscbloom"), "ntscbloom", list(V.images(cid)), c["noise"], c["enc_hue"], c["mon_hue"], c["sat"])
    want = _BLOOM[cid]
    assert max(int(V.amplitudes(r["trace"]).max()) for p in want for r in p) == c["amp"]
    per, _ = _run(crtlib, cid, system="ntscbloom")
    for k in range(c["n"]):
        for step in range(V.STEPS):
            sig, st, out = per[step]
            _check_field(crtlib, "ntscbloom", sig[k], st[k], out[k], want[k][step], "%s bloom field %d pass %d: " % (cid, k, step))


# ---------------------------------------------------------------------------------------------------------------------------
# the other fused entry points
# ---------------------------------------------------------------------------------------------------------------------------
_KNOB_WANT = {}


def _knob_fields(keys, family="phase"):
    """(n, 8) knobs -- noise, mon_hue, saturation, brightness, contrast, black_point, white_point, ENCODER hue -- of the tuples'
    fields side by side on one image family, the images, and per field the oracle's batch-of-one results [pass]"""
    rows, imgs, want, ks = [], [], [], []
    for key in keys:
        enc, mon, sat, amp = V.TUPLES[key]
        fam = [V.image(key[0], family, k) for k in range(V.N_FIELDS)]
        if key not in _KNOB_WANT:
            _KNOB_WANT[key] = V.run_fields(V.oracle(key[0]), key[0], fam, key[1], enc, mon, sat)
            assert max(int(V.amplitudes(r["trace"]).max()) for per in _KNOB_WANT[key] for r in per) == amp
        for k in range(V.N_FIELDS):
            rows.append((key[1], mon, sat, 0, 180, 0, 100, enc))
            imgs.append(fam[k])
            want.append(_KNOB_WANT[key][k])
            ks.append(k)
    return np.array(rows, dtype=np.int32), np.stack(imgs), want, ks


@pytest.mark.parametrize("keys", [(("ntsc", 0, "B", "below"), ("ntsc", 0, "B", "above"), ("ntsc", 24, "B", "below"), ("ntsc", 24, "B", "above")),
                                  (("ntsc", 0, "lo", "below"), ("ntsc", 0, "lo", "above"), ("ntsc", 24, "lo", "above"), ("ntsc", 0, "t0", "above"))],
                         ids=["B", "lo-t0"])
def test_fieldpass_knobs_straddles_fields_and_tiers(crtlib, keys):
    """fieldpass_knobs, one batch of 8 fields: the below and above tuples of a bound side by side (240 lines per field: the 64 lines of
    a wave straddle two fields and two tiers), noises 0 and 24 in one batch, so env.loskip_wave_max is the batch minimum B(24) -- every
    field must still equal its own batch-of-one oracle run, whose bound is the field's own"""
    knobs, imgs, want, ks = _knob_fields(keys)
    n = len(ks)
    assert n == 8
    g = _context(crtlib, "ntsc", n, GEOM)
    ones = [_context(crtlib, "ntsc", 1, GEOM) for _ in range(n)]       # the batch-1 loop on the GPU: each field under its OWN bound
    data = _device_images(imgs)
    for step in range(V.STEPS):
        s = crtlib.Settings(data, format=V.OUTFMT, as_color=1, field=[V.E.field_of(k, step) for k in ks],
                            frame=[V.E.frame_of(k) for k in ks], hue=0)
        g.fieldpass_knobs(s, knobs)
        g.synchronize()
        assert g._knob_env.loskip_wave_max == V.BOUNDS["ntsc"][24]
        sig = g.fieldpass_signal()[0].cpu().numpy()[:, :g.input_size]
        st, out = g.state.cpu().numpy(), g.out.cpu().numpy()
        for i in range(n):
            _check_field(crtlib, "ntsc", sig[i], st[i], out[i], want[i][step], "knobs field %d pass %d: " % (i, step))
            s1 = crtlib.Settings(data[i:i + 1], format=V.OUTFMT, as_color=1, field=V.E.field_of(ks[i], step), frame=V.E.frame_of(ks[i]),
                                 hue=0, spare_row=True)
            ones[i].fieldpass_knobs(s1, knobs[i:i + 1])
            ones[i].synchronize()
            assert ones[i]._knob_env.loskip_wave_max == V.BOUNDS["ntsc"][int(knobs[i, 0])]
            np.testing.assert_array_equal(ones[i].fieldpass_signal()[0].cpu().numpy()[0, :g.input_size], sig[i])
            np.testing.assert_array_equal(ones[i].state.cpu().numpy()[0], st[i], err_msg="field %d pass %d: state, batch of 8 against batch of 1" % (i, step))
            np.testing.assert_array_equal(ones[i].out.cpu().numpy()[0], out[i], err_msg="field %d pass %d: out, batch of 8 against batch of 1" % (i, step))
    g.close()
    for o in ones:
        o.close()


def _straddles(trace, b):
    """the field holds tier-1 lines (65 532 < amplitude <= B) and lines above B"""
    a = V.amplitudes(trace)
    return bool(((a > V.LOSKIP_WAVE_MAX) & (a <= b)).any() and (a > b).any())


def _sequence_oracle(n):
    """n consecutive fields of ONE television set on the oracle: state and picture carried over"""
    noise, fam, enc, mon, sat = V.SEQUENCE_TUPLE
    orc = V.oracle("ntsc")
    crt = orc.new_crt(*GEOM)
    crt.set("hue", mon)
    crt.set("saturation", sat)
    like = V._case_like("ntsc", enc)
    res = []
    for k in range(n):
        img = V.image("ntsc", fam, k % 2)
        crt.settings(np.concatenate([img, img[-1:]]), w=int(img.shape[1]), h=int(img.shape[0]), **V.E.settings_kw(like, k, 0))
        crt.analog[:] = 0
        crt.modulate()
        hs = crt.get("hsync")
        crt.demodulate(noise, trace=True)
        assert not R.reads_past_inp(orc, crt.trace, crt.get("vsync"), hs)
        assert _straddles(crt.trace, V.BOUNDS["ntsc"][noise]), "field %d of the sequence does not straddle B" % k
        res.append((crt.out.copy(), crt.get("hsync"), crt.get("vsync"), crt.get("rn")))
    return res


def test_sequence_on_an_above_B_tuple(crtlib):
    """crthip_sequence: four consecutive fields of one set, tier-1 lines and lines above B in every field (asserted on the oracle's
    trace)"""
    n = 4
    noise, fam, enc, mon, sat = V.SEQUENCE_TUPLE
    want = _sequence_oracle(n)
    g = _context(crtlib, "ntsc", n, GEOM, hue=mon, saturation=sat)
    imgs = np.stack([V.image("ntsc", fam, k % 2) for k in range(n)])
    s = crtlib.Settings(_device_images(imgs), format=V.OUTFMT, as_color=1, field=[V.E.field_of(k, 0) for k in range(n)],
                        frame=[V.E.frame_of(k) for k in range(n)], hue=enc)
    g.sequence(s, noise)
    g.synchronize()
    st, out = g.state.cpu().numpy(), g.out.cpu().numpy()
    for k in range(n):
        assert (int(st[k][crtlib.ST_HSYNC]), int(st[k][crtlib.ST_VSYNC]), int(st[k][crtlib.ST_RN])) == want[k][1:], "field %d" % k
        np.testing.assert_array_equal(out[k].reshape(-1), want[k][0], err_msg="sequence field %d" % k)
    g.close()


def test_stills_on_an_above_B_tuple_shared_signal(crtlib):
    """crthip_stills at noise 0 (every distinct schedule entry is encoded once and shared by its passes), two stills; every pass of
    either still holds tier-1 lines and lines above B (asserted on the oracle's trace)"""
    noise, fam, enc, mon, sat = V.STILLS_TUPLE
    assert noise == 0
    sched = crtlib.stills_schedule(True, 0, 2)
    orc = V.oracle("ntsc")
    like = V._case_like("ntsc", enc)
    imgs = np.stack([V.image("ntsc", fam, k) for k in range(2)])
    g = _context(crtlib, "ntsc", 2, GEOM, hue=mon, saturation=sat)
    g.stills(crtlib.Settings(_device_images(imgs), format=V.OUTFMT, as_color=1, hue=enc), 0, schedule=sched)
    g.synchronize()
    st, out = g.state.cpu().numpy(), g.out.cpu().numpy()
    for k in range(2):
        crt = orc.new_crt(*GEOM)
        crt.set("hue", mon)
        crt.set("saturation", sat)
        for field, frame, _aux in sched:
            kw = V.E.settings_kw(like, 0, 0)
            kw.update(field=field, frame=frame)
            crt.settings(np.concatenate([imgs[k], imgs[k][-1:]]), w=int(imgs.shape[2]), h=int(imgs.shape[1]), **kw)
            crt.analog[:] = 0
            crt.modulate()
            crt.demodulate(0, trace=True)
            assert _straddles(crt.trace, V.BOUNDS["ntsc"][0]), "still %d, pass (%d, %d) does not straddle B" % (k, field, frame)
        assert (int(st[k][crtlib.ST_HSYNC]), int(st[k][crtlib.ST_VSYNC]), int(st[k][crtlib.ST_RN])) == \
               (crt.get("hsync"), crt.get("vsync"), crt.get("rn")), "still %d" % k
        np.testing.assert_array_equal(out[k].reshape(-1), crt.out, err_msg="still %d" % k)
    g.close()

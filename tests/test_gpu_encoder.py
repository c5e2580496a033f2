"""The encoder (crt_encode.hip) on the hand-made images and knob edges of tests/encoder_cases.py, bit for bit against the CPU oracle
(which tests/test_encoder_cpu.py pins to the real reference on the same cases, and which proves what each case reaches).

Every case runs with set_exact(0) and set_exact(1): both must equal the oracle and each other.
* stage level (modulate): analog[:input_size] and the ccf after modulate -- nothing left out;
* fused (fieldpass / fieldpass_knobs): fieldpass_signal()[:input_size] against the oracle's inp, and rn -- nothing left out; the
  picture, hsync, vsync and ccf wherever crtref.reads_past_inp is false, which outside the noise-edge cases (|noise| >= 32767) must be
  everywhere."""
import numpy as np
import pytest

import crtref as R
import encoder_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def _device_images(cid):
    """[n, h, w, ...] inside an allocation with one more row per image (the reference reads row h, crt_ntsc.c:263)"""
    import torch
    imgs = E.images(cid)
    if imgs.dtype == np.uint16:
        imgs = imgs.view(np.int16)
    full = torch.from_numpy(np.concatenate([imgs, imgs[:, -1:]], axis=1)).to("cuda:0")
    return full[:, :imgs.shape[1]]


def _settings(crtlib, case, data, step):
    n, name = case["n"], case["name"]
    dco = [E.dco_of(name, k, step) for k in range(n)]
    if E.is_nes(name):
        return crtlib.Settings(data, hue=case["hue"], dot_crawl_offset=dco)
    return crtlib.Settings(data, format=case["fmt"], raw=case["raw"], as_color=1, field=[E.field_of(k, step) for k in range(n)],
                           frame=[E.frame_of(k) for k in range(n)], hue=case["hue"], xoffset=case["xoffset"], dot_crawl_offset=dco)


def _context(crtlib, cid, exact, shape=1, tile=0, layout=1):
    case = E.CASES[cid]
    g = crtlib.CRT(case["n"], E.OUTW, E.OUTH, E.OUTFMT, case["name"], device=0)
    g.set_shape(shape)
    g.set_exact(exact)
    g.set_signal_tile(tile)
    g.set_signal_layout(layout)
    for k, v in case["knobs"].items():
        setattr(g, k, v)
    if case["name"] in E.RAND_BUILDS:
        g.srand(list(E.SEEDS[:case["n"]]))
    return g


def _stage(crtlib, cid, exact, **kw):
    """-> per pass (analog, ccf after modulate); every pass from a clean analog[], like the oracle's"""
    case = E.CASES[cid]
    g = _context(crtlib, cid, exact, **kw)
    data = _device_images(cid)
    per = []
    for step in range(E.STEPS):
        g.analog.zero_()
        g.modulate(_settings(crtlib, case, data, step))
        g.synchronize()
        per.append((g.analog.cpu().numpy()[:, :g.input_size].copy(), g.ccf.copy()))
    g.close()
    return per


def _fused(crtlib, cid, exact, **kw):
    """-> per pass (the fused path's signal in the reference's layout, state, out)"""
    case = E.CASES[cid]
    g = _context(crtlib, cid, exact, **kw)
    data = _device_images(cid)
    nz = case["noise"]
    per = []
    for step in range(E.STEPS):
        s = _settings(crtlib, case, data, step)
        if isinstance(nz, (list, tuple)):
            g.fieldpass_knobs(s, np.array([[v, g.hue, g.saturation] for v in nz], dtype=np.int32))
        else:
            g.fieldpass(s, nz)
        g.synchronize()
        sig, _ = g.fieldpass_signal()
        per.append((sig.cpu().numpy()[:, :g.input_size].copy(), g.state.cpu().numpy().copy(), g.out.cpu().numpy().copy()))
    g.close()
    return per


def _check_stage(cid, per, what):
    case = E.CASES[cid]
    orc = E.oracle(case["name"])
    want = E.expected(cid)
    for step in range(E.STEPS):
        analog, ccf = per[step]
        for k in range(case["n"]):
            o = want[k][step]
            w = "%s %s field %d pass %d: " % (cid, what, k, step)
            np.testing.assert_array_equal(analog[k], o["analog"], err_msg=w + "analog")
            np.testing.assert_array_equal(ccf[k, :orc.vper, :orc.ccs], o["ccf_mod"], err_msg=w + "ccf after modulate")


def _check_fused(crtlib, cid, per, what):
    """-> the fields whose picture was compared in every pass"""
    case = E.CASES[cid]
    orc = E.oracle(case["name"])
    want = E.expected(cid)
    kept = []
    for k in range(case["n"]):
        whole = True
        for step in range(E.STEPS):
            sig, st, out = per[step]
            o = want[k][step]
            w = "%s %s field %d pass %d: " % (cid, what, k, step)
            np.testing.assert_array_equal(sig[k], o["inp"], err_msg=w + "inp")
            assert int(st[k][crtlib.ST_RN]) == o["rn"], w + "rn"
            if o["undefined"]:
                whole = False
                break
            assert (int(st[k][crtlib.ST_HSYNC]), int(st[k][crtlib.ST_VSYNC])) == (o["hsync"], o["vsync"]), w + "hsync, vsync"
            np.testing.assert_array_equal(st[k][crtlib.ST_CCF:crtlib.ST_CCF + 25].reshape(5, 5)[:orc.vper, :orc.ccs], o["ccf"], err_msg=w + "ccf")
            np.testing.assert_array_equal(out[k].reshape(-1), o["out"], err_msg=w + "out")
        if whole:
            kept.append(k)
    if not E.is_noise_edge(case):
        assert kept == list(range(case["n"])), "outside the noise-edge cases no field may drop out: kept %s" % kept
    return kept


def _both_exact(crtlib, cid, what, stage=True, **kw):
    fused = [_fused(crtlib, cid, exact, **kw) for exact in (0, 1)]
    kept = [_check_fused(crtlib, cid, fused[e], "%s exact %d" % (what, e)) for e in (0, 1)]
    assert kept[0] == kept[1]
    for step in range(E.STEPS):
        a, b = fused[0][step], fused[1][step]
        np.testing.assert_array_equal(a[0], b[0], err_msg="%s pass %d: signal, fast against exact" % (cid, step))
        np.testing.assert_array_equal(a[1][:, crtlib.ST_RN], b[1][:, crtlib.ST_RN])
        np.testing.assert_array_equal(a[1][kept[0]], b[1][kept[0]], err_msg="%s pass %d: state, fast against exact" % (cid, step))
        np.testing.assert_array_equal(a[2][kept[0]], b[2][kept[0]], err_msg="%s pass %d: out, fast against exact" % (cid, step))
    if stage:
        staged = [_stage(crtlib, cid, exact, **{k: v for k, v in kw.items() if k == "shape"}) for exact in (0, 1)]
        for e in (0, 1):
            _check_stage(cid, staged[e], "%s exact %d" % (what, e))
        for step in range(E.STEPS):
            np.testing.assert_array_equal(staged[0][step][0], staged[1][step][0], err_msg="%s pass %d: analog, fast against exact" % (cid, step))


@pytest.mark.parametrize("cid", sorted(E.CASES))
def test_encoder_cases_lane_per_row(crtlib, cid):
    """k_active (k_active_nes / the narrow NES loop; fieldpass_knobs cases: the KN instantiations) with the library's own tiles"""
    _both_exact(crtlib, cid, "shape 1", shape=1)


# Which instantiation each variant pins (launch_active, crt_encode.hip):
#   shape2   k_active_row (RGB systems; the NES has one shape)          tile16   OT = 16 beside either image tile
#   tile32 / tile64   the large sample tiles: OT = 32 beside the 16-dword image tile, OT = 64 (staged) beside the 32-dword one -- which of
#                     the two is the image width's business (w >= 1280), so both run on the 1279- and the 1280-wide case
#   flat     set_signal_layout(0): the reference's flat lines instead of the padded ones
# The sample tiles and the signal layout belong to the fused path alone (launch_active: `if constexpr (FULL && FAST ...)`; crt_run_encoder:
# `lay && fused`): modulate() never reads either switch, so the stage-level comparison runs for shape2 only -- every case has had it in
# test_encoder_cases_lane_per_row
# on extremes, phase, one knob edge of each kind, 3-byte and 4-byte pixels, per-field noise (KN), the NES table kernel and its narrow loop
VARIANTS = {"shape2": dict(shape=2), "tile16": dict(shape=1, tile=16), "tile32": dict(shape=1, tile=32), "tile64": dict(shape=1, tile=64),
            "flat": dict(shape=1, layout=0)}
PINNED = E.PINNED


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("cid", PINNED)
def test_encoder_instantiations(crtlib, cid, variant):
    _both_exact(crtlib, cid, variant, stage=variant == "shape2", **VARIANTS[variant])

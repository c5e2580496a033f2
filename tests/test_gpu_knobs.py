"""crthip_fieldpass_knobs on the GPU: a batch whose fields differ in channel noise, monitor hue and saturation against the oracle
run once per field with that field's knobs (tests/knobs_cases.py) -- inp[] (crthip_fieldpass_signal), hsync / vsync / rn / ccf and
the picture, bit for bit; no field of any case is excluded (none falls into the reference's undefined over-read, asserted)."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import knobs_cases as KC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_fieldpass_knobs")
    return crtlib


def _device_images(name, geo, n, distinct=None):
    import torch
    if name.startswith("nes") and not name.startswith("nesrgb"):
        ppu = np.stack([KC.ppu_image(k, distinct) for k in range(n)]).astype(np.int16)
        full = torch.zeros((n, 241, 256), dtype=torch.int16, device="cuda:0")
        full[:, :240] = torch.from_numpy(ppu).to("cuda:0")
        full[:, 240] = full[:, 239]
        return full[:, :240]
    imgs = np.stack([KC.image(geo, k, distinct) for k in range(n)])
    full = torch.zeros((n, geo["h"] + 1, geo["w"], 4), dtype=torch.uint8, device="cuda:0")
    full[:, :geo["h"]] = torch.from_numpy(imgs).to("cuda:0")
    full[:, geo["h"]] = full[:, geo["h"] - 1]
    return full[:, :geo["h"]]


def _make(crtlib, name, geo, n, crt_knobs=None, shape=1, sig_pad=1, seeds=None, distinct=None, overlap=None):
    g = crtlib.CRT(n, geo["outw"], geo["outh"], crtlib.FMT_BGRA, name[:4] if name.startswith("ntscfir") else name, device=0)
    g.eq_fir = R.EQ_KERNEL.get(name, 0)
    g.scanlines = 1
    for a, v in (crt_knobs or {}).items():
        setattr(g, a, v)
    g.set_shape(shape)
    g.set_signal_layout(sig_pad)
    if overlap:
        g.set_overlap(overlap)
    if seeds is not None:
        g.srand(seeds)
    par = [KC.parity(k) for k in range(n)]
    dc = R.Oracle(name).system in R.DOT_CRAWL_SYSTEMS
    s = crtlib.Settings(_device_images(name, geo, n, distinct), format=crtlib.FMT_BGRA, as_color=1,
                        field=[a for a, _ in par], frame=[b for _, b in par],
                        dot_crawl_offset=[KC.dot_crawl(name, k) for k in range(n)] if dc else 0)
    return g, s


def _next_parity(s, step):
    s.field = [f ^ 1 for f in s.field]
    if step % 2 == 0:
        s.frame = [f ^ 1 for f in s.frame]


def _compare(g, want, step, what, signal=True, fields=None):
    """every field of the batch against its oracle run; `want`: KC.oracle_fields"""
    g.synchronize()
    orc_size = want[fields[0] if fields else 0][step]["inp"].shape[0]
    gout = g.out.cpu().numpy()
    hs, vs, rn, ccf = g.get("hsync"), g.get("vsync"), g.get("rn"), g.ccf
    sig = g.fieldpass_signal()[0].cpu().numpy() if signal else None
    for k in (fields if fields is not None else range(len(want))):
        w = want[k][step]
        tag = "%s step %d field %d" % (what, step, k)
        assert not w["undefined"], tag + ": inside the reference's undefined over-read -- choose other knobs, exclude nothing"
        if sig is not None:
            np.testing.assert_array_equal(sig[k, :orc_size], w["inp"], err_msg=tag + " inp")
        assert (hs[k], vs[k], rn[k]) == (w["hsync"], w["vsync"], w["rn"]), tag + " hsync / vsync / rn"
        np.testing.assert_array_equal(ccf[k, :w["ccf"].shape[0], :w["ccf"].shape[1]], w["ccf"], err_msg=tag + " ccf")
        np.testing.assert_array_equal(gout[k].reshape(-1), w["out"], err_msg=tag + " out")


_WANT = {}


def _want(key, fn):
    """an expected result is computed once and shared by the tests (and parametrisations) that need it"""
    if key not in _WANT:
        _WANT[key] = fn()
    return _WANT[key]


@pytest.mark.parametrize("sig_pad", [1, 0])
@pytest.mark.parametrize("shape", [1, 2])
def test_six_fields_six_triples_mixed_tiers(crtlib, shape, sig_pad):
    """64x48 -> 160x120, six triples: one clean field inside the noisy batch, saturation / hue at the values that switch the
    decoder's tiers (the lines of one wavefront carry different tiers); both kernel shapes, padded and flat signal lines"""
    want = _want("small", lambda: KC.oracle_fields("ntsc", KC.SMALL, KC.SMALL_TRIPLES, steps=2))
    g, s = _make(crtlib, "ntsc", KC.SMALL, 6, shape=shape, sig_pad=sig_pad)
    for step in range(2):
        g.fieldpass_knobs(s, np.array(KC.SMALL_TRIPLES))
        _compare(g, want, step, "shape %d pad %d" % (shape, sig_pad))
        assert g.fieldpass_signal()[1] == bool(sig_pad)
        _next_parity(s, step)
    g.close()


@pytest.mark.parametrize("blend", [0, 1])
def test_seventy_fields_every_one_its_own_triple(crtlib, blend):
    """640x480 x 70: more than one wavefront of fields in the per-field kernels and a ragged last one; triples from a fixed seed"""
    trip = KC.drawn_triples(70, 20261018)
    want = _want(("full", blend), lambda: KC.oracle_fields("ntsc", KC.FULL, trip, steps=1, crt_knobs=dict(blend=blend), distinct=5))
    g, s = _make(crtlib, "ntsc", KC.FULL, 70, crt_knobs=dict(blend=blend), distinct=5)
    g.fieldpass_knobs(s, np.array(trip))
    _compare(g, want, 0, "70 fields blend %d" % blend)
    g.close()


@pytest.mark.parametrize("name,n", [("nes", 6), ("vhs", 5), ("vhslcg", 6), ("ntscbloom", 6), ("ntscfir7", 4), ("snes", 5)])
def test_one_case_per_system_and_build(crtlib, name, n):
    """NES (PPU-pixel encoder), the rand()-noise VHS build (per-field generators), VHS with the LCG noise, a bloom build (max_e from
    the field's noise), the 7-tap FIR decoder, and a system with per-line-class carriers"""
    geo = dict(w=256, h=240, outw=320, outh=240) if name == "nes" else KC.SMALL
    trip = KC.drawn_triples(n, 500 + n, noise_max=40, sat_lo=-15, sat_hi=30)
    seeds = [3 + 11 * k for k in range(n)] if name == "vhs" else None
    want = KC.oracle_fields(name, geo, trip, steps=2, seeds=seeds)
    g, s = _make(crtlib, name, geo, n, seeds=seeds)
    for step in range(2):
        g.fieldpass_knobs(s, np.array(trip))
        _compare(g, want, step, name)
        _next_parity(s, step)
    g.close()


def test_pv1000_is_refused(crtlib):
    """the 5-sample decoder takes monitor hue and saturation from the uniform parameters in its own prologue (crt_hip.h): refused,
    d_out and d_state untouched"""
    import torch
    g, s = _make(crtlib, "pv1k", KC.SMALL, 4)
    g.out.fill_(37)
    g._load_field_state(s)
    state = g.state.clone()
    with pytest.raises(RuntimeError, match="PV-1000"):
        g.fieldpass_knobs(s, np.array([(24, 0, 10)] * 4))
    g.synchronize()
    assert torch.equal(g.state, state) and bool((g.out == 37).all())
    g.fieldpass(s, 24)                                  # the uniform entry point still takes the system
    g.synchronize()
    g.close()


@pytest.mark.parametrize("name", ["ntsc", "vhs"])
def test_overlap_chunks(crtlib, name):
    """crthip_set_overlap(2), 512 fields: every chunk must read ITS fields' records -- the fused LCG-noise path (encoder + sync chain
    on the internal stream, decoders on the caller's) and the rand()-noise VHS unit.  Triples with period 15 over images with period
    4: a chunk reading from record 0 again would be off by 256 = 1 mod 15."""
    n, per = 512, 60
    base = KC.drawn_triples(15, 77, noise_max=40, sat_lo=5, sat_hi=30)
    trip = [base[(7 * k) % 15] for k in range(n)]
    seeds = [5 + (k % per) for k in range(n)] if name == "vhs" else None
    # field k and field k + 60 share image, parity, triple and seed: 60 oracle runs stand for the 512 fields
    first = KC.oracle_fields(name, KC.SMALL, trip[:per], steps=1, seeds=seeds[:per] if seeds else None, distinct=4)
    want = [first[k % per] for k in range(n)]
    g, s = _make(crtlib, name, KC.SMALL, n, seeds=seeds, distinct=4, overlap=2)
    g.fieldpass_knobs(s, np.array(trip))
    _compare(g, want, 0, name + " two chunks", signal=(name != "vhs"))
    g.close()


@pytest.mark.parametrize("phosphor", ["keep", "fade"])
def test_all_equal_triples_equal_the_uniform_field_pass(crtlib, phosphor):
    """byte for byte: out, state and the signal; also with the phosphor fade of the display modes"""
    import torch
    res = []
    for knobs in (False, True):
        g, s = _make(crtlib, "ntsc", KC.SMALL, 6, crt_knobs=dict(hue=-33, saturation=14, blend=1, phosphor=phosphor))
        g.out.fill_(200)
        for step in range(2):
            if knobs:
                g.fieldpass_knobs(s, np.array([(24, -33, 14)] * 6))
            else:
                g.fieldpass(s, 24)
            _next_parity(s, step)
        g.synchronize()
        res.append((g.out.clone(), g.state.clone(), g.fieldpass_signal()[0].clone()))
        g.close()
    for a, b, what in zip(res[0], res[1], ("out", "state", "signal")):
        assert torch.equal(a, b), what


def test_graph_capture_reads_the_records_at_replay(crtlib):
    """capture one knob call; replay; overwrite the record buffer (other triples inside the captured bounds); replay again: the second
    replay must be the oracle's result for the NEW knobs"""
    import torch
    n = 6
    first = KC.SMALL_TRIPLES
    second = [first[(k + 2) % n][:1] + (first[k][1] + 40,) + first[(k + 4) % n][2:] for k in range(n)]     # same extremes, other fields
    want = [_want("small", lambda: KC.oracle_fields("ntsc", KC.SMALL, first, steps=2)),
            _want("small2", lambda: KC.oracle_fields("ntsc", KC.SMALL, second, steps=1))]
    g, s = _make(crtlib, "ntsc", KC.SMALL, n)
    g.reserve(n)
    side = torch.cuda.Stream()
    g.use_stream(side)
    p = g.params(s, 0)
    g._load_field_state(s)
    torch.cuda.synchronize()
    state0 = g.state.clone()
    env = g.upload_knobs(np.array(first), p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.fieldpass_knobs(s, None, params=p)
    for r, trip in enumerate((first, second)):
        env2 = g.upload_knobs(np.array(trip), p)
        assert (env2.noise_max, env2.sat_abs_max, env2.loskip_wave_max) == (env.noise_max, env.sat_abs_max, env.loskip_wave_max)
        g.state.copy_(state0)
        g.out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _compare(g, want[r], 0, "replay %d" % r, signal=False)
    del graph
    g.close()


def test_a_knob_call_between_two_uniform_calls_leaves_nothing_behind(crtlib):
    """one long-lived context: fieldpass, fieldpass_knobs, fieldpass -- each equal to the same call on a fresh context"""
    import torch
    n = 6
    trip = np.array(KC.SMALL_TRIPLES)

    def call(g, s, which):
        g.state.zero_()
        g.state[:, 5] = 194
        g.out.zero_()
        if which == "knobs":
            g.fieldpass_knobs(s, trip)
        else:
            g.hue, g.saturation = which
            g.fieldpass(s, 30)
        g.synchronize()
        return g.out.clone(), g.state.clone()
    order = [(0, 10), "knobs", (25, 13)]
    fresh = []
    for which in order:
        g, s = _make(crtlib, "ntsc", KC.SMALL, n)
        fresh.append(call(g, s, which))
        g.close()
    g, s = _make(crtlib, "ntsc", KC.SMALL, n)
    for which, want in zip(order, fresh):
        out, state = call(g, s, which)
        assert torch.equal(out, want[0]) and torch.equal(state, want[1]), which
    g.close()
    want = _want("small", lambda: KC.oracle_fields("ntsc", KC.SMALL, KC.SMALL_TRIPLES, steps=2))
    np.testing.assert_array_equal(fresh[1][0][2].cpu().numpy().reshape(-1), want[2][0]["out"])


def test_refusals_leave_out_and_state_untouched(crtlib):
    import torch
    n = 4
    g, s = _make(crtlib, "ntsc", KC.SMALL, n)
    L = g.L
    p = g.params(s, 0)
    g._load_field_state(s)
    g.out.fill_(91)
    torch.cuda.synchronize()
    state = g.state.clone()
    g.upload_knobs(np.array(KC.SMALL_TRIPLES[:n]), p)

    def call(params, env, count=n):
        return L.crthip_fieldpass_knobs(g.ctx, C.byref(params), count, C.c_void_p(s.data.data_ptr()), g._image_stride(s),
                                        C.c_void_p(g.out.data_ptr()), g.out.stride(0), C.c_void_p(g.state.data_ptr()),
                                        C.c_void_p(g.knob_recs.data_ptr()), C.byref(env) if env is not None else None)
    good = g._knob_env
    bad_n = crtlib.KnobsEnv.from_buffer_copy(bytes(good))
    bad_n.n = n - 1
    bad_magic = crtlib.KnobsEnv.from_buffer_copy(bytes(good))
    bad_magic.magic = 0
    both = crtlib.Params.from_buffer_copy(bytes(p))
    both.flags |= crtlib.PHOSPHOR_FLAGS["fade"] | crtlib.PHOSPHOR_FLAGS["clear"]
    assert call(p, bad_n) == -1 and b"number of fields" in L.crthip_error_string(g.ctx)
    assert call(p, bad_magic) == -1
    assert call(both, good) == -1 and b"phosphor" in L.crthip_error_string(g.ctx)
    assert call(p, None) == -1
    assert L.crthip_fieldpass_knobs(g.ctx, C.byref(p), n, C.c_void_p(s.data.data_ptr()), g._image_stride(s), C.c_void_p(g.out.data_ptr()),
                                    g.out.stride(0), C.c_void_p(g.state.data_ptr()), None, C.byref(good)) == -1
    g.synchronize()
    assert torch.equal(g.state, state) and bool((g.out == 91).all())
    assert call(p, good) == 0                           # and the same arguments with the right env go through
    g.synchronize()
    assert not bool((g.out == 91).all())
    g.close()

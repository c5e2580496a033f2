"""crthip_fieldpass_sizes_knobs / crthip_stills_sizes_knobs on the GPU: batches whose fields differ in image size AND look against the
checker's loop of batch-1 calls (tests/sizes_knobs_cases.py; pinned to the real reference by tests/test_sizes_knobs_cpu.py) -- inp[]
(crthip_fieldpass_signal), ccf, hsync / vsync / rn and the picture, bit for bit; no field of any case is left out (asserted)."""
import ctypes as C
import os

import numpy as np
import pytest

import crtref as R
import fence as F
import sizes_cases as SC
import sizes_knobs_cases as ZK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_fieldpass_sizes_knobs")
    return crtlib


_WANT = {}


def _want(case, schedule=None):
    """the checker's loop for a case, computed once and shared (left unchanged by its users)"""
    key = (case, tuple(schedule) if schedule else None)
    if key not in _WANT:
        _WANT[key] = ZK.checker_fields(R.Oracle(ZK.base(case)["name"]), case, schedule=schedule)
    return _WANT[key]


def _make(crtlib, case, shape=1, sig_pad=1, exact=0, sig_tile=0, overlap=None, out=None):
    b = ZK.base(case)
    name, n = b["name"], len(ZK.CASES[case]["rows"])
    g = crtlib.CRT(n, ZK.OUTW, ZK.OUTH, crtlib.FMT_BGRA, name[:4] if name.startswith("ntscfir") else name, device=0, out=out)
    g.eq_fir = R.EQ_KERNEL.get(name, 0)
    g.scanlines = 1
    for a, v in b.get("crt_knobs", {}).items():
        setattr(g, a, v)
    g.set_shape(shape)
    g.set_signal_layout(sig_pad)
    g.set_exact(bool(exact))
    g.set_signal_tile(sig_tile)
    if overlap:
        g.set_overlap(overlap)
    if "seeds" in b:
        g.srand(b["seeds"])
    par = [SC.parity(k) for k in range(n)]
    dc = R.Oracle(name).system in R.DOT_CRAWL_SYSTEMS
    s = crtlib.Settings(None, format=b["fmt"], as_color=1, field=[a for a, _ in par], frame=[f for _, f in par],
                        dot_crawl_offset=[SC.dot_crawl(name, k) for k in range(n)] if dc else 0, spare_row=b["spare"])
    return g, s


def _device_layout(case):
    import torch
    buf, sizes = ZK.layout(case)
    return torch.from_numpy(buf).to("cuda:0"), sizes


def _rows(case):
    return np.array(ZK.CASES[case]["rows"], dtype=np.int32)


def _call(g, case, images, knobs, s, params=None, stills=None):
    """the call of the case: through CRT.fieldpass_sizes_knobs / stills_sizes_knobs; `hue_only` cases unbind the levels an (n, 8)
    upload binds and go on with the uploaded records"""
    p = params if params is not None else g.sizes_params(s, 0)
    if ZK.CASES[case].get("hue_only") and knobs is not None:
        if images is not None:
            g.upload_sizes(images, p)
        g.upload_knobs(knobs, p)
        assert g.L.crthip_bind_levels(g.ctx, None, None) == 0
        g._levels_bound = False
        images = knobs = None
    if params is None:
        g._load_field_state(s)
    if stills is not None:
        g.stills_sizes_knobs(images, knobs, schedule=stills, params=p, settings=s)
    else:
        g.fieldpass_sizes_knobs(images, knobs, params=p, settings=s)


def _compare(g, want, step, what, signal=True, fields=None):
    g.synchronize()
    gout = g.out.cpu().numpy()
    hs, vs, rn, ccf = g.get("hsync"), g.get("vsync"), g.get("rn"), g.ccf
    sig = g.fieldpass_signal()[0].cpu().numpy() if signal else None
    left_out = 0
    for k in (range(len(want)) if fields is None else fields):
        w = want[k][step]
        tag = "%s pass %d field %d" % (what, step, k)
        left_out += bool(w["undefined"])
        if sig is not None:
            np.testing.assert_array_equal(sig[k, :w["inp"].shape[0]], w["inp"], err_msg=tag + " inp")
        assert (hs[k], vs[k], rn[k]) == (w["hsync"], w["vsync"], w["rn"]), tag + " hsync / vsync / rn"
        np.testing.assert_array_equal(ccf[k, :w["ccf"].shape[0], :w["ccf"].shape[1]], w["ccf"], err_msg=tag + " ccf")
        np.testing.assert_array_equal(gout[k].reshape(-1), w["out"], err_msg=tag + " out")
    assert left_out == 0, what + ": fields inside the reference's undefined over-read -- choose other inputs, exclude nothing"


def _run_case(crtlib, case, what, **kw):
    want = _want(case)
    g, s = _make(crtlib, case, **kw)
    images, knobs = _device_layout(case), _rows(case)
    for step in range(ZK.STEPS):
        _call(g, case, images, knobs, s)
        _compare(g, want, step, case + " " + what)
        s.field = [f ^ 1 for f in s.field]
        if step % 2 == 0:
            s.frame = [f ^ 1 for f in s.frame]
    g.close()


PLAIN = sorted(c for c in ZK.CASES if not c.startswith("stills") and c != "many")


@pytest.mark.parametrize("case", PLAIN)
def test_every_case_equals_the_loop_of_batch_one_calls(crtlib, case):
    _run_case(crtlib, case, "default")


@pytest.mark.parametrize("case", ["scale8", "narrow8", "bound_white", "hue_only", "clean8"])
@pytest.mark.parametrize("sig_pad,exact,shape", [(0, 0, 1), (1, 1, 1), (0, 1, 2), (1, 0, 2)])
def test_layouts_exact_kernels_and_the_shape_setting(crtlib, case, sig_pad, exact, shape):
    """flat and padded signal lines x the exact (32-bit) instantiations x crthip_set_shape 1 / 2 (the encoder of a sizes call stays
    lane-per-scanline; the decoder follows the setting)"""
    _run_case(crtlib, case, "pad %d exact %d shape %d" % (sig_pad, exact, shape), sig_pad=sig_pad, exact=exact, shape=shape)


@pytest.mark.parametrize("case", ["scale8", "wide_only8", "clean3"])
@pytest.mark.parametrize("tile", [16, 32, 64])
def test_forced_signal_tiles_give_identical_bytes(crtlib, case, tile):
    """crthip_set_signal_tile: the knob instantiations exist for the 64-byte pieces only -- a forced larger tile is taken by the plain
    SZ kernel alone (clean3: noise 0, nothing bound) -- and every setting gives the oracle's bytes"""
    _run_case(crtlib, case, "signal tile %d" % tile, sig_tile=tile)


@pytest.mark.parametrize("tile", [16, 32])
def test_forced_image_tiles_give_identical_bytes(crtlib, tile):
    """the wide image tile on narrow images and the narrow one on wide images (crthip_set_pixel_tile's encoder half)"""
    for case in ("tiles8", "wide_mixed8"):
        g, s = _make(crtlib, case)
        g.L.crthip_set_pixel_tile(g.ctx, tile)
        _call(g, case, _device_layout(case), _rows(case), s)
        _compare(g, _want(case), 0, "%s image tile %d" % (case, tile))
        g.close()


def test_overlap_chunks(crtlib):
    """520 fields in two overlap chunks: all four record pointers are advanced to the chunk's first field"""
    _run_case(crtlib, "many", "overlap 2", overlap=2)


def _result(g, signal=True):
    g.synchronize()
    return (g.out.cpu().numpy(), g.state.cpu().numpy()) + ((g.fieldpass_signal()[0].cpu().numpy(),) if signal else ())


def test_equal_looks_give_the_sizes_call(crtlib):
    """every field with the CRT's own look and noise 24 == crthip_fieldpass_sizes at noise 24, byte for byte and state for state"""
    case = "scale8"
    images = _device_layout(case)
    g, s = _make(crtlib, case)
    g.fieldpass_sizes(images, 24, settings=s)
    want = _result(g)
    g.close()
    for width in (3, 8):
        g, s = _make(crtlib, case)
        g.fieldpass_sizes_knobs(images, np.array([(24,) + ZK.DEFAULTS[1:width]] * g.n, dtype=np.int32), settings=s)
        for a, b, what in zip(_result(g), want, ("out", "state", "inp")):
            np.testing.assert_array_equal(a, b, err_msg="width %d %s" % (width, what))
        g.close()


def test_equal_sizes_give_the_knobs_call(crtlib):
    """a batch whose sizes are all equal == crthip_fieldpass_knobs with the same looks"""
    import torch
    n, w, h = 6, 100, 37
    dev = torch.from_numpy(np.stack([R.synth_image(w, h + 1, 4, 99 + k) for k in range(n)])).to("cuda:0")
    par = [SC.parity(k) for k in range(n)]
    rows = np.array(ZK.COMBINED, dtype=np.int32)
    res = []
    for combined in (False, True):
        g = crtlib.CRT(n, ZK.OUTW, ZK.OUTH, crtlib.FMT_BGRA, "ntsc", device=0)
        g.scanlines = 1
        g.set_shape(1)
        s = crtlib.Settings(dev[:, :h], format=crtlib.FMT_BGRA, as_color=1, field=[a for a, _ in par], frame=[b for _, b in par], spare_row=True)
        if combined:
            g.fieldpass_sizes_knobs([dev[k] for k in range(n)], rows, settings=s)
        else:
            g.fieldpass_knobs(s, rows)
        res.append(_result(g))
        g.close()
    for a, b, what in zip(res[0], res[1], ("out", "state", "inp")):
        np.testing.assert_array_equal(a, b, err_msg=what)


CLI = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 0)]


@pytest.mark.parametrize("case", ["stills_clean", "stills_one_noisy"])
def test_stills_equal_the_loop(crtlib, case):
    """the interlaced CLI schedule: every still clean takes the shared signal (4 encoder runs for 8 passes, with every still's own
    size, levels and hue), one noisy still encodes per pass; both equal the checker's loop and the loop of fieldpass_sizes_knobs calls"""
    want = _want(case, CLI)
    images, knobs = _device_layout(case), _rows(case)
    g, s = _make(crtlib, case)
    _call(g, case, images, knobs, s, stills=CLI)
    _compare(g, want, len(CLI) - 1, case, signal=False)
    with pytest.raises(RuntimeError):
        g.fieldpass_signal()
    stills = _result(g, signal=False)
    g.close()
    g, s = _make(crtlib, case)
    for field, frame, aux in CLI:
        s.field, s.frame = field, frame
        _call(g, case, images, knobs, s)
    for a, b, what in zip(_result(g, signal=False), stills, ("out", "state")):
        np.testing.assert_array_equal(a, b, err_msg=what)
    g.close()


def test_graph_capture_with_size_and_knob_records_rewritten_between_replays(crtlib):
    """captured after crthip_reserve; all records are read at replay -- a replay after the size AND knob (level, hue) records of two
    fields were swapped (inside the captured envs: the same sizes and looks, other fields) gives the swapped batch's result"""
    import torch
    case = "scale8"
    want = _want(case)
    n = len(want)
    g, s = _make(crtlib, case)
    g.reserve()
    side = torch.cuda.Stream()
    g.use_stream(side)
    buf, sizes = _device_layout(case)
    rows = _rows(case)
    p = g.sizes_params(s, 0)
    g._load_field_state(s)
    torch.cuda.synchronize()
    state0 = g.state.clone()
    g.upload_sizes((buf, sizes), p)
    g.upload_knobs(rows, p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.fieldpass_sizes_knobs(None, None, params=p, settings=s)
    g.out.zero_()
    g.state.copy_(state0)
    graph.replay()
    torch.cuda.synchronize()
    _compare(g, want, 0, "replay 1", signal=False)
    # fields 0 and 4 (the same parity) trade size, image AND look
    assert SC.parity(0) == SC.parity(4)
    perm = list(range(n))
    perm[0], perm[4] = 4, 0
    srecs, senv = crtlib.sizes_prepare(p, sizes[perm])
    recs, levs, hues, env, lenv, henv = crtlib.knobs_prepare8(p, rows[perm])
    assert bytes(senv) == bytes(g._size_env) and bytes(env) == bytes(g._knob_env)
    assert bytes(lenv) == bytes(g._knob_env.lenv) and bytes(henv) == bytes(g._knob_env.henv)
    g.size_recs.copy_(torch.from_numpy(srecs.view("int32")))
    g.knob_recs.copy_(torch.from_numpy(recs))
    g.level_recs.copy_(torch.from_numpy(levs))
    g.hue_recs.copy_(torch.from_numpy(hues))
    g.out.zero_()
    g.state.copy_(state0)
    graph.replay()
    torch.cuda.synchronize()
    out = g.out.cpu().numpy()
    for k in range(n):
        np.testing.assert_array_equal(out[k].reshape(-1), want[perm[k]][0]["out"], err_msg="replay 2 field %d" % k)
    g.close()


def test_refusals_leave_out_and_state_untouched(crtlib):
    import torch
    case = "scale8"
    g, s = _make(crtlib, case)
    L = g.L
    buf, sizes = _device_layout(case)
    p = g.sizes_params(s, 0)
    g.upload_sizes((buf, sizes), p)
    g.upload_knobs(_rows(case), p)
    senv, env = g._size_env, g._knob_env
    g.out.fill_(0x5A)
    g.state[:, 0] = 7
    out0, state0 = g.out.clone(), g.state.clone()
    vp = C.c_void_p

    def call(params=p, images=buf.data_ptr(), srec=g.size_recs.data_ptr(), se=senv, rec=g.knob_recs.data_ptr(), e=env, n=g.n):
        return L.crthip_fieldpass_sizes_knobs(g.ctx, C.byref(params), n, vp(images), vp(g.out.data_ptr()), g.out.stride(0),
                                              vp(g.state.data_ptr()), vp(srec), C.byref(se) if se is not None else None,
                                              vp(rec), C.byref(e) if e is not None else None)

    def refused(rc, word):
        assert rc == -1
        msg = L.crthip_error_string(g.ctx).decode()
        assert word in msg, msg
        g.synchronize()
        assert torch.equal(g.out, out0) and torch.equal(g.state, state0)

    def altered(e, **kw):
        bad = type(e).from_buffer_copy(bytes(e))
        for a, v in kw.items():
            setattr(bad, a, v)
        return bad
    refused(call(se=altered(senv, magic=senv.magic ^ 1)), "crthip_sizes_prepare")
    refused(call(se=altered(senv, n=senv.n + 1)), "another number of fields")
    refused(call(e=altered(env, magic=env.magic ^ 1)), "crthip_knobs_prepare")
    refused(call(e=altered(env, n=env.n + 1)), "another number of fields")
    refused(call(srec=g.size_recs.data_ptr() + 2), "alignment")
    refused(call(rec=g.knob_recs.data_ptr() + 2), "alignment")
    refused(call(images=buf.data_ptr() + 2), "alignment")
    raw = g.sizes_params(crtlib.Settings(None, format=crtlib.FMT_BGRA, raw=1, spare_row=True), 0)
    refused(call(params=raw), "raw")
    both = g.sizes_params(s, 0)
    both.flags |= crtlib.PHOSPHOR_FLAGS["fade"] | crtlib.PHOSPHOR_FLAGS["clear"]
    refused(call(params=both), "phosphor")
    # level / hue envs prepared for another number of fields
    lenv = altered(env.lenv, n=env.lenv.n + 1)
    assert L.crthip_bind_levels(g.ctx, vp(g.level_recs.data_ptr()), C.byref(lenv)) == 0
    refused(call(), "levels")
    assert L.crthip_bind_levels(g.ctx, vp(g.level_recs.data_ptr()), C.byref(env.lenv)) == 0
    henv = altered(env.henv, n=env.henv.n + 1)
    assert L.crthip_bind_hues(g.ctx, vp(g.hue_recs.data_ptr()), C.byref(henv)) == 0
    refused(call(), "hues")
    assert L.crthip_bind_hues(g.ctx, vp(g.hue_recs.data_ptr()), C.byref(env.henv)) == 0
    assert call(se=None) == -1 and call(e=None) == -1 and call(srec=0) == -1 and call(rec=0) == -1 and call(images=0) == -1
    sched = (crtlib.Pass * 2)()
    rc = L.crthip_stills_sizes_knobs(g.ctx, C.byref(raw), g.n, vp(buf.data_ptr()), vp(g.out.data_ptr()), g.out.stride(0),
                                     vp(g.state.data_ptr()), 2, sched, vp(g.size_recs.data_ptr()), C.byref(senv),
                                     vp(g.knob_recs.data_ptr()), C.byref(env))
    refused(rc, "raw")
    # ... and the call still works afterwards
    g.out.zero_()
    g.state.zero_()
    g.state[:, crtlib.ST_RN] = 194
    g._load_field_state(s)
    assert call() == 0
    _compare(g, _want(case), 0, "after the refusals")
    g.close()
    for name, pkw, word in (("nes", dict(w=256, h=240), "NES"), ("pv1k", dict(w=1, h=1, format=crtlib.FMT_BGRA), "PV-1000")):
        c = crtlib.CRT(g.n, ZK.OUTW, ZK.OUTH, crtlib.FMT_BGRA, name, device=0)
        pn = crtlib.make_params(name, outw=ZK.OUTW, outh=ZK.OUTH, out_format=crtlib.FMT_BGRA, **pkw)
        c.out.fill_(0x5A)
        c.state[:, 0] = 7
        c_out0, c_state0 = c.out.clone(), c.state.clone()
        env3 = crtlib.knobs_prepare(crtlib.make_params("ntsc", w=1, h=1, outw=ZK.OUTW, outh=ZK.OUTH), np.array([(0, 0, 10)] * g.n, dtype=np.int32))[1]
        # (refused before anything is read: the image buffer stands in for both record arrays)
        rc = L.crthip_fieldpass_sizes_knobs(c.ctx, C.byref(pn), g.n, vp(buf.data_ptr()), vp(c.out.data_ptr()), c.out.stride(0),
                                            vp(c.state.data_ptr()), vp(buf.data_ptr()), C.byref(senv), vp(buf.data_ptr()), C.byref(env3))
        assert rc == -1 and word in L.crthip_error_string(c.ctx).decode(), L.crthip_error_string(c.ctx)
        c.synchronize()
        assert torch.equal(c.out, c_out0) and torch.equal(c.state, c_state0)
        c.close()


def test_long_lived_context(crtlib):
    """ONE context: the new call, fieldpass_sizes, fieldpass_knobs, fieldpass, the new call again with other records -- each equals a
    fresh context's result (nothing of a call survives it)"""
    import torch
    case = "scale8"
    n, w, h = len(ZK.CASES[case]["rows"]), 64, 48
    images, rows = _device_layout(case), _rows(case)
    dev = torch.from_numpy(np.stack([R.synth_image(w, h + 1, 4, 500 + k) for k in range(n)])).to("cuda:0")
    perm = [5, 4, 3, 2, 1, 0]

    def steps(s):
        su = crtlib.Settings(dev[:, :h], format=crtlib.FMT_BGRA, as_color=1, field=s.field, frame=s.frame, spare_row=True)
        return [lambda g: g.fieldpass_sizes_knobs(images, rows, settings=s),
                lambda g: g.fieldpass_sizes(images, 24, settings=s),
                lambda g: g.fieldpass_knobs(su, rows[perm]),
                lambda g: g.fieldpass(su, 24),
                lambda g: g.fieldpass_sizes_knobs((images[0], images[1][perm]), rows[::-1].copy(), settings=s),
                lambda g: g.fieldpass_knobs(su, rows[:, :3].copy()),
                lambda g: g.fieldpass_sizes_knobs(images, rows[:, :5].copy(), settings=s)]

    def power_on(g):
        g.out.zero_()
        g.state.zero_()
        g.state[:, crtlib.ST_RN] = 194
    old, s_old = _make(crtlib, case)
    for i in range(len(steps(s_old))):
        power_on(old)
        steps(s_old)[i](old)
        fresh, s_new = _make(crtlib, case)
        steps(s_new)[i](fresh)
        for a, b, what in zip(_result(old), _result(fresh), ("out", "state", "inp")):
            np.testing.assert_array_equal(a, b, err_msg="step %d %s" % (i, what))
        fresh.close()
    old.close()


def test_every_way_in_and_out_of_a_record_call_leaves_nothing_behind(crtlib):
    """ONE context through every record entry point -- field-passes, stills, sequences, sets and the bound phases, with levels and
    hues bound from the first knob call until they are unbound -- and through a refused call of every family in between.  Every
    accepted call equals the same call on a fresh context in out, state and (where the entry point leaves one) the signal; every
    refused call leaves out and state as they were.  GPU against GPU: the oracle is pinned per entry point elsewhere, this pins only
    that no call, accepted or refused, leaves anything of its records behind."""
    import torch
    case = "scale8"
    n, w, h = len(ZK.CASES[case]["rows"]), 64, 48
    images, rows = _device_layout(case), _rows(case)
    assert rows.shape == (n, 8)                             # (n, 8): upload_knobs binds level and hue records
    dev = torch.from_numpy(np.stack([R.synth_image(w, h + 1, 4, 500 + k) for k in range(n)])).to("cuda:0")
    perm = [5, 4, 3, 2, 1, 0]
    sched = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 0, 0)]
    ragged = [0, 2, n]
    vp = C.c_void_p

    def uniform(s):
        return crtlib.Settings(dev[:, :h], format=crtlib.FMT_BGRA, as_color=1, field=s.field, frame=s.frame, spare_row=True)

    def phases(g, s):
        g.seq_bind_knobs(rows[perm])
        g.seq_encode(uniform(s), 0, 0, 194)
        g.seq_sync(0, 0)
        g.seq_decode()
        g.seq_weave()

    def unbind(g):
        assert g.L.crthip_bind_levels(g.ctx, None, None) == 0 and g.L.crthip_bind_hues(g.ctx, None, None) == 0
        g._levels_bound = g._hues_bound = False

    def power_on(g):
        g.out.zero_()
        g.state.zero_()
        g.state[:, crtlib.ST_RN] = 194

    old, s_old = _make(crtlib, case)

    def accepted(what, call, signal=True):
        power_on(old)
        call(old, s_old)
        fresh, s_new = _make(crtlib, case)
        call(fresh, s_new)
        # the signal: CRT_INPUT_SIZE samples and the CRTHIP_TAIL mirror (16 bytes).  What crthip_fieldpass_signal copies behind them --
        # the slack of its last 16-byte piece -- is the library's workspace, not signal (crt_hip.h, Buffer contract): a padded
        # field-pass after a flat sequence call finds the sequence's samples there, in this library as in the one before it
        sig_len = old.input_size + 16
        for a, b, part in zip(_result(old, signal), _result(fresh, signal), ("out", "state", "inp")):
            if part == "inp":
                a, b = a[:, :sig_len], b[:, :sig_len]
            np.testing.assert_array_equal(a, b, err_msg="%s %s" % (what, part))
        fresh.close()

    def refused(what, env, word, call, **bad):
        """`call` with the fields `bad` of `env` altered for its duration: refused with `word`, out and state untouched"""
        old._load_field_state(s_old)                        # (what the wrappers below write before they call)
        old.synchronize()
        out0, state0 = old.out.clone(), old.state.clone()
        good = {a: getattr(env, a) for a in bad}
        for a, v in bad.items():
            setattr(env, a, v)
        try:
            with pytest.raises(RuntimeError, match=word):
                call(old, s_old)
        finally:
            for a, v in good.items():
                setattr(env, a, v)
        old.synchronize()
        assert torch.equal(old.out, out0) and torch.equal(old.state, state0), what + ": a refused call wrote"

    accepted("fieldpass", lambda g, s: g.fieldpass(uniform(s), 24))
    accepted("fieldpass_knobs", lambda g, s: g.fieldpass_knobs(uniform(s), rows))
    kenv = old._knob_env
    refused("fieldpass_knobs", kenv, "another number of fields", lambda g, s: g.fieldpass_knobs(uniform(s), None), n=n + 1)
    accepted("stills_knobs", lambda g, s: g.stills_knobs(uniform(s), rows[perm], schedule=sched), signal=False)
    kenv = old._knob_env
    refused("stills_knobs", kenv, "another number of fields", lambda g, s: g.stills_knobs(uniform(s), None, schedule=sched), n=n + 1)
    accepted("stills_sizes", lambda g, s: g.stills_sizes(images, 0, schedule=sched, settings=s), signal=False)
    senv = old._size_env
    refused("stills_sizes", senv, "another number of fields", lambda g, s: g.stills_sizes(None, 0, schedule=sched, settings=s), n=n + 1)
    accepted("stills_sizes_knobs", lambda g, s: g.stills_sizes_knobs(images, rows, schedule=sched, settings=s), signal=False)
    kenv = old._knob_env
    # the sizes env is good, the knob env is not: nothing of the size records may stay behind either
    refused("stills_sizes_knobs", kenv, "crthip_knobs_prepare", lambda g, s: g.stills_sizes_knobs(None, None, schedule=sched, settings=s),
            magic=kenv.magic ^ 1)
    refused("fieldpass_sizes_knobs", kenv, "another number of fields", lambda g, s: g.fieldpass_sizes_knobs(None, None, settings=s), n=n + 1)
    accepted("sequence_knobs", lambda g, s: g.sequence_knobs(uniform(s), rows))
    kenv = old._knob_env
    refused("sequence_knobs", kenv, "another number of fields", lambda g, s: g.sequence_knobs(uniform(s), None), n=n + 1)
    accepted("sequence_sets_knobs", lambda g, s: g.sequence_sets_knobs(uniform(s), rows[::-1].copy(), ragged))
    kenv = old._knob_env
    refused("sequence_sets_knobs", kenv, "another number of fields", lambda g, s: g.sequence_sets_knobs(uniform(s), None, ragged), n=n + 1)
    accepted("the bound phases", phases)
    kenv = old._knob_env
    kenv.n = n + 1                                          # (the binding takes any n > 0: every phase checks it against its own)
    assert old.L.crthip_seq_bind_knobs(old.ctx, vp(old.knob_recs.data_ptr()), C.byref(kenv)) == 0
    kenv.n = n
    refused("seq_encode", kenv, "another number of fields", lambda g, s: g.seq_encode(uniform(s), 0, 0, 194))
    refused("seq_sync", kenv, "another number of fields", lambda g, s: g.seq_sync(0, 0))
    refused("seq_decode", kenv, "another number of fields", lambda g, s: g.seq_decode())
    unbind(old)                                             # (the phases' binding stays: no call below reads it)
    accepted("fieldpass_knobs, nothing bound", lambda g, s: g.fieldpass_knobs(uniform(s), rows[:, :5].copy()))
    accepted("fieldpass_sizes", lambda g, s: g.fieldpass_sizes(images, 24, settings=s))
    accepted("stills", lambda g, s: g.stills(uniform(s), 24, schedule=sched), signal=False)
    accepted("sequence", lambda g, s: g.sequence(uniform(s), 24))
    accepted("fieldpass again", lambda g, s: g.fieldpass(uniform(s), 24))
    old.close()


@pytest.mark.parametrize("case", ["scale8", "hues"])
def test_fenced_buffers(crtlib, case):
    """images packed with no slack inside a fenced allocation, d_out and d_state fenced too, VALID records: the payloads equal the
    oracle, nothing outside d_out and d_state is written, the image buffer is unchanged"""
    import torch
    want = _want(case)
    buf, sizes = ZK.layout(case)
    n = len(want)
    fi = F.Fenced(1, buf.size, device="cuda:0", name="images")
    fo = F.Fenced(n, ZK.OUTW * ZK.OUTH * 4, pitch=ZK.OUTW * 4, device="cuda:0", name="d_out")
    fs = F.Fenced(n, 144, device="cuda:0", name="d_state")
    pre_i = fi.prefill(11, buf[None])
    pre_o = fo.prefill(111, np.zeros((n, ZK.OUTW * ZK.OUTH * 4), dtype=np.uint8))
    st = np.zeros((n, 36), dtype=np.int32)
    st[:, 5] = 194
    pre_s = fs.prefill(211, st)
    g, s = _make(crtlib, case, out=fo.view((ZK.OUTH, ZK.OUTW, 4)))
    g.state = fs.view((36,), torch.int32)
    _call(g, case, (fi.view((buf.size,))[0], sizes), _rows(case), s)
    _compare(g, want, 0, case + " fenced")
    fi.assert_unchanged(pre_i)
    fo.assert_fence_intact(pre_o)
    fs.assert_fence_intact(pre_s)
    g.close()


def test_stills_dir_uniform_looks_write_the_one_call_files(crtlib, tmp_path):
    """tools/stills_dir.py --one-call --looks FILE with every picture at the command line's NOISE / HUE and the defaults writes the
    files --one-call alone writes; other looks write other files"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("stills_dir", os.path.join(R.ROOT, "tools", "stills_dir.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = tmp_path / "in"
    src.mkdir()
    names = ["pic%d.ppm" % k for k in range(5)]
    for k, (w, h) in enumerate([(40, 30), (17, 9), (40, 30), (300, 5), (8, 100)]):
        tool.write_ppm(str(src / names[k]), R.synth_image(w, h, 3, 70 + k))
    for flags, noise, hue in (("-o", 0, 5), ("-f", 12, -30)):
        looks = tmp_path / ("looks%s.txt" % flags)
        looks.write_text("".join("%s %s\n" % (nm, " ".join(str(v) for v in tool.default_look(noise, hue))) for nm in names))
        a, b = tmp_path / ("one" + flags), tmp_path / ("looks" + flags)
        assert tool.main(["stills_dir.py", "--one-call", flags, "64", "48", str(noise), str(hue), str(src), str(a)]) == 0
        assert tool.main(["stills_dir.py", "--one-call", "--looks", str(looks), flags, "64", "48", "99", "99", str(src), str(b)]) == 0
        assert sorted(os.listdir(str(a))) == sorted(os.listdir(str(b))) == names
        for name in names:
            assert (a / name).read_bytes() == (b / name).read_bytes(), name
    looks.write_text("".join("%s 0 %d 14 3 170 2 95 %d\n" % (nm, 10 * k, 40 * k) for k, nm in enumerate(names)))
    c = tmp_path / "varied"
    assert tool.main(["stills_dir.py", "--one-call", "--looks", str(looks), "-o", "64", "48", "0", "0", str(src), str(c)]) == 0
    assert sum((c / nm).read_bytes() != (a / nm).read_bytes() for nm in names) == len(names)

"""GPU parity of stills with one look per still (crthip_stills_knobs / CRT.stills_knobs, include/crt_hip.h): several field-passes of
n images onto n pictures in one call, record k still k's look in every pass; with every still at noise 0 the clean signal of every
distinct schedule entry is encoded once, with every still's own levels and hue.  Every picture and every (hsync, vsync, rn, ccf)
against the oracle running the reference's loop once per still with that still's values (tests/stills_knobs_cases.py; the compiled
reference runs the same loops in tests/test_stills_knobs_cpu.py, which also asserts that no case needs the UB exclusion).  Bit-exact."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import stills_cases as SC
import stills_knobs_cases as SKC
from test_gpu_levels import _untouched_after
from test_gpu_stills import _compare, _result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_stills_knobs"), "no crthip_stills_knobs in this build"
    return crtlib


def _settings(crtlib, case, one_image=None, copies=False, **geo):
    """device settings of the case's images (every image followed by a readable row: crt_ntsc.c:263); one_image = k: image k alone,
    expanded to the n stills (stride(0) == 0), or -- copies -- n copies of it"""
    import torch
    imgs = SKC.images(case)
    n, h = imgs.shape[0], imgs.shape[1]
    if one_image is not None and copies:
        imgs = np.stack([imgs[one_image]] * n)
    nes = SC.sysid(case) == R.SYS_NES
    full = torch.zeros((n, h + 1) + tuple(imgs.shape[2:]), dtype=torch.int16 if nes else torch.uint8, device="cuda:0")
    full[:, :h] = torch.from_numpy(np.ascontiguousarray(imgs.astype(np.int16) if nes else imgs)).to("cuda:0")
    full[:, h] = full[:, h - 1]
    data = full[:, :h]
    if one_image is not None and not copies:
        data = full[one_image:one_image + 1, :h].expand((n,) + tuple(data.shape[1:]))
        assert data.stride(0) == 0
    if nes:
        return crtlib.Settings(data, hue=0, **geo)
    return crtlib.Settings(data, format=crtlib.FMT_BGRA, as_color=1, **geo)


def _context(crtlib, case, config=(0, 1, 0), n=None):
    shape, pad, exact = config
    name = case["name"]
    g = crtlib.CRT(n or case["n"], case["outw"], case["outh"], case["ofmt"], name[:4] if name.startswith("ntscfir") else name, device=0)
    g.eq_fir = R.EQ_KERNEL.get(name, 0)
    for k, v in case["knobs"].items():
        setattr(g, k, v)
    g.phosphor = case["mode"]
    g.set_shape(shape)
    g.set_signal_layout(pad)
    g.set_exact(exact)
    if SC.is_vhs_rand(case):
        g.srand(case["seeds"][:case["n"]])
    return g


def _rows(case):
    return np.array(case["rows"])


def _knobs_loop(g, case, s, rows):
    """the hand-written loop: one CRT.fieldpass_knobs per schedule entry, the encoder inputs set in the state before each"""
    dot = SC.sysid(case) in R.DOT_CRAWL_SYSTEMS
    for field, frame, aux in case["sched"]:
        s.field, s.frame = field & 1, frame & 1
        s.dot_crawl_offset, s.aberration = (aux, 0) if dot else (0, aux)
        g.fieldpass_knobs(s, rows)


def _same(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what)
    assert a[1] == b[1], what
    np.testing.assert_array_equal(a[2], b[2], err_msg=what)


@pytest.mark.parametrize("cid", SKC.CASE_IDS)
def test_stills_knobs_equal_the_loop_per_still(crtlib, cid):
    """every case on every (kernel shape, signal layout, set_exact) it lists, against the oracle; as an extra, library against
    library: the loop of CRT.fieldpass_knobs calls"""
    case = SKC.case(cid)
    want = SKC.expected(case)
    for config in case["configs"]:
        g = _context(crtlib, case, config)
        g.stills_knobs(_settings(crtlib, case), _rows(case), schedule=case["sched"])
        got = _result(g)
        with pytest.raises(RuntimeError):
            g.fieldpass_signal()                             # refused after the call, as after crthip_stills
        g.close()
        _compare(case, want, got, "%s config %s" % (cid, config))
    g = _context(crtlib, case, case["configs"][-1])
    _knobs_loop(g, case, _settings(crtlib, case), _rows(case))
    loop = _result(g)
    g.close()
    _same(loop, got, cid + ": the loop of fieldpass_knobs calls")


def test_cli_keywords_are_the_cli_schedule(crtlib):
    for cid, kw in (("ntsc-cli-sat-noise0", dict()), ("ntsc-cli1-combined-one-noisy", dict(first_field=1)),
                    ("ntsc-bound-inside-noise0", dict(interlaced=False))):
        case = SKC.case(cid)
        g = _context(crtlib, case)
        g.stills_knobs(_settings(crtlib, case), _rows(case), **kw)
        _compare(case, SKC.expected(case), _result(g), cid + " by keywords")
        g.close()


def _launches(crtlib, case, call):
    g = _context(crtlib, case)
    s = _settings(crtlib, case)
    g.fieldpass(s, 0)                                       # the cached tables are built by a call that is not counted
    g.synchronize()
    g.profile(True)
    call(g, s)
    cnt = g.profile_read()
    g.profile(False)
    g.close()
    return cnt["active"][1], cnt["decode"][1]


@pytest.mark.parametrize("width", [3, 8])
def test_launch_counts_with_records(crtlib, width):
    """crthip_profile_read counts the launches: with every still at noise 0 the encoder's active-video kernel runs once per distinct
    entry (4 for the interlaced CLI schedule, 1 for the progressive one, 3 for CUSTOM5), with ONE noisy still once per pass; the
    decoder always once per pass.  The same with an (n, 8) upload: level and hue records bound"""
    case = SKC.case("ntsc-cli-sat-noise0")
    clean = np.array(SKC.with_noise(SKC.COMBINED, 0))[:, :width]
    noisy = np.array(SKC.with_noise(SKC.COMBINED, [0, 24, 0, 0, 0, 0]))[:, :width]
    act1, dec1 = _launches(crtlib, case, lambda g, s: g.fieldpass_knobs(s, clean))
    assert act1 >= 1 and dec1 >= 1
    assert _launches(crtlib, case, lambda g, s: g.fieldpass_knobs(s, noisy)) == (act1, dec1)
    assert _launches(crtlib, case, lambda g, s: g.stills_knobs(s, clean)) == (4 * act1, 8 * dec1)
    assert _launches(crtlib, case, lambda g, s: g.stills_knobs(s, clean, interlaced=False)) == (1 * act1, 4 * dec1)
    assert len(SC.distinct_entries(dict(sched=SKC.CUSTOM5))) == 3
    assert _launches(crtlib, case, lambda g, s: g.stills_knobs(s, clean, schedule=SKC.CUSTOM5)) == (3 * act1, 5 * dec1)
    assert _launches(crtlib, case, lambda g, s: g.stills_knobs(s, noisy)) == (8 * act1, 8 * dec1)


@pytest.mark.parametrize("cid", ["ntsc-custom5-hues-noise0", "ntsc-cli1-combined-one-noisy"])
def test_one_image_with_n_looks(crtlib, cid):
    """image_stride == 0 (a tensor expanded from one image, its one spare row behind it): equal to the call with n copies of that
    image, and to the oracle -- once on the shared path, once with noise"""
    case = SKC.case(cid)
    want = SKC.expected(case, one_image=1)
    res = []
    for copies in (False, True):
        g = _context(crtlib, case, case["configs"][0])
        s = _settings(crtlib, case, one_image=1, copies=copies)
        assert (g._image_stride(s) == 0) == (not copies) and g._has_spare_row(s)
        g.stills_knobs(s, _rows(case), schedule=case["sched"])
        res.append(_result(g))
        g.close()
        _compare(case, want, res[-1], "%s: one image, %s" % (cid, "n copies" if copies else "image_stride 0"))
    _same(res[0], res[1], cid + ": image_stride 0 against n copies")


def _oracle_step(case, crts, imgs, sched, rows):
    """`sched` on the oracle's television sets as they stand, set k with the look rows[k] -> what _result gives"""
    for k, c in enumerate(crts):
        row = rows[k]
        for a, v in zip(SKC.CRT_KNOBS, row[1:7]):
            c.set(a, v)
        pad = np.concatenate([imgs[k], imgs[k][-1:]], axis=0)
        for field, frame, _aux in sched:
            c.settings(pad, format=R.FMT_BGRA, w=case["inp"][0], h=case["inp"][1], as_color=1, field=field & 1, frame=frame & 1)
            c.sset("hue", row[7])
            c.analog[:] = 0
            c.modulate()
            hs_before = c.get("hsync")
            c.demodulate(row[0], trace=True)
            assert not R.reads_past_inp(c.ref, c.trace, c.get("vsync"), hs_before), "still %d: the reference over-reads here (undefined)" % k
    return [(c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn"), np.array(c.ccf)) for c in crts]


def test_call_history_on_one_context(crtlib):
    """stills_knobs at (n, 8), a uniform stills, fieldpass_knobs, stills_knobs at (n, 3) -- on ONE context, the television sets
    carried from call to call, every step against the oracle; the uniform call also against a context that never saw a record;
    the (n, 3) upload unbinds levels and hues"""
    import torch
    case = dict(SKC.case("ntsc-cli-sat-noise0"))
    n, imgs = case["n"], SKC.images(case)
    orc = R.Oracle("ntsc")
    crts = []
    for _ in range(n):
        c = orc.new_crt(case["outw"], case["outh"], case["ofmt"])
        for a, v in case["knobs"].items():
            c.set(a, v)
        crts.append(c)
    uniform = lambda noise: [(noise, 0, 10, 0, 180, 0, 100, 0)] * n
    g = _context(crtlib, case, (1, 1, 0))
    check = lambda want, what: _compare(case, want, _result(g), what)

    rows8 = SKC.with_noise(SKC.COMBINED, 0)
    g.stills_knobs(_settings(crtlib, case), np.array(rows8))
    assert g._levels_bound and g._hues_bound
    check(_oracle_step(case, crts, imgs, SKC.INTERLACED0, rows8), "1: stills_knobs at (n, 8), noise 0")
    fresh = _context(crtlib, case, (1, 1, 0))
    for noise, kw, sched in ((0, dict(interlaced=False), SKC.PROGRESSIVE), (24, dict(first_field=1), SKC.INTERLACED1)):
        fresh.out.copy_(g.out)
        fresh.state.copy_(g.state)
        torch.cuda.synchronize()
        g.stills(_settings(crtlib, case), noise, **kw)
        fresh.stills(_settings(crtlib, case), noise, **kw)
        check(_oracle_step(case, crts, imgs, sched, uniform(noise)), "2: uniform stills at noise %d with records bound" % noise)
        _same(_result(fresh), _result(g), "2: uniform stills at noise %d against a fresh context" % noise)
    fresh.close()
    assert g._levels_bound and g._hues_bound
    s = _settings(crtlib, case)
    s.field, s.frame = 1, 0
    g.fieldpass_knobs(s, np.array(SKC.COMBINED))
    check(_oracle_step(case, crts, imgs, [(1, 0, 0)], SKC.COMBINED), "3: fieldpass_knobs at (n, 8)")
    g.fieldpass_signal()                                     # works after a field-pass
    rows3 = SKC.with_noise(SKC.SAT_ROWS, 0)
    g.stills_knobs(_settings(crtlib, case), np.array(rows3), schedule=SKC.CUSTOM5)
    assert not g._levels_bound and not g._hues_bound
    check(_oracle_step(case, crts, imgs, SKC.CUSTOM5, [r + (0, 180, 0, 100, 0) for r in rows3]), "4: stills_knobs at (n, 3)")
    g.close()


def test_reserved_workspace_and_a_second_identical_call(crtlib):
    case = SKC.case("ntsc-custom5-hues-noise0")
    g = _context(crtlib, case, (2, 1, 0))
    g.reserve()
    g.stills_reserve(len(SC.distinct_entries(case)))
    s = _settings(crtlib, case)
    g.stills_knobs(s, _rows(case), schedule=case["sched"])
    first = _result(g)
    _compare(case, SKC.expected(case), first, "first call")
    g.out.zero_()
    g.state.zero_()
    g.state[:, crtlib.ST_RN] = 194
    g.stills_knobs(s, _rows(case), schedule=case["sched"])
    _same(first, _result(g), "second identical call")
    g.close()


def test_captured_call_reads_the_records_at_replay(crtlib):
    """one call captured into a HIP graph; between the replays all three record buffers are rewritten inside the captured bounds
    (the stills trade looks): every replay = the oracle for the records the buffers then hold"""
    import torch
    case = SKC.case("ntsc-custom5-hues-noise0")
    first = case["rows"]
    moved = first[::-1]
    want = {0: SKC.expected(case), 1: SKC.expected(case, rows=moved)}
    g = _context(crtlib, case, (1, 1, 0))
    g.reserve()
    g.stills_reserve(len(SC.distinct_entries(case)))
    s = _settings(crtlib, case)
    g.fieldpass(s, 24)                                       # a uniform call builds the cached tables
    g.synchronize()
    g.out.zero_()
    g.state.zero_()
    g.state[:, crtlib.ST_RN] = 194
    state0 = g.state.clone()
    side = torch.cuda.Stream()
    g.use_stream(side)
    p = g.params(s, 0)
    env = g.upload_knobs(np.array(first), p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.stills_knobs(s, None, schedule=case["sched"], params=p)
    torch.cuda.synchronize()
    assert bool((g.out == 0).all()), "a capture runs nothing"
    for r, which in enumerate((0, 1, 0)):
        env2 = g.upload_knobs(np.array(first if which == 0 else moved), p)
        assert bytes(env2) == bytes(env) and bytes(env2.lenv) == bytes(env.lenv) and bytes(env2.henv) == bytes(env.henv)
        g.state.copy_(state0)
        g.out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _compare(case, want[which], _result(g), "replay %d" % r)
    del graph
    g.use_stream(None)
    g.close()


def test_refusals_leave_pictures_and_states_alone(crtlib):
    """what crthip_stills refuses and what crthip_fieldpass_knobs refuses: -1, a message, d_out still holds its fill pattern and
    d_state its values, and crthip_fieldpass_signal still hands out the signal of the field-pass before (a refused call claims
    nothing); the context works afterwards"""
    import torch
    vp = C.c_void_p
    case = SKC.case("ntsc-cli-sat-noise0")
    n = case["n"]
    g = _context(crtlib, case, (1, 1, 0))
    s = _settings(crtlib, case)
    L = g.L
    rows8 = np.array(SKC.COMBINED)
    g.fieldpass_knobs(s, rows8)
    g.synchronize()
    signal = g.fieldpass_signal()[0].clone()
    p = g.params(s, 0)
    env = g._knob_env
    sched = (crtlib.Pass * 65)()

    def call(params=p, count=n, images=None, out=True, passes=8, sch=sched, recs=None, e=env):
        return L.crthip_stills_knobs(g.ctx, C.byref(params), count, vp(s.data.data_ptr() if images is None else images), g._image_stride(s),
                                     vp(g.out.data_ptr()) if out else None, g.out.stride(0), vp(g.state.data_ptr()), passes, sch,
                                     vp(g.knob_recs.data_ptr() if recs is None else recs), C.byref(e))

    def refused(fn, match):
        _untouched_after(g, fn, match)
        assert torch.equal(g.fieldpass_signal()[0], signal), match

    for bad in (0, -3, 65):
        refused(lambda: call(passes=bad), b"n_passes")
    refused(lambda: call(sch=None), b"sched")
    refused(lambda: call(out=False), b"null device pointer")
    refused(lambda: call(images=s.data.data_ptr() + 2), b"d_images")
    refused(lambda: call(recs=g.knob_recs.data_ptr() + 2), b"d_recs")
    bad = crtlib.KnobsEnv.from_buffer_copy(bytes(env))
    bad.magic ^= 1
    refused(lambda: call(e=bad), b"crthip_knobs_prepare")
    bad = crtlib.KnobsEnv.from_buffer_copy(bytes(env))
    bad.n = n - 1
    refused(lambda: call(e=bad), b"another number of fields")
    bad = crtlib.KnobsEnv.from_buffer_copy(bytes(env))
    bad.reserved[0] = 2                                     # pic
    refused(lambda: call(e=bad), b"picture words")
    both = g.params(s, 0)
    both.flags |= crtlib.F_PHOSPHOR_FADE | crtlib.F_PHOSPHOR_CLEAR
    refused(lambda: call(params=both), b"phosphor")
    far = g.params(_settings(crtlib, case, yoffset=30), 0)
    refused(lambda: call(params=far), b"out of contract")
    # the bound level / hue records were prepared for another number of stills
    lenv, henv = env.lenv, env.henv
    for which, good, bind, ptr in (("levels", lenv, L.crthip_bind_levels, g.level_recs), ("hues", henv, L.crthip_bind_hues, g.hue_recs)):
        wrong = type(good).from_buffer_copy(bytes(good))
        wrong.n = n - 1
        assert bind(g.ctx, vp(ptr.data_ptr()), C.byref(wrong)) == 0
        refused(call, which.encode() + b": the bound")
        assert bind(g.ctx, vp(ptr.data_ptr()), C.byref(good)) == 0
    with pytest.raises(ValueError):
        g.stills_knobs(s, rows8, schedule=[])
    g.synchronize()
    g.out.zero_()
    g.state.zero_()
    g.state[:, crtlib.ST_RN] = 194
    rows = SKC.with_noise(SKC.COMBINED, 0)
    g.stills_knobs(s, np.array(rows))                       # and the context still works
    _compare(case, SKC.expected(case, rows=rows), _result(g), "after the refusals")
    g.close()

    # the PV-1000 (no per-field knobs at all), and the NES with level or hue records bound by hand (with the levels also its border)
    g = crtlib.CRT(n, case["outw"], case["outh"], crtlib.FMT_BGRA, "pv1k", device=0)
    s = _settings(crtlib, case)

    def wrapped(fn, text):
        def run():
            try:
                fn()
            except RuntimeError as e:
                assert text in str(e), str(e)
                return -1
            return 0
        return run
    _untouched_after(g, wrapped(lambda: g.stills_knobs(s, rows8[:, :3]), "PV-1000"), b"PV-1000", fill=37)
    g.close()
    nes = SKC.case("nes-dots-pic-one-noisy")
    g = _context(crtlib, nes)
    s = _settings(crtlib, nes)
    levs = torch.zeros((nes["n"], crtlib.LEVEL_REC_INTS), dtype=torch.int32, device="cuda:0")
    hues = torch.zeros((nes["n"], crtlib.HUE_REC_INTS), dtype=torch.int32, device="cuda:0")
    assert nes["n"] == n - 1
    lenv5 = crtlib.LevelsEnv.from_buffer_copy(bytes(lenv))
    lenv5.n = nes["n"]
    henv5 = crtlib.HuesEnv.from_buffer_copy(bytes(henv))
    henv5.n = nes["n"]
    assert g.L.crthip_bind_levels(g.ctx, vp(levs.data_ptr()), C.byref(lenv5)) == 0
    _untouched_after(g, wrapped(lambda: g.stills_knobs(s, _rows(nes)), "levels: the NES"), b"levels: the NES", fill=37)
    pb = g.params(s, 0)
    pb.flags |= crtlib.F_NES_BORDER
    _untouched_after(g, wrapped(lambda: g.stills_knobs(s, _rows(nes), params=pb), "CRTHIP_F_NES_BORDER"), b"CRTHIP_F_NES_BORDER", fill=37)
    assert g.L.crthip_bind_levels(g.ctx, None, None) == 0
    assert g.L.crthip_bind_hues(g.ctx, vp(hues.data_ptr()), C.byref(henv5)) == 0
    _untouched_after(g, wrapped(lambda: g.stills_knobs(s, _rows(nes)), "hues: the NES"), b"hues: the NES", fill=37)
    assert g.L.crthip_bind_hues(g.ctx, None, None) == 0
    g.out.zero_()
    g.stills_knobs(s, _rows(nes), schedule=nes["sched"])   # nothing bound: the NES takes its (n, 5) looks
    _compare(nes, SKC.expected(nes), _result(g), "nes after the refusals")
    g.close()

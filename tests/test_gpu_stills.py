"""GPU parity of the stills mode (crthip_stills / CRT.stills, include/crt_hip.h): several field-passes of the same images onto the
same pictures in one call, at noise 0 with every distinct (field, frame, aux) of the schedule encoded once.  Every picture and every
(hsync, vsync, rn, ccf) against the oracle running the reference's serial loop once per image (tests/stills_cases.py; the compiled
reference and its `ntsc` program run the same loops in tests/test_stills_cpu.py).  Bit-exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import crtref as R
import stills_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _settings(crtlib, case, **geo):
    """device settings of the case's images (every image followed by a readable row: crt_ntsc.c:263)"""
    import torch
    imgs = SC.images(case)
    n, h = imgs.shape[0], imgs.shape[1]
    if SC.sysid(case) == R.SYS_NES:
        full = torch.zeros((n, h + 1, imgs.shape[2]), dtype=torch.int16, device="cuda:0")
        full[:, :h] = _to_dev(imgs.astype(np.int16))
        full[:, h] = full[:, h - 1]
        return crtlib.Settings(full[:, :h], hue=0, **geo)
    full = torch.zeros((n, h + 1) + tuple(imgs.shape[2:]), dtype=torch.uint8, device="cuda:0")
    full[:, :h] = _to_dev(imgs)
    full[:, h] = full[:, h - 1]
    return crtlib.Settings(full[:, :h], format=crtlib.FMT_BGRA, **geo)


def _context(crtlib, case, shape=0):
    g = crtlib.CRT(case["n"], case["outw"], case["outh"], case["ofmt"], case["name"], device=0)
    for k, v in case["knobs"].items():
        setattr(g, k, v)
    g.phosphor = case["mode"]
    g.set_shape(shape)
    if SC.is_vhs_rand(case):
        g.srand(SC.VHS_SEEDS[:case["n"]])
    return g


def _result(g):
    g.synchronize()
    return g.out.cpu().numpy(), list(zip(g.get("hsync"), g.get("vsync"), g.get("rn"))), g.ccf


def _compare(case, want, got, what):
    out, st, ccf = got
    orc = R.Oracle(case["name"])
    for k in range(case["n"]):
        o, hs, vs, rn, cf = want[k]
        assert st[k] == (hs, vs, rn), "%s: state of still %d" % (what, k)
        np.testing.assert_array_equal(ccf[k, :orc.vper, :orc.ccs], cf, err_msg="%s: ccf of still %d" % (what, k))
        np.testing.assert_array_equal(out[k].reshape(-1), o, err_msg="%s: picture of still %d" % (what, k))


def _fieldpass_loop(crtlib, g, case, s):
    """the hand-written loop: one CRT.fieldpass per schedule entry, the encoder inputs set in the state before each"""
    dot = SC.sysid(case) in R.DOT_CRAWL_SYSTEMS
    for field, frame, aux in case["sched"]:
        s.field, s.frame = field & 1, frame & 1
        s.dot_crawl_offset, s.aberration = (aux, 0) if dot else (0, aux)
        g.fieldpass(s, case["noise"])


@pytest.mark.parametrize("cid", SC.CASE_IDS)
def test_stills_equal_the_serial_loop_per_image(crtlib, cid):
    """ntsc / bloom / nes / pv1k / vhs (rand() noise, one stream per still) / vhslcg (aberration band); noise 0, 24, 120; the CLI's
    schedule from either field, progressive, and schedules of the case's own; blend 1 and 0; a phosphor mode; row collisions,
    duplicated rows, the wide-run decoder; every kernel shape the case lists.  As an extra, library against library: the loop of
    CRT.fieldpass calls."""
    case = SC.case(cid)
    want = SC.expected(case)
    for shape in case["shapes"]:
        g = _context(crtlib, case, shape)
        g.stills(_settings(crtlib, case), case["noise"], schedule=case["sched"])
        got = _result(g)
        g.close()
        _compare(case, want, got, "%s shape %d" % (cid, shape))
    g = _context(crtlib, case, case["shapes"][-1])
    _fieldpass_loop(crtlib, g, case, _settings(crtlib, case))
    loop = _result(g)
    g.close()
    np.testing.assert_array_equal(loop[0], got[0])
    assert loop[1] == got[1]
    np.testing.assert_array_equal(loop[2], got[2])


def test_cli_keywords_are_the_cli_schedule(crtlib):
    """CRT.stills(interlaced, first_field, frames) without a schedule = the schedule of crt_main.c"""
    for cid, kw in (("ntsc-cli-noise0", dict()), ("ntsc-cli-field1-noise24", dict(first_field=1)),
                    ("ntsc-progressive-rgb-duprows", dict(interlaced=False))):
        case = SC.case(cid)
        g = _context(crtlib, case)
        g.stills(_settings(crtlib, case), case["noise"], **kw)
        _compare(case, SC.expected(case), _result(g), cid + " by keywords")
        g.close()


def _launches(crtlib, case, noise, call):
    g = _context(crtlib, case)
    s = _settings(crtlib, case)
    g.fieldpass(s, noise)                                   # the cached tables are built by a call that is not counted
    g.synchronize()
    g.profile(True)
    call(g, s)
    cnt = g.profile_read()
    g.profile(False)
    g.close()
    return cnt["active"][1], cnt["decode"][1]


def test_noise0_encodes_every_distinct_entry_once(crtlib):
    """crthip_profile_enable counts the launches: the encoder's active-video kernel runs once per distinct entry at noise 0 (4 for
    the interlaced CLI schedule, 1 for the progressive one) and once per pass at noise 24; the decoder always once per pass"""
    case = SC.case("ntsc-cli-noise0")
    act1, dec1 = _launches(crtlib, case, 0, lambda g, s: g.fieldpass(s, 0))
    assert act1 >= 1 and dec1 >= 1
    assert _launches(crtlib, case, 24, lambda g, s: g.fieldpass(s, 24)) == (act1, dec1)
    assert _launches(crtlib, case, 0, lambda g, s: g.stills(s, 0)) == (4 * act1, 8 * dec1)
    assert _launches(crtlib, case, 0, lambda g, s: g.stills(s, 0, interlaced=False)) == (1 * act1, 4 * dec1)
    assert _launches(crtlib, case, 24, lambda g, s: g.stills(s, 24)) == (8 * act1, 8 * dec1)
    assert _launches(crtlib, case, 24, lambda g, s: g.stills(s, 24, interlaced=False)) == (4 * act1, 4 * dec1)
    assert len(SC.distinct_entries(dict(sched=SC.CUSTOM5))) == 3
    assert _launches(crtlib, case, 0, lambda g, s: g.stills(s, 0, schedule=SC.CUSTOM5)) == (3 * act1, 5 * dec1)


def _oracle_step(case, crts, imgs, sched, noise, geo):
    """`sched` on the oracle's television sets as they stand -> what _result gives"""
    for k, c in enumerate(crts):
        pad = np.concatenate([imgs[k], imgs[k][-1:]], axis=0)
        for field, frame, _aux in sched:
            c.settings(pad, format=R.FMT_BGRA, w=case["inp"][0], h=case["inp"][1], as_color=1, field=field & 1, frame=frame & 1, **geo)
            c.analog[:] = 0                  # every field-pass starts from a crt_init-clean analog[] (crt_hip.h): the offsets change
            c.modulate()
            c.demodulate(noise)
    return [(c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn"), np.array(c.ccf)) for c in crts]


def test_call_history_on_one_context(crtlib):
    """stills at noise 0, a field-pass at noise 24, stills at noise 24, stills at noise 0 with another x offset and schedule, a
    sequence -- on ONE context, the television sets carried from call to call, every step against the oracle: nothing of the shared
    signal leaks into the calls behind it, nor the other way round (forced shape: the padded signal lines, whose shift follows the
    x offset)"""
    import torch
    case = dict(SC.case("ntsc-cli-noise0"))
    n, imgs = case["n"], SC.images(case)
    orc = R.Oracle("ntsc")
    crts = []
    for _ in range(n):
        c = orc.new_crt(case["outw"], case["outh"], case["ofmt"])
        for a, v in case["knobs"].items():
            c.set(a, v)
        crts.append(c)
    g = _context(crtlib, case, 1)

    def check(want, what):
        _compare(case, want, _result(g), what)

    g.stills(_settings(crtlib, case), 0)
    check(_oracle_step(case, crts, imgs, SC.INTERLACED0, 0, {}), "1: stills at noise 0")
    s = _settings(crtlib, case)
    s.field, s.frame = 1, 0
    g.fieldpass(s, 24)
    check(_oracle_step(case, crts, imgs, [(1, 0, 0)], 24, {}), "2: fieldpass at noise 24")
    g.stills(_settings(crtlib, case), 24, interlaced=False)
    with pytest.raises(RuntimeError):
        g.fieldpass_signal()                                 # refused after a stills call (crt_hip.h)
    check(_oracle_step(case, crts, imgs, SC.PROGRESSIVE, 24, {}), "3: stills at noise 24, progressive")
    geo = dict(xoffset=12, yoffset=0)
    g.stills(_settings(crtlib, case, **geo), 0, schedule=SC.CUSTOM5)
    check(_oracle_step(case, crts, imgs, SC.CUSTOM5, 0, geo), "4: stills at noise 0, another x offset and schedule")
    # 5: the n images as n consecutive fields of the FIRST set (state and picture of set 0 carried on), blend off (sequence mode
    # with blend needs one line per row)
    g.blend = 0
    crts[0].set("blend", 0)
    par = [(k & 1, ((k + 1) >> 1) & 1) for k in range(n)]
    s = _settings(crtlib, case)
    s.field, s.frame = [a for a, _ in par], [b for _, b in par]
    init = g.out[0].clone()
    g.sequence(s, 24, out_init=init)
    torch.cuda.synchronize()
    out, st, _ = _result(g)
    c = crts[0]
    for k in range(n):
        pad = np.concatenate([imgs[k], imgs[k][-1:]], axis=0)
        c.settings(pad, format=R.FMT_BGRA, w=case["inp"][0], h=case["inp"][1], as_color=1, field=par[k][0], frame=par[k][1], xoffset=0, yoffset=0)
        c.analog[:] = 0
        c.modulate()
        c.demodulate(24)
        assert st[k] == (c.get("hsync"), c.get("vsync"), c.get("rn")), "5: sequence, state after field %d" % k
        np.testing.assert_array_equal(out[k].reshape(-1), c.out, err_msg="5: sequence, picture after field %d" % k)
    g.close()


def test_reserved_workspace_and_a_second_identical_call(crtlib):
    """after stills_reserve a second identical call (same inputs, the television sets powered on again) gives identical results"""
    case = SC.case("ntsc-cli-noise0")
    g = _context(crtlib, case, 2)
    g.reserve()
    g.stills_reserve(4)
    s = _settings(crtlib, case)
    g.stills(s, 0)
    first = _result(g)
    _compare(case, SC.expected(case), first, "first call")
    g.out.zero_()
    g.state.zero_()
    g.state[:, crtlib.ST_RN] = 194
    g.stills(s, 0)
    second = _result(g)
    np.testing.assert_array_equal(first[0], second[0])
    assert first[1] == second[1]
    np.testing.assert_array_equal(first[2], second[2])
    g.close()


def test_captured_stills_call_replays_to_the_eager_result(crtlib):
    """one stills call captured into a HIP graph (the way tests/test_gpu_context_reuse.py captures a field-pass: a stream of the
    test's own, the workspace reserved before) and replayed = the eager call = the oracle"""
    import torch
    case = SC.case("ntsc-cli-noise0")
    want = SC.expected(case)
    g = _context(crtlib, case, 1)
    g.reserve()
    g.stills_reserve(len(SC.distinct_entries(case)))
    stream = torch.cuda.Stream()
    g.use_stream(stream)
    s = _settings(crtlib, case)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        g.stills(s, 0)
    torch.cuda.synchronize()
    assert bool((g.out == 0).all()), "a capture runs nothing"
    graph.replay()
    torch.cuda.synchronize()
    _compare(case, want, _result(g), "replayed graph")
    del graph
    g.close()


def _raw(g, p, s, n_passes, sched, out=True):
    return g.L.crthip_stills(g.ctx, C.byref(p), g.n, C.c_void_p(s.data.data_ptr()), g._image_stride(s),
                             C.c_void_p(g.out.data_ptr()) if out else None, g.out.stride(0), C.c_void_p(g.state.data_ptr()), n_passes, sched)


def test_refusals_leave_pictures_and_states_alone(crtlib):
    """n_passes <= 0 or > CRTHIP_STILLS_MAX_PASSES, no schedule, and what crthip_fieldpass refuses (a rectangle that leaves analog[],
    the decoder's argument checks, a null pointer, unfinalized parameters): -1, a message, d_out still holds its fill pattern and
    d_state its values; the context works afterwards"""
    import torch
    case = SC.case("ntsc-cli-noise0")
    g = _context(crtlib, case)
    s = _settings(crtlib, case)
    p = g.params(s, 0)
    sched = (crtlib.Pass * 65)()
    g.out.fill_(0x5a)
    state0 = g.state.clone()
    err = lambda: g.L.crthip_error_string(g.ctx)
    for bad in (0, -3, 65):
        assert _raw(g, p, s, bad, sched) == -1, bad
        assert b"n_passes" in err()
    assert _raw(g, p, s, 8, None) == -1
    assert b"sched" in err()
    assert _raw(g, p, s, 8, sched, out=False) == -1
    far = g.params(_settings(crtlib, case, yoffset=30), 0)
    assert _raw(g, far, s, 8, sched) == -1
    assert b"out of contract" in err()
    gains = g.params(s, 0)
    gains.eq_g[0][1] += 1
    assert _raw(g, gains, s, 8, sched) == -1
    assert b"equaliser gains" in err()
    raw = g.params(s, 0)
    raw.finalized = 0
    assert _raw(g, raw, s, 8, sched) == -1
    with pytest.raises(ValueError):
        g.stills(s, 0, schedule=[])
    with pytest.raises(RuntimeError):
        g.stills(_settings(crtlib, case, yoffset=30), 0)
    g.synchronize()
    assert bool((g.out == 0x5a).all()) and torch.equal(g.state, state0)
    g.out.zero_()
    g.stills(s, 0)                                          # and the context still works
    _compare(case, SC.expected(case), _result(g), "after the refusals")
    g.close()


def test_stills_dir_tool_writes_the_files_of_the_reference_program(tmp_path):
    """tools/stills_dir.py on three generated PPMs of two sizes: byte-identical to the reference's `ntsc` program where it was
    built, to the oracle's still written as PPM otherwise"""
    src, dst = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    pics = {"a": R.synth_image(80, 60, 4, 11), "b": R.synth_image(80, 60, 4, 12, "bars"), "c": R.synth_image(64, 48, 4, 13)}
    for name, bgra in pics.items():
        bgra[:, :, 3] = 0
        SC.write_ppm(str(src / (name + ".ppm")), bgra[:, :, 2::-1])
    outw, outh = 160, 120
    exe = os.path.join(R.REF_DIR, "ntsc_cli")
    for flags, kw in (("-o", dict(interlaced=True)), ("-opf", dict(interlaced=False, first_field=1))):
        r = subprocess.run([sys.executable, os.path.join(R.ROOT, "tools", "stills_dir.py"), flags, str(outw), str(outh), "0", "0",
                            str(src), str(dst)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        for name, bgra in pics.items():
            with open(str(dst / (name + ".ppm")), "rb") as f:
                got = f.read()
            if os.path.exists(exe):
                ref = str(tmp_path / ("ref_" + name + ".ppm"))
                subprocess.run([exe, flags, str(outw), str(outh), "0", "0", str(src / (name + ".ppm")), ref], check=True, capture_output=True)
                with open(ref, "rb") as f:
                    want = f.read()
            else:
                want = b"P6\n%d %d\n255\n" % (outw, outh) + SC.cli_still(R.Oracle("ntsc"), bgra, outw, outh, 0, **kw).tobytes()
            assert got == want, "%s %s" % (flags, name)

"""crthip_fieldpass_sizes / crthip_stills_sizes on the GPU: batches whose fields differ in image size against the checker's loop of
batch-1 calls (tests/sizes_cases.py; pinned to the real reference by tests/test_sizes_cpu.py, and compared with the reference's own
bytes here where oracle/_ref has the build) -- inp[] (crthip_fieldpass_signal), ccf, hsync / vsync / rn and the picture, bit for bit;
no field of any case is left out (asserted)."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import fence as F
import sizes_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_fieldpass_sizes")
    return crtlib


_WANT = {}


def _want(case, schedule=None):
    """the checker's loop for a case, computed once and shared (left unchanged by its users); the oracle's, after it was compared
    with the reference's own bytes where the reference build travels with the tree"""
    key = (case, tuple(schedule) if schedule else None)
    if key not in _WANT:
        name = SC.CASES[case]["name"]
        got = SC.checker_fields(R.Oracle(name), case, schedule=schedule)
        if R.have_ref(name):
            ref = SC.checker_fields(R.RefLib(name), case, schedule=schedule)
            for k in range(min(len(got), SC.CASES[case].get("distinct", len(got)))):
                for a, b in zip(got[k], ref[k]):
                    for f in ("inp", "out", "ccf"):
                        np.testing.assert_array_equal(a[f], b[f], err_msg="%s field %d: oracle against the reference, %s" % (case, k, f))
                    assert (a["hsync"], a["vsync"], a["rn"]) == (b["hsync"], b["vsync"], b["rn"])
        _WANT[key] = got
    return _WANT[key]


def _make(crtlib, case, shape=1, sig_pad=1, exact=0, sig_tile=0, overlap=None, out=None):
    c = SC.CASES[case]
    name, n = c["name"], len(c["sizes"])
    g = crtlib.CRT(n, SC.OUTW, SC.OUTH, crtlib.FMT_BGRA, name[:4] if name.startswith("ntscfir") else name, device=0, out=out)
    g.eq_fir = R.EQ_KERNEL.get(name, 0)
    g.scanlines = 1
    for a, v in c.get("crt_knobs", {}).items():
        setattr(g, a, v)
    g.set_shape(shape)
    g.set_signal_layout(sig_pad)
    g.set_exact(bool(exact))
    g.set_signal_tile(sig_tile)
    if overlap:
        g.set_overlap(overlap)
    if "seeds" in c:
        g.srand(c["seeds"])
    par = [SC.parity(k) for k in range(n)]
    dc = R.Oracle(name).system in R.DOT_CRAWL_SYSTEMS
    s = crtlib.Settings(None, format=c["fmt"], as_color=1, field=[a for a, _ in par], frame=[b for _, b in par],
                        dot_crawl_offset=[SC.dot_crawl(name, k) for k in range(n)] if dc else 0, spare_row=c["spare"])
    return g, s


def _device_layout(case):
    import torch
    buf, sizes = SC.layout(case)
    return torch.from_numpy(buf).to("cuda:0"), sizes


def _next_parity(s, step):
    s.field = [f ^ 1 for f in s.field]
    if step % 2 == 0:
        s.frame = [f ^ 1 for f in s.frame]


def _compare(g, want, step, what, signal=True):
    g.synchronize()
    gout = g.out.cpu().numpy()
    hs, vs, rn, ccf = g.get("hsync"), g.get("vsync"), g.get("rn"), g.ccf
    sig = g.fieldpass_signal()[0].cpu().numpy() if signal else None
    for k in range(len(want)):
        w = want[k][step]
        tag = "%s pass %d field %d" % (what, step, k)
        assert not w["undefined"], tag + ": inside the reference's undefined over-read -- choose other inputs, exclude nothing"
        if sig is not None:
            np.testing.assert_array_equal(sig[k, :w["inp"].shape[0]], w["inp"], err_msg=tag + " inp")
        assert (hs[k], vs[k], rn[k]) == (w["hsync"], w["vsync"], w["rn"]), tag + " hsync / vsync / rn"
        np.testing.assert_array_equal(ccf[k, :w["ccf"].shape[0], :w["ccf"].shape[1]], w["ccf"], err_msg=tag + " ccf")
        np.testing.assert_array_equal(gout[k].reshape(-1), w["out"], err_msg=tag + " out")


def _run_case(crtlib, case, what, **kw):
    want = _want(case)
    g, s = _make(crtlib, case, **kw)
    images = _device_layout(case)
    for step in range(SC.STEPS):
        g.fieldpass_sizes(images, SC.CASES[case]["noise"], settings=s)
        _compare(g, want, step, case + " " + what)
        _next_parity(s, step)
    g.close()


PLAIN = sorted(c for c in SC.CASES if not c.startswith("stills") and c != "many")


@pytest.mark.parametrize("case", PLAIN)
def test_every_case_equals_the_loop_of_batch_one_calls(crtlib, case):
    _run_case(crtlib, case, "default")


@pytest.mark.parametrize("case", ["scale", "tiles", "heights_tight", "rgb_odd", "wide_only"])
@pytest.mark.parametrize("sig_pad,exact,shape", [(0, 0, 1), (1, 1, 1), (0, 1, 2), (1, 0, 2), (1, 0, 0)])
def test_layouts_exact_kernels_and_the_shape_setting(crtlib, case, sig_pad, exact, shape):
    """flat and padded signal lines, the exact (32-bit) encoder instantiations, and crthip_set_shape: shape 2 (and the automatic
    choice, which gives so small a batch to the scanline-parallel shape) leaves a sizes call's ENCODER in the lane-per-scanline
    shape -- a documented no-op, not an error -- while the decoder follows it"""
    _run_case(crtlib, case, "pad %d exact %d shape %d" % (sig_pad, exact, shape), sig_pad=sig_pad, exact=exact, shape=shape)


@pytest.mark.parametrize("case", ["scale", "wide_only"])
@pytest.mark.parametrize("tile", [16, 32, 64])
def test_signal_tiles(crtlib, case, tile):
    """the 64-, 128- and 256-byte signal pieces (crthip_set_signal_tile) beside the narrow and the wide image tile"""
    _run_case(crtlib, case, "signal tile %d" % tile, sig_tile=tile)


@pytest.mark.parametrize("tile", [16, 32])
def test_image_tile_choice_gives_identical_bytes(crtlib, tile):
    """the wide image tile on narrow images and the narrow one on wide images (crthip_set_pixel_tile's encoder half)"""
    for case in ("tiles", "wide_mixed"):
        want = _want(case)
        g, s = _make(crtlib, case)
        g.L.crthip_set_pixel_tile(g.ctx, tile)
        g.fieldpass_sizes(_device_layout(case), SC.CASES[case]["noise"], settings=s)
        _compare(g, want, 0, "%s image tile %d" % (case, tile))
        g.close()


def test_overlap_chunks(crtlib):
    """520 fields in two overlap chunks: the record pointer is offset per chunk like every other per-field pointer"""
    _run_case(crtlib, "many", "overlap 2", overlap=2)


def test_equal_sizes_give_the_uniform_call(crtlib):
    """a batch whose sizes are all equal == crthip_fieldpass, byte for byte and state for state"""
    import torch
    n, w, h = 6, 100, 37
    imgs = np.stack([R.synth_image(w, h + 1, 4, 99 + k) for k in range(n)])
    dev = torch.from_numpy(imgs).to("cuda:0")
    par = [SC.parity(k) for k in range(n)]
    res = []
    for sizes_call in (False, True):
        g = crtlib.CRT(n, SC.OUTW, SC.OUTH, crtlib.FMT_BGRA, "ntsc", device=0)
        g.scanlines = 1
        g.set_shape(1)
        s = crtlib.Settings(dev[:, :h], format=crtlib.FMT_BGRA, as_color=1, field=[a for a, _ in par], frame=[b for _, b in par], spare_row=True)
        if sizes_call:
            g.fieldpass_sizes([dev[k] for k in range(n)], 24, settings=s)
        else:
            g.fieldpass(s, 24)
        g.synchronize()
        res.append((g.out.cpu().numpy(), g.state.cpu().numpy(), g.fieldpass_signal()[0].cpu().numpy()))
        g.close()
    for a, b, what in zip(res[0], res[1], ("out", "state", "inp")):
        np.testing.assert_array_equal(a, b, err_msg=what)


CLI = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 0)]


@pytest.mark.parametrize("case", ["stills0", "stills12"])
def test_stills_sizes_equals_the_loop(crtlib, case):
    """the interlaced CLI schedule: noise 0 takes the shared clean signal (4 encoder runs for 8 passes), noise 12 encodes per pass;
    both equal the checker's loop of field-passes and the loop of fieldpass_sizes calls"""
    assert crtlib.stills_schedule(True, 0, 4) == CLI
    want = _want(case, CLI)
    noise = SC.CASES[case]["noise"]
    g, s = _make(crtlib, case)
    g.stills_sizes(_device_layout(case), noise, settings=s)
    _compare(g, want, len(CLI) - 1, case, signal=False)
    with pytest.raises(RuntimeError):
        g.fieldpass_signal()
    stills_out, stills_state = g.out.cpu().numpy(), g.state.cpu().numpy()
    g.close()
    g, s = _make(crtlib, case)
    images = _device_layout(case)
    for field, frame, aux in CLI:
        s.field, s.frame = field, frame
        g.fieldpass_sizes(images, noise, settings=s)
    g.synchronize()
    np.testing.assert_array_equal(g.out.cpu().numpy(), stills_out)
    np.testing.assert_array_equal(g.state.cpu().numpy(), stills_state)
    g.close()


def test_graph_capture_with_records_rewritten_between_replays(crtlib):
    """captured after crthip_reserve: nothing is allocated, nothing synchronises; the records are read at replay -- a replay after
    the records were permuted (inside the captured env: the same sizes, other fields) gives the permuted batch's result"""
    import torch
    case = "scale"
    want = _want(case)
    n = len(want)
    g, s = _make(crtlib, case)
    g.reserve()
    side = torch.cuda.Stream()
    g.use_stream(side)
    buf, sizes = _device_layout(case)
    p = g.sizes_params(s, SC.CASES[case]["noise"])
    g._load_field_state(s)
    torch.cuda.synchronize()
    state0 = g.state.clone()
    g.upload_sizes((buf, sizes), p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.fieldpass_sizes(None, SC.CASES[case]["noise"], params=p, settings=s)
    g.out.zero_()
    g.state.copy_(state0)
    graph.replay()
    torch.cuda.synchronize()
    _compare(g, want, 0, "replay 1", signal=False)
    # the records of fields 0 and 4 swapped: each field now reads the other's image with the other's size, its own parity
    perm = list(range(n))
    perm[0], perm[4] = 4, 0
    recs, env = crtlib.sizes_prepare(p, sizes[perm])
    assert bytes(env) == bytes(g._size_env)
    g.size_recs.copy_(torch.from_numpy(recs.view("int32")))
    g.out.zero_()
    g.state.copy_(state0)
    graph.replay()
    torch.cuda.synchronize()
    out = g.out.cpu().numpy()
    for k in (1, 2, 3, 5):
        np.testing.assert_array_equal(out[k].reshape(-1), want[k][0]["out"], err_msg="replay 2 field %d" % k)
    # fields 0 and 4 have the same parity (k & 1, (k >> 1) & 1 differ: 0 -> (0, 0), 4 -> (0, 0)): the swapped pictures are each other's
    assert SC.parity(0) == SC.parity(4)
    np.testing.assert_array_equal(out[0].reshape(-1), want[4][0]["out"], err_msg="replay 2 field 0 = field 4's image")
    np.testing.assert_array_equal(out[4].reshape(-1), want[0][0]["out"], err_msg="replay 2 field 4 = field 0's image")
    g.close()


def test_refusals_leave_out_and_state_untouched(crtlib):
    import torch
    case = "scale"
    g, s = _make(crtlib, case)
    L = g.L
    buf, sizes = _device_layout(case)
    p = g.sizes_params(s, 24)
    recs, env = crtlib.sizes_prepare(p, sizes)
    drecs = torch.zeros((g.n + 1, crtlib.SIZE_REC_INTS), dtype=torch.int32, device="cuda:0")
    drecs[:g.n].copy_(torch.from_numpy(recs.view("int32")))
    g.out.fill_(0x5A)
    g.state[:, 0] = 7
    out0, state0 = g.out.clone(), g.state.clone()
    vp = C.c_void_p

    def call(params=p, images=buf.data_ptr(), rec_ptr=drecs.data_ptr(), e=env, n=g.n):
        return L.crthip_fieldpass_sizes(g.ctx, C.byref(params), n, vp(images), vp(g.out.data_ptr()), g.out.stride(0),
                                        vp(g.state.data_ptr()), vp(rec_ptr), C.byref(e) if e is not None else None)

    def refused(rc, word):
        assert rc == -1
        msg = L.crthip_error_string(g.ctx).decode()
        assert word in msg, msg
        g.synchronize()
        assert torch.equal(g.out, out0) and torch.equal(g.state, state0)
    bad = crtlib.SizesEnv.from_buffer_copy(bytes(env))
    bad.magic ^= 1
    refused(call(e=bad), "crthip_sizes_prepare")
    bad = crtlib.SizesEnv.from_buffer_copy(bytes(env))
    bad.n += 1
    refused(call(e=bad), "another number of fields")
    bad = crtlib.SizesEnv.from_buffer_copy(bytes(env))
    bad.extent_lo, bad.extent_hi = 3, 0
    refused(call(e=bad), "contradict")
    refused(call(rec_ptr=drecs.data_ptr() + 2), "alignment")
    refused(call(images=buf.data_ptr() + 2), "alignment")
    raw = g.sizes_params(crtlib.Settings(None, format=crtlib.FMT_BGRA, raw=1, spare_row=True), 24)
    refused(call(params=raw), "raw")
    assert call(e=None) == -1 and call(rec_ptr=0) == -1 and call(images=0) == -1
    g.synchronize()
    assert torch.equal(g.out, out0) and torch.equal(g.state, state0)
    sched = (crtlib.Pass * 2)()
    rc = L.crthip_stills_sizes(g.ctx, C.byref(raw), g.n, vp(buf.data_ptr()), vp(g.out.data_ptr()), g.out.stride(0),
                               vp(g.state.data_ptr()), 2, sched, vp(drecs.data_ptr()), C.byref(env))
    refused(rc, "raw")
    g.close()
    nes = crtlib.CRT(1, SC.OUTW, SC.OUTH, crtlib.FMT_BGRA, "nes", device=0)
    pn = crtlib.make_params("nes", w=256, h=240, outw=SC.OUTW, outh=SC.OUTH, out_format=crtlib.FMT_BGRA)
    env1 = crtlib.SizesEnv.from_buffer_copy(bytes(env))
    env1.n = 1
    nes.out.fill_(0x5A)
    nes.state[:, 0] = 7
    nes_out0, nes_state0 = nes.out.clone(), nes.state.clone()
    rc = L.crthip_fieldpass_sizes(nes.ctx, C.byref(pn), 1, vp(buf.data_ptr()), vp(nes.out.data_ptr()), nes.out.stride(0),
                                  vp(nes.state.data_ptr()), vp(drecs.data_ptr()), C.byref(env1))
    assert rc == -1 and "NES" in L.crthip_error_string(nes.ctx).decode()
    nes.synchronize()
    assert torch.equal(nes.out, nes_out0) and torch.equal(nes.state, nes_state0)
    nes.close()


def test_records_outside_the_extent_read_nothing_outside_it(crtlib):
    """records that do not come from the prepare call that made the env (a graph replay after a bad rewrite): the call runs, and the
    fields beside the bad records (0, 2 and 5) still equal the oracle -- a wavefront takes nothing from another field's record.  That
    the bad records themselves form no address outside the extent is not something a GPU test can see (reads leave no trace, and a
    fault is no test result): tests/test_sizes_cpu.py runs the guard's own code over hostile records on the host.  The image buffer
    is read only and is checked for that."""
    import torch
    case = "scale"
    want = _want(case)
    g, s = _make(crtlib, case)
    buf, sizes = SC.layout(case)
    fb = F.Fenced(1, buf.size, device="cuda:0", name="images")
    pre = fb.prefill(5, buf[None])
    p = g.sizes_params(s, SC.CASES[case]["noise"])
    g._load_field_state(s)
    g.upload_sizes((fb.view((buf.size,))[0], sizes), p)
    recs = g.size_recs.cpu().numpy().copy()
    recs[1, crtlib.SZ_OFF_LO] = buf.size - 64              # the image would end far behind the extent
    recs[3, crtlib.SZ_STEP_HI] = -2 ** 31                  # col_step_hi = 0x80000000: the column is negative from sample 1 on
    recs[4, crtlib.SZ_W] = 1 << 20                         # a row wider than the whole buffer
    recs[4, crtlib.SZ_H] = -5
    g.size_recs.copy_(torch.from_numpy(recs))
    g.fieldpass_sizes(None, SC.CASES[case]["noise"], params=p, settings=s)
    g.synchronize()
    out = g.out.cpu().numpy()
    for k in (0, 2, 5):
        np.testing.assert_array_equal(out[k].reshape(-1), want[k][0]["out"], err_msg="field %d beside the bad records" % k)
    fb.assert_unchanged(pre)
    g.close()


def test_long_lived_context(crtlib):
    """sizes call, uniform call, sizes call with other sizes on ONE context: each equals a fresh context's result"""
    import torch
    g, s = _make(crtlib, "scale")
    g.fieldpass_sizes(_device_layout("scale"), SC.CASES["scale"]["noise"], settings=s)
    _compare(g, _want("scale"), 0, "first sizes call")
    # a uniform call through the same context
    n, w, h = g.n, 64, 48
    imgs = np.stack([R.synth_image(w, h + 1, 4, 500 + k) for k in range(n)])
    su = crtlib.Settings(torch.from_numpy(imgs).to("cuda:0")[:, :h], format=crtlib.FMT_BGRA, as_color=1, field=s.field, frame=s.frame, spare_row=True)
    fresh = crtlib.CRT(n, SC.OUTW, SC.OUTH, crtlib.FMT_BGRA, "ntsc", device=0)
    fresh.scanlines = 1
    fresh.set_shape(1)
    for c in (g, fresh):
        c.out.zero_()
        c.state.zero_()
        c.state[:, 5] = 194
        c.fieldpass(su, 24)
        c.synchronize()
    assert torch.equal(g.out, fresh.out) and torch.equal(g.state, fresh.state)
    fresh.close()
    # other sizes: every field now has another field's image and size
    g.out.zero_()
    g.state.zero_()
    g.state[:, 5] = 194
    perm = [5, 4, 3, 2, 1, 0]
    buf, sizes = _device_layout("scale")
    g.fieldpass_sizes((buf, sizes[perm]), SC.CASES["scale"]["noise"], settings=s)
    g.synchronize()
    f2, s2 = _make(crtlib, "scale")
    f2.fieldpass_sizes((buf, sizes[perm]), SC.CASES["scale"]["noise"], settings=s2)
    f2.synchronize()
    assert torch.equal(g.out, f2.out) and torch.equal(g.state, f2.state)
    f2.close()
    g.close()


@pytest.mark.parametrize("case", ["scale", "heights_tight", "rgb_odd"])
def test_fenced_buffers(crtlib, case):
    """images packed with no slack inside a fenced allocation, d_out and d_state fenced too, two random fills: the payloads equal the
    oracle, nothing outside d_out and d_state is written, the image buffer is unchanged, and the result does not depend on the fill"""
    import torch
    want = _want(case)
    buf, sizes = SC.layout(case)
    n = len(want)
    outs = []
    for seed in (11, 12):
        fi = F.Fenced(1, buf.size, device="cuda:0", name="images")
        fo = F.Fenced(n, SC.OUTW * SC.OUTH * 4, pitch=SC.OUTW * 4, device="cuda:0", name="d_out")
        fs = F.Fenced(n, 144, device="cuda:0", name="d_state")
        pre_i = fi.prefill(seed, buf[None])
        pre_o = fo.prefill(seed + 100, np.zeros((n, SC.OUTW * SC.OUTH * 4), dtype=np.uint8))
        st = np.zeros((n, 36), dtype=np.int32)
        st[:, 5] = 194
        pre_s = fs.prefill(seed + 200, st)
        g, s = _make(crtlib, case, out=fo.view((SC.OUTH, SC.OUTW, 4)))
        g.state = fs.view((36,), torch.int32)
        g.fieldpass_sizes((fi.view((buf.size,))[0], sizes), SC.CASES[case]["noise"], settings=s)
        _compare(g, want, 0, "%s fenced, fill %d" % (case, seed))
        fi.assert_unchanged(pre_i)
        fo.assert_fence_intact(pre_o)
        fs.assert_fence_intact(pre_s)
        outs.append((fo.payloads(), fs.payloads()))
        g.close()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_stills_dir_one_call_writes_the_grouped_path_files(crtlib, tmp_path):
    """tools/stills_dir.py --one-call: a folder of mixed-size pictures through ONE stills_sizes call, its output files byte-identical
    to the grouped default's"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("stills_dir", os.path.join(R.ROOT, "tools", "stills_dir.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = tmp_path / "in"
    src.mkdir()
    for k, (w, h) in enumerate([(40, 30), (17, 9), (40, 30), (300, 5), (8, 100)]):
        tool.write_ppm(str(src / ("pic%d.ppm" % k)), R.synth_image(w, h, 3, 70 + k))
    for flags, noise in (("-o", 0), ("-f", 12)):
        a, b = tmp_path / ("grouped" + flags), tmp_path / ("one" + flags)
        assert tool.main(["stills_dir.py", flags, "64", "48", str(noise), "5", str(src), str(a)]) == 0
        assert tool.main(["stills_dir.py", "--one-call", flags, "64", "48", str(noise), "5", str(src), str(b)]) == 0
        names = sorted(os.listdir(str(a)))
        assert names == sorted(os.listdir(str(b))) and len(names) == 5
        for name in names:
            assert (a / name).read_bytes() == (b / name).read_bytes(), name

"""GPU parity of the phosphor display modes (CRTHIP_F_PHOSPHOR_FADE / _CLEAR, include/crt_hip.h) against the CPU oracle running the
reference's live-viewer loop (crt_main.c:454-463 displaycb): for every field the output buffer is faded (crt_main.c:438-451) or
cleared (:462) first, then crt_modulate / crt_demodulate run onto it.  Bit-exact, tolerance 0.  Where the compiled reference exists
(oracle/_ref) the same loop runs through it too.

Every parity test also checks, on the CPU side, that the expected fade / clear pictures differ from the keep-mode pictures of the same
loop: the library before these flags ignores the unknown bits and must fail here."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

import crtref as R
from test_phosphor_cpu import display_step_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _padded(imgs):
    """[n,h,w,c] -> device view inside an [n,h+1,...] allocation (row h readable: crt_ntsc.c:263)"""
    import torch
    n, h = imgs.shape[0], imgs.shape[1]
    full = torch.zeros((n, h + 1) + tuple(imgs.shape[2:]), dtype=torch.uint8, device="cuda:0")
    full[:, :h] = _to_dev(imgs)
    full[:, h] = full[:, h - 1]
    return full[:, :h]


def _frames(name, n, seed, iw=640, ih=480):
    orc_sys = R.SYSTEMS[name][0]
    if orc_sys == R.SYS_NES:
        return np.stack([R.synth_ppu(256, 240, seed + k) for k in range(n)])
    if orc_sys == R.SYS_NESRGB:
        iw, ih = 256, 240
    return np.stack([R.synth_image(iw, ih, 4, seed + k, "random" if k % 3 else "bars") for k in range(n)])


def _field_settings(name, frame, k, field, frame_bit):
    """keyword settings of field k for the oracle / reference (the sequence-mode tests' choices)"""
    sysid = R.SYSTEMS[name][0]
    pad = np.concatenate([frame, frame[-1:]], axis=0)
    if sysid == R.SYS_NES:
        return pad, dict(w=256, h=240, dot_crawl_offset=k % 3, hue=0), None
    h, w = frame.shape[0], frame.shape[1]
    if sysid == R.SYS_NESRGB:
        return pad, dict(format=R.FMT_BGRA, w=w, h=h, dot_crawl_offset=k % 3, hue=0), None
    kw = dict(format=R.FMT_BGRA, w=w, h=h, as_color=1, field=field, frame=frame_bit)
    return pad, kw, (k % 3 if sysid in R.DOT_CRAWL_SYSTEMS else None)


def _live_loop(lib, name, outw, outh, ofmt, knobs, mode, init, frames, parities, noise, hs0=7, vs0=2):
    """the reference's real-time loop on ONE set: per field  display step (fade / clear / keep);  crt_modulate;  crt_demodulate.
    lib: R.Oracle(name) or R.RefLib(name).  Returns [(out, hsync, vsync, rn)] after every field."""
    c = lib.new_crt(outw, outh, ofmt)
    for k, v in knobs.items():
        c.set(k, v)
    c.out[:] = init.reshape(-1)
    c.set("hsync", hs0)
    c.set("vsync", vs0)
    want = []
    for k in range(len(frames)):
        if mode != "keep":
            c.out[:] = display_step_np(c.out, ofmt, mode)          # in place: the set keeps its buffer pointer
        pad, kw, dco = _field_settings(name, frames[k], k, *parities[k])
        c.settings(pad, **kw)
        if dco is not None:
            c.sset("dot_crawl_offset", dco)
        c.modulate()
        c.demodulate(noise)
        want.append((c.out.copy(), c.get("hsync"), c.get("vsync"), c.get("rn")))
    return want


def _expected(name, outw, outh, ofmt, knobs, mode, init, frames, parities, noise):
    """the oracle's live loop (and the compiled reference's, where it exists); asserts that the display mode shows"""
    want = _live_loop(R.Oracle(name), name, outw, outh, ofmt, knobs, mode, init, frames, parities, noise)
    if R.have_ref(name):
        ref = _live_loop(R.RefLib(name), name, outw, outh, ofmt, knobs, mode, init, frames, parities, noise)
        for k, (a, b) in enumerate(zip(want, ref)):
            np.testing.assert_array_equal(a[0], b[0], err_msg="oracle vs reference, %s field %d" % (mode, k))
            assert a[1:] == b[1:], "oracle vs reference state, %s field %d" % (mode, k)
    keep = _live_loop(R.Oracle(name), name, outw, outh, ofmt, knobs, "keep", init, frames, parities, noise)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(want, keep)), \
        "%s: the %s pictures equal the keep-mode pictures -- the case cannot tell the modes apart" % (name, mode)
    return want


def _sequence_settings(crtlib, name, frames, parities):
    import torch
    n = len(frames)
    sysid = R.SYSTEMS[name][0]
    if sysid == R.SYS_NES:
        full = torch.zeros((n, 241, 256), dtype=torch.int16, device="cuda:0")
        full[:, :240] = torch.from_numpy(frames.astype(np.int16)).to("cuda:0")
        return crtlib.Settings(full[:, :240], hue=0, dot_crawl_offset=[k % 3 for k in range(n)])
    return crtlib.Settings(_padded(frames), format=crtlib.FMT_BGRA, field=[a for a, _ in parities], frame=[b for _, b in parities],
                           dot_crawl_offset=[k % 3 for k in range(n)] if sysid in R.DOT_CRAWL_SYSTEMS else 0)


def _check_sequence(crtlib, name, outw, outh, ofmt, knobs, mode, noise, n, parities, shapes=(0,), seed=300):
    frames = _frames(name, n, seed)
    bpp = R.bpp4fmt(ofmt)
    init = R.lcg_bytes(outw * outh * bpp, 5).reshape(outh, outw, bpp)
    want = _expected(name, outw, outh, ofmt, knobs, mode, init, frames, parities, noise)
    for shape in shapes:
        g = crtlib.CRT(n, outw, outh, ofmt, name, device=0)
        for k, v in knobs.items():
            setattr(g, k, v)
        g.phosphor = mode
        g.set_shape(shape)
        g.state[0, crtlib.ST_HSYNC] = 7
        g.state[0, crtlib.ST_VSYNC] = 2
        g.sequence(_sequence_settings(crtlib, name, frames, parities), noise, out_init=_to_dev(init))
        g.synchronize()
        out = g.out.cpu().numpy()
        for k in range(n):
            o, hs, vs, rn = want[k]
            assert (g.get("hsync")[k], g.get("vsync")[k], g.get("rn")[k]) == (hs, vs, rn), "field %d state" % k
            np.testing.assert_array_equal(out[k].reshape(-1), o, err_msg="%s %s sequence shape %d field %d" % (name, mode, shape, k))
        g.close()


# At 320x240 with v_fac 0 every line of a field writes one output row and the lines cover every row (crt_core.c:428-431), so no row
# is ever carried over and the display mode cannot show; v_fac = 240 doubles the span (outh + v_fac) so that scanlines 1 leaves a gap
# row under every line -- rows a field does not write.
SMALL = dict(scanlines=1, v_fac=240)
SEQ_CASES = [("ntsc", 640, 480, R.FMT_BGRA, 24, dict(scanlines=1), (0,)),
             ("ntsc", 832, 624, R.FMT_RGB, 0, dict(scanlines=0), (0,)),
             ("ntsc", 320, 240, R.FMT_ARGB, 120, SMALL, (0,)),
             ("nes", 640, 480, R.FMT_BGRA, 12, dict(scanlines=1), (0,)),
             ("pv1k", 640, 480, R.FMT_BGRA, 30, dict(scanlines=0), (0,)),
             ("ntscbloom", 640, 480, R.FMT_BGRA, 24, dict(scanlines=1), (0, 1))]


@pytest.mark.parametrize("mode", ["fade", "clear"])
@pytest.mark.parametrize("case", range(len(SEQ_CASES)))
def test_sequence_display_modes(crtlib, case, mode):
    """crthip_sequence: image k = the display after field k, with a fade / clear of the whole display before every field"""
    import shard
    name, outw, outh, ofmt, noise, knobs, shapes = SEQ_CASES[case]
    n = 9
    _check_sequence(crtlib, name, outw, outh, ofmt, knobs, mode, noise, n, [shard.field_parity(k) for k in range(n)], shapes)


@pytest.mark.parametrize("mode", ["fade", "clear"])
@pytest.mark.parametrize("ofmt,scanlines,outsz", [(R.FMT_BGRA, 1, (640, 480)), (R.FMT_RGB, 0, (832, 624)), (R.FMT_ARGB, 1, (320, 240))])
def test_sequence_display_modes_with_blend(crtlib, ofmt, scanlines, outsz, mode):
    """blend = 1 (crt_main.c:528): the decoder blends against the faded (cleared) display -- the fold step fades the old row first"""
    import shard
    n = 9
    _check_sequence(crtlib, "ntsc", outsz[0], outsz[1], ofmt, dict(scanlines=scanlines, blend=1), mode, 24, n,
                    [shard.field_parity(k) for k in range(n)], seed=800)


@pytest.mark.parametrize("mode", ["fade", "clear"])
def test_sequence_fade_depth(crtlib, mode):
    """progressive fields with scanlines 1 (and v_fac 240, see SMALL): the gap rows are never written, so their age runs past 38 over
    48 fields (a wrong cap or a wrong table shows up there)"""
    n = 48
    _check_sequence(crtlib, "ntsc", 320, 240, R.FMT_BGRA, SMALL, mode, 24, n, [(0, 0)] * n, seed=4000)


class _LocalComm:
    """the subset of torch.distributed that shard.sequence_sharded uses, between threads of one process (several crtlib.CRT objects
    on one GPU play the ranks)"""

    class ReduceOp:
        MAX = "max"

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.mail = {}
        self.cv = threading.Condition()

    class _View:
        def __init__(self, comm, rank):
            self.c, self.rank, self.ReduceOp = comm, rank, _LocalComm.ReduceOp

        def all_gather(self, out, t):
            self.c.slots[self.rank] = t.clone()
            self.c.barrier.wait()
            for r in range(self.c.world):
                out[r].copy_(self.c.slots[r])
            self.c.barrier.wait()

        def all_reduce(self, t, op=None):
            self.c.slots[self.rank] = t.clone()
            self.c.barrier.wait()
            m = max(int(x.item()) for x in self.c.slots)
            self.c.barrier.wait()
            t.fill_(m)

        def send(self, t, dst):
            with self.c.cv:
                self.c.mail[(self.rank, dst)] = t.clone()
                self.c.cv.notify_all()

        def recv(self, t, src):
            with self.c.cv:
                self.c.cv.wait_for(lambda: (src, self.rank) in self.c.mail, timeout=120)
                t.copy_(self.c.mail.pop((src, self.rank)))

    def view(self, rank):
        return _LocalComm._View(self, rank)


# (scanlines 1 without blend: at 400x300 with scanlines 0 every field writes every row and the fade could not show)
@pytest.mark.parametrize("world,total,blend,scanlines", [(2, 9, 0, 1), (3, 10, 0, 1), (2, 7, 1, 0), (4, 5, 0, 1), (4, 3, 1, 1)])
def test_sequence_sharded_fade(crtlib, world, total, blend, scanlines):
    """shard.sequence_sharded (unchanged) over `world` crtlib.CRT objects with phosphor = "fade" equals single-context crthip_sequence
    with FADE: the placeholder weave + patch revisit gives the rows nobody in a block wrote fade^(k+1) of the predecessor's picture,
    and a rank with an empty block (the last one in (4, 5) and (4, 3)) passes the picture on unfaded -- no field ran there"""
    import torch
    import shard
    w, h, outw, outh, noise = 320, 240, 400, 300, 120
    frames = np.stack([R.synth_image(w, h, 4, 900 + k, "random" if k % 3 else "bars") for k in range(total)])
    init = torch.from_numpy(R.lcg_bytes(outh * outw * 4, 5).reshape(outh, outw, 4).copy()).to("cuda:0")

    def settings(lo, hi):
        full = torch.zeros((hi - lo, h + 1, w, 4), dtype=torch.uint8, device="cuda:0")
        full[:, :h] = torch.from_numpy(frames[lo:hi]).to("cuda:0")
        par = [shard.field_parity(k) for k in range(lo, hi)]
        return crtlib.Settings(full[:, :h], format=crtlib.FMT_BGRA, field=[a for a, _ in par], frame=[b for _, b in par])

    def results(mode):
        one = crtlib.CRT(total, outw, outh, crtlib.FMT_BGRA, "ntsc", device=0)
        one.scanlines, one.blend, one.phosphor = scanlines, blend, mode
        one.state[0, crtlib.ST_HSYNC] = 7
        one.state[0, crtlib.ST_VSYNC] = 2
        one.sequence(settings(0, total), noise, out_init=init)
        one.synchronize()
        r = one.out.cpu().numpy(), [one.get(f) for f in ("hsync", "vsync", "rn")]
        one.close()
        return r

    want, want_state = results("fade")
    keep, _ = results("keep")
    assert not np.array_equal(want, keep), "the fade pictures equal the keep pictures: the case cannot tell the modes apart"

    comm = _LocalComm(world)
    res, errors = [None] * world, []

    def run(rank):
        try:
            lo, hi = shard.shard_range(total, rank, world)
            crt = crtlib.CRT(max(hi - lo, 1), outw, outh, crtlib.FMT_BGRA, "ntsc", device=0)
            crt.scanlines, crt.blend, crt.phosphor = scanlines, blend, "fade"
            eng = shard.CrtSequenceEngine(crt, settings(lo, max(hi, lo + 1)) if hi > lo else None, noise)
            rounds = shard.sequence_sharded(eng, comm.view(rank), rank, world, total, 7, 2, 194,
                                            init if rank == 0 else None, blend, torch.device("cuda:0"), (outh, outw, 4))
            crt.synchronize()
            res[rank] = (lo, hi, crt.out.cpu().numpy()[:hi - lo], [crt.get(f)[:hi - lo] for f in ("hsync", "vsync", "rn")], rounds)
            crt.close()
        except Exception as e:                                   # pragma: no cover
            errors.append((rank, repr(e)))
            try:
                comm.barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    if world == 4:
        assert any(hi == lo for lo, hi, *_ in res), "the case was meant to hold a rank with an empty block"
    for lo, hi, out, st, rounds in res:
        assert 1 <= rounds <= world + 1
        np.testing.assert_array_equal(out, want[lo:hi], err_msg="fields %d..%d" % (lo, hi))
        for got, full in zip(st, want_state):
            assert got == full[lo:hi]


def _check_fieldpass(crtlib, name, n, outw, outh, ofmt, knobs, mode, noise, shape=1, overlap=1, iw=640, ih=480, steps=2, seed=60):
    """n independent displays, each with its own random prior picture; one display step per fieldpass() call, `steps` calls"""
    bpp = R.bpp4fmt(ofmt)
    imgs = np.stack([R.synth_image(iw, ih, 4, seed + 7 * k, "random" if k % 2 == 0 else "bars") for k in range(n)])
    priors = [R.lcg_bytes(outw * outh * bpp, 1000 + k).reshape(outh, outw, bpp) for k in range(n)]
    orc = R.Oracle(name)
    ocrts, kcrts = [], []
    for k in range(n):
        for lst in (ocrts, kcrts):
            c = orc.new_crt(outw, outh, ofmt)
            for a, v in knobs.items():
                c.set(a, v)
            c.out[:] = priors[k].reshape(-1)
            lst.append(c)
    g = crtlib.CRT(n, outw, outh, ofmt, name, device=0)
    for a, v in knobs.items():
        setattr(g, a, v)
    g.phosphor = mode
    g.set_shape(shape)
    g.set_overlap(overlap)
    g.out.copy_(_to_dev(np.stack(priors)))
    fields = [k & 1 for k in range(n)]
    frames = [(k >> 1) & 1 for k in range(n)]
    s = crtlib.Settings(_padded(imgs), format=crtlib.FMT_BGRA, field=list(fields), frame=list(frames))
    differs = False
    for step in range(steps):
        g.fieldpass(s, noise)
        g.synchronize()
        gout = g.out.cpu().numpy()
        gst = {f: g.get(f) for f in ("hsync", "vsync", "rn")}
        for k in range(n):
            for c, m in ((ocrts[k], mode), (kcrts[k], "keep")):
                if m != "keep":
                    c.out[:] = display_step_np(c.out, ofmt, m)
                c.settings(np.concatenate([imgs[k], imgs[k][-1:]]), format=R.FMT_BGRA, w=iw, h=ih, as_color=1, field=fields[k], frame=frames[k])
                c.modulate()
                c.demodulate(noise)
            c = ocrts[k]
            differs = differs or not np.array_equal(c.out, kcrts[k].out)
            what = "%s %s shape %d overlap %d step %d display %d" % (name, mode, shape, overlap, step, k)
            for f in ("hsync", "vsync", "rn"):
                assert gst[f][k] == c.get(f), "%s %s" % (what, f)
            np.testing.assert_array_equal(gout[k].reshape(-1), c.out, err_msg=what)
        fields = [f ^ 1 for f in fields]
        if step % 2 == 0:
            frames = [f ^ 1 for f in frames]
        s.field, s.frame = list(fields), list(frames)
    assert differs, "the %s pictures equal the keep-mode pictures: the case cannot tell the modes apart" % mode
    g.close()


FP_CASES = [  # name, n, outw, outh, ofmt, knobs, noise, shape, overlap, iw, ih
    ("ntsc", 5, 640, 480, R.FMT_BGRA, dict(scanlines=1), 24, 1, 1, 640, 480),
    ("ntsc", 5, 640, 480, R.FMT_BGRA, dict(scanlines=1, blend=1), 24, 1, 1, 640, 480),
    ("ntsc", 5, 640, 480, R.FMT_BGRA, dict(scanlines=1), 24, 2, 1, 640, 480),
    ("ntsc", 5, 640, 480, R.FMT_BGRA, dict(scanlines=0, blend=1), 24, 2, 1, 640, 480),
    ("ntsc", 4, 833, 601, R.FMT_RGB, dict(scanlines=1), 12, 1, 1, 640, 480),
    ("ntsc", 4, 833, 601, R.FMT_RGB, dict(scanlines=1, blend=1), 12, 2, 1, 640, 480),
    ("ntsc", 4, 322, 250, R.FMT_ARGB, dict(scanlines=1, blend=1), 12, 1, 1, 320, 240),
    ("ntsc", 512, 96, 480, R.FMT_BGRA, dict(scanlines=1), 24, 1, 2, 64, 48),
    ("ntsc", 512, 98, 240, R.FMT_RGB, dict(scanlines=1, blend=1), 24, 1, 2, 64, 48),
    ("ntscbloom", 4, 640, 480, R.FMT_BGRA, dict(scanlines=1), 24, 1, 1, 640, 480),
    ("ntscbloom", 4, 640, 480, R.FMT_BGRA, dict(scanlines=1, blend=1), 24, 1, 1, 640, 480),
    ("ntsc", 3, 1920, 1080, R.FMT_BGRA, dict(scanlines=1), 24, 1, 1, 1920, 1080),
]


@pytest.mark.parametrize("mode", ["fade", "clear"])
@pytest.mark.parametrize("case", range(len(FP_CASES)))
def test_fieldpass_display_modes(crtlib, case, mode):
    """crthip_fieldpass: every image is its own display; k_phosphor_rows fades (clears) the rows the field does not write, or every
    row before a blending decoder -- both kernel shapes, the overlap chunks, the bloom decoder, the wide-run decoder (1080p)"""
    name, n, outw, outh, ofmt, knobs, noise, shape, overlap, iw, ih = FP_CASES[case]
    _check_fieldpass(crtlib, name, n, outw, outh, ofmt, knobs, mode, noise, shape, overlap, iw, ih)


@pytest.mark.parametrize("shape", [0, 1])
def test_fade_fieldpass_is_graph_capturable(crtlib, shape):
    """a FADE field-pass only enqueues kernels (no workspace of its own): captured into a graph and replayed it gives the bytes of
    the direct calls"""
    import torch
    n, w, h = 6, 640, 480
    imgs = _padded(np.stack([R.synth_image(w, h, 4, 40 + k) for k in range(n)]))
    prior = _to_dev(np.stack([R.lcg_bytes(w * h * 4, 70 + k).reshape(h, w, 4) for k in range(n)]))
    s = crtlib.Settings(imgs, format=crtlib.FMT_BGRA, field=[k & 1 for k in range(n)], frame=0)

    def context():
        g = crtlib.CRT(n, w, h, crtlib.FMT_BGRA, "ntsc", device=0)
        g.scanlines, g.phosphor = 1, "fade"
        g.set_shape(shape)
        g.reserve(n)
        return g
    g = context()
    p = g.params(s, 24)
    assert p.flags & crtlib.F_PHOSPHOR_FADE
    side = torch.cuda.Stream()
    g.use_stream(side)
    g._load_field_state(s)
    torch.cuda.synchronize()
    state0 = g.state.clone()
    g.out.copy_(prior)
    eager = []
    for _ in range(2):
        g.fieldpass(s, 24, params=p)
        g.synchronize()
        eager.append((g.out.clone(), g.state.clone()))
    assert not torch.equal(eager[0][0], eager[1][0])
    for fresh in (False, True):
        c = context() if fresh else g
        c.use_stream(side)
        if fresh:
            c._load_field_state(s)
        c.state.copy_(state0)
        c.out.copy_(prior)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            c.fieldpass(s, 24, params=p)
        for k in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(c.out, eager[k][0]), "fresh=%s replay %d: picture differs from the direct calls" % (fresh, k)
            assert torch.equal(c.state, eager[k][1]), "fresh=%s replay %d: state differs" % (fresh, k)
        del graph
        c.use_stream(None)
        c.close()


@pytest.mark.parametrize("mode", ["fade", "clear"])
def test_stage_level_entry_points_refuse_the_display_modes(crtlib, mode):
    """crthip_modulate / _noise / _sync / _decode: the host owns the buffer there (crt_main.c), so a phosphor flag is CRTHIP_E_ARG"""
    n, w, h = 2, 320, 240
    g = crtlib.CRT(n, w, h, crtlib.FMT_BGRA, "ntsc", device=0)
    s = crtlib.Settings(_padded(np.stack([R.synth_image(w, h, 4, 5 + k) for k in range(n)])), format=crtlib.FMT_BGRA)
    g.modulate(s)                                     # keep: fine
    g.demodulate(0)
    g.synchronize()
    before = g.out.clone()
    g.phosphor = mode
    p = g.params(s, 0)
    L, vp = g.L, C.c_void_p
    assert L.crthip_decode(g.ctx, C.byref(p), n, vp(g.inp.data_ptr()), vp(g.line_table.data_ptr()), vp(g.out.data_ptr()),
                           g.out.stride(0)) == -1
    assert L.crthip_sync(g.ctx, C.byref(p), n, vp(g.inp.data_ptr()), vp(g.state.data_ptr()), vp(g.line_table.data_ptr())) == -1
    assert L.crthip_noise(g.ctx, C.byref(p), n, vp(g.analog.data_ptr()), vp(g.inp.data_ptr()), vp(g.state.data_ptr())) == -1
    assert L.crthip_modulate(g.ctx, C.byref(p), n, vp(s.data.data_ptr()), g._image_stride(s), vp(g.analog.data_ptr()),
                             vp(g.state.data_ptr())) == -1
    with pytest.raises(RuntimeError):
        g.modulate(s)
    g.synchronize()
    assert g.out.equal(before)
    g.close()

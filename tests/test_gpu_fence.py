"""No entry point touches memory outside its buffers: every case of tests/fence_cases.py runs twice on fenced buffers
(tests/fence.py) whose guards, gaps and rows behind the images hold two different random fills.  Each run: (a) payloads equal the
oracle bit for bit, (b) every byte outside the payloads of EVERY buffer handed to the call is unchanged (read-only buffers whole),
(c) both runs leave identical payloads and states.  Alignments the header forbids are refused before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import fence as F
import fence_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ARG = -1                            # CRTHIP_E_ARG
STATE_SPARE = 8                      # state records behind the n the call is told about


@pytest.fixture(scope="module")
def crtlib():
    import os
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(g.PKG, "lib", "libcrthip.so")):
        g.build()
    import crtlib
    crtlib.load_library()
    return crtlib


class Run:
    """one run of one case: the fenced buffers, their prefills, the call"""

    def __init__(self, crtlib, c, seed):
        import torch
        self.c, self.lib, self.seed, self.bufs, self.readonly = c, crtlib, seed, {}, set()
        n = c["n"]
        g = crtlib.CRT(n, c["outw"], c["outh"], c["ofmt"], c["name"], device=0, out=torch.zeros(1, dtype=torch.uint8, device=DEV))
        self.g = g
        g.set_exact(c["exact"])
        g.set_shape(c["shape"])
        g.set_signal_tile(c["tile"])
        g.set_wide_lpw(c["lpw"])
        g.set_signal_layout(c["layout"])
        if c["overlap"]:
            g.set_overlap(c["overlap"])
        for k, v in c["knobs"].items():
            setattr(g, k, v)
        g.phosphor = c["mode"]
        # pictures
        size, stride, base = FC.picture_layout(c)
        pitch = FC.picture_row_bytes(c)
        bpp = R.bpp4fmt(c["ofmt"])
        fo = self.add("out", F.Fenced(n, size, stride, base, pitch, DEV, "d_out"), FC.out_prefill(c))
        g.out = fo.view((c["outh"], c["outw"], bpp))
        assert g.out.stride(0) == stride and g.out.data_ptr() == fo.ptr()
        # images
        payload, istride, ibase, spare = FC.image_layout(c)
        self.imgs = FC.images(c)
        fi = self.add("images", F.Fenced(n, payload, istride, ibase, FC.image_row_bytes(c), DEV, "d_images"), self.imgs, readonly=True)
        rows = c["h"] + (1 if spare else 0)
        if FC.is_nes(c):
            data = fi.view((rows, c["w"]), torch.int16)[:, :c["h"]]
        else:
            data = fi.view((rows, c["w"], R.bpp4fmt(c["ifmt"])))[:, :c["h"]]
        par = [FC.parity(k) for k in range(n)]
        if c["kind"] in ("sequence", "sets"):
            par = [FC.parity(k - lo) for lo, hi in FC.sets_of(c) for k in range(lo, hi)]
        dco = [FC.dot_crawl(c, k) for k in range(n)]
        dot = g.sysid in crtlib.DOT_CRAWL_SYSTEMS
        self.s = crtlib.Settings(data, format=c["ifmt"], field=[p[0] for p in par], frame=[p[1] for p in par],
                                 dot_crawl_offset=dco if dot else 0, spare_row=spare, **dict(dict(as_color=1), **c["skw"]))
        assert g._image_stride(self.s) == istride and data.data_ptr() == fi.ptr()
        # states: n + STATE_SPARE records, the call is told n (the spare ones lie in the back guard's place and are checked with it)
        st = np.zeros((n, crtlib.STATE_INTS), dtype=np.int32)
        st[:, crtlib.ST_RN] = 194
        fs = self.add("state", F.Fenced(n, 4 * crtlib.STATE_INTS, None, 0, 4 * crtlib.STATE_INTS * STATE_SPARE // 2, DEV, "d_state"), st)
        assert fs.guard >= 4 * crtlib.STATE_INTS * STATE_SPARE
        g.state = fs.view((crtlib.STATE_INTS,), torch.int32)
        if c["kind"] == "stage":
            isz = g.input_size
            an = np.zeros((n, g.fstride), dtype=np.int8)
            an[:, :isz] = FC.analog_prefill(c, isz)
            g._analog = self.add("analog", F.Fenced(n, g.fstride, None, 0, g.hres, DEV, "d_analog"), an).view((g.fstride,), torch.int8)
            g._inp = self.add("inp", F.Fenced(n, g.fstride, None, 0, g.hres, DEV, "d_inp"), R.lcg_bytes(n * g.fstride, 8080)).view((g.fstride,), torch.int8)
            g._lines = self.add("lines", F.Fenced(n, g.lines * 4 * crtlib.LINE_INTS, None, 0, 0, DEV, "d_lines"),
                                   R.lcg_bytes(n * g.lines * 4 * crtlib.LINE_INTS, 8181)) \
                .view((g.lines, crtlib.LINE_INTS), torch.int32)
        if c["kind"] == "fieldpass" and n <= 8:
            # crthip_fieldpass_signal: the fused path's own signal, repacked into a fenced d_inp_flat (not for the 512 fields of the
            # chunk case: 120 MB of random fill per run)
            self.add("signal", F.Fenced(n, g.fstride, None, 0, g.hres, DEV, "d_inp_flat"), R.lcg_bytes(n * g.fstride, 8282))
        if g.vhs_hist is not None:
            fh = self.add("hist", F.Fenced(n, 128, None, 0, 0, DEV, "d_hist"), np.zeros((n, 128), dtype=np.uint8))
            g.vhs_hist = fh.view((32,), torch.int32)
            g._check(g.L.crthip_vhs_bind_history(g.ctx, C.c_void_p(fh.ptr())), "crthip_vhs_bind_history")
            seeds = [FC.VHS_SEEDS[k % 5] for k in range(n)]
            if c["kind"] == "sets":
                seeds = [1] * n
                for s_, (lo, hi) in enumerate(FC.sets_of(c)):
                    seeds[lo] = FC.VHS_SEEDS[s_ % 5]
            g.srand(seeds)
            self.pre["hist"] = fh.host()
        self.init = None
        init = FC.init_pictures(c)
        if init is not None:
            loose = c["init"] == "loose"
            fx = self.add("out_init", F.Fenced(init.shape[0], size, size + (pitch + 4 * 13 if loose else 0), base, pitch, DEV, "d_out_init"),
                          init, readonly=True)
            v = fx.view((c["outh"], c["outw"], bpp))
            self.init = v if (c["kind"] == "sets" and init.shape[0] > 1) else v[0]
            self.init_stride = fx.stride if init.shape[0] > 1 else 0
        self.params = None
        if c["triples"]:
            fk = self.add("knob_recs", F.Fenced(n, 4 * crtlib.KNOB_REC_INTS, None, 0, 0, DEV, "d_recs"),
                          np.zeros((n, 4 * crtlib.KNOB_REC_INTS), dtype=np.uint8), readonly=True)
            g.knob_recs = fk.view((crtlib.KNOB_REC_INTS,), torch.int32)
            self.params = g.params(self.s, 0)
            g._load_field_state(self.s)
            g.upload_knobs(np.array(c["triples"], dtype=np.int32), self.params)
            self.pre["knob_recs"] = fk.host()

    def add(self, key, fenced, contents, readonly=False):
        self.pre = getattr(self, "pre", {})
        self.bufs[key] = fenced
        self.pre[key] = fenced.prefill(self.seed + 101 * len(self.bufs), contents)
        if readonly:
            self.readonly.add(key)
        return fenced

    def call(self):
        c, g, s = self.c, self.g, self.s
        if c["kind"] == "stage":
            g.modulate(s)
            g.demodulate(c["noise"])
        elif c["kind"] == "fieldpass":
            if c["triples"]:
                g.fieldpass_knobs(s, None, params=self.params)
            else:
                g.fieldpass(s, c["noise"])
            self.fstage = g.float_stages_used()
            if "signal" in self.bufs:
                g._check(g.L.crthip_fieldpass_signal(g.ctx, c["n"], C.c_void_p(self.bufs["signal"].ptr()), None), "crthip_fieldpass_signal")
        elif c["kind"] == "stills":
            g.stills(s, c["noise"], schedule=c["sched"])
        elif c["kind"] == "sequence":
            if c["triples"]:
                g.sequence_knobs(s, None, out_init=self.init, params=self.params)
            else:
                g.sequence(s, c["noise"], out_init=self.init)
        else:
            first, n_sets, ip, _ = g._sets_args(c["set_first"], None)
            p = g.params(s, c["noise"], self.lib.F_VHS_SET_STREAMS if c["vhs_streams"] else 0)
            g._load_field_state(s)
            passes = C.c_int(0)
            rc = g.L.crthip_sequence_sets(g.ctx, C.byref(p), n_sets, (C.c_int * (n_sets + 1))(*first), C.c_void_p(s.data.data_ptr()),
                                          g._image_stride(s), C.c_void_p(g.out.data_ptr()), g.out.stride(0),
                                          C.c_void_p(self.init.data_ptr()) if self.init is not None else None,
                                          self.init_stride if self.init is not None else 0, C.c_void_p(g.state.data_ptr()), C.byref(passes))
            g._check(rc, "crthip_sequence_sets")
        g.synchronize()

    def check(self):
        """(a) + (b); returns the payloads for (c)"""
        c, g = self.c, self.g
        want = FC.expected(c)
        now = {k: f.host() for k, f in self.bufs.items()}
        for k, f in self.bufs.items():                            # (b) first: a stray store explains a wrong picture
            if k in self.readonly:
                f.assert_unchanged(self.pre[k], now[k])
            else:
                f.assert_fence_intact(self.pre[k], now[k])
        got = {k: self.bufs[k].payloads(now[k]) for k in self.bufs if k not in self.readonly}
        what = "%s seed %d" % (c["id"], self.seed)
        isz = want["input_size"]
        if c["kind"] == "stage":
            np.testing.assert_array_equal(got["analog"][:, :isz].view(np.int8), np.stack(want["analog"]), err_msg=what + " analog")
            np.testing.assert_array_equal(got["inp"][:, :isz].view(np.int8), np.stack(want["inp"]), err_msg=what + " inp")
            # the line table as tests/test_gpu_parity.py compares it: valid lines, then (pos, wave0, wave1, beg, hsync, dx, scanl)
            glines = got["lines"].view(np.int32).reshape(c["n"], -1, self.lib.LINE_INTS)
            for k, tr in enumerate(want["trace"]):
                valid = tr[:, 0] == 1
                np.testing.assert_array_equal((glines[k][:, 4] & 0xffff) > 0, valid, err_msg="%s field %d valid lines" % (what, k))
                np.testing.assert_array_equal(glines[k][valid][:, [0, 1, 2, 3, 5, 6, 7]], tr[valid][:, [1, 2, 3, 4, 6, 7, 8]],
                                              err_msg="%s field %d line table" % (what, k))
        if "signal" in got:
            np.testing.assert_array_equal(got["signal"][:, :isz].view(np.int8), np.stack(want["inp"]), err_msg=what + " crthip_fieldpass_signal")
            if c["id"].startswith("dec-wide"):
                assert self.fstage == 0, "%s: the wide-run decoder was not taken (the lane decoder's float stages ran)" % what
            if c["id"] == "dec-lane-1650x120-blend":
                assert self.fstage == 1, "%s: float_stages_used does not tell the lane decoder from the wide-run one any more" % what
        st = got["state"].view(np.int32).reshape(c["n"], -1)
        cols = [self.lib.ST_HSYNC, self.lib.ST_VSYNC] + ([] if c["name"] == "vhs" else [self.lib.ST_RN])
        np.testing.assert_array_equal(st[:, cols].astype(np.int64), want["state"][:, :len(cols)], err_msg=what + " hsync, vsync, rn")
        if want["ccf"]:
            orc_ccf = np.stack(want["ccf"])
            gccf = st[:, self.lib.ST_CCF:self.lib.ST_CCF + 25].reshape(c["n"], 5, 5)[:, :orc_ccf.shape[1], :orc_ccf.shape[2]]
            np.testing.assert_array_equal(gccf, orc_ccf, err_msg=what + " ccf")
        bad = np.flatnonzero((got["out"] != want["out"]).any(axis=1))
        assert bad.size == 0, "%s: pictures %r differ from the oracle, first byte %d of picture %d" % (
            what, bad.tolist(), int(np.flatnonzero(got["out"][bad[0]] != want["out"][bad[0]])[0]), int(bad[0]))
        return got

    def close(self):
        self.g.close()


@pytest.mark.parametrize("id", FC.CASE_IDS)
def test_fenced_buffers(crtlib, id):
    c = FC.case(id)
    got = []
    for seed in FC.FILL_SEEDS:
        r = Run(crtlib, c, seed)
        try:
            r.call()
            got.append(r.check())
        finally:
            r.close()
    assert got[0].keys() == got[1].keys()
    for k in got[0]:                                              # (c)
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg="%s: %s depends on what lies outside the buffers" % (id, k))


# ---- what the header forbids is refused before anything is launched -------------------------------------------------------------
def _refusal_setup(crtlib, name, ifmt, ofmt):
    c = FC.C("refusal", name=name, w=17 if name != "nes" else 256, h=7 if name != "nes" else 240, ifmt=ifmt, ofmt=ofmt, n=2,
             img=(8, 4 if name != "nes" else 2, False), out=(8, 4), init="loose", kind="sequence")
    return Run(crtlib, c, 31337)


def _args(r, crtlib, noise=12):
    g, s = r.g, r.s
    p = g.params(s, noise)
    g._load_field_state(s)
    return dict(p=p, img=s.data.data_ptr(), istride=g._image_stride(s), out=g.out.data_ptr(), ostride=g.out.stride(0),
                st=g.state.data_ptr(), init=r.init.data_ptr())


def _refused_and_untouched(r, crtlib, rc, what, name=None):
    """CRTHIP_E_ARG, an error string that names the argument (`name`: default the last word of `what` before " + "), and every buffer
    of the run byte-identical with its snapshot"""
    r.g.synchronize()
    assert rc == E_ARG, "%s: returned %d, not CRTHIP_E_ARG" % (what, rc)
    name = name or what.split(" + ")[0].split()[-1]
    msg = r.g.L.crthip_error_string(r.g.ctx).decode()
    assert name in msg and "alignment" in msg, "%s: the error string %r does not name %s" % (what, msg, name)
    for k, f in r.bufs.items():
        f.assert_unchanged(r.snap[k])


BAD4 = [1, 2, 3]


@pytest.mark.parametrize("entry,which", [(e, w) for e in ("fieldpass", "sequence", "sequence_sets", "stills")
                                         for w in ("d_out", "out_stride", "d_images", "image_stride", "d_state", "d_out_init")
                                         if w != "d_out_init" or e.startswith("sequence")])
def test_misaligned_4_byte_pixels_and_records_are_refused(crtlib, entry, which):
    r = _refusal_setup(crtlib, "ntsc", R.FMT_BGRA, R.FMT_BGRA)
    try:
        a = _args(r, crtlib)
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        L, vp = r.g.L, C.c_void_p
        for off in BAD4:
            b = dict(a)
            key = {"d_out": "out", "out_stride": "ostride", "d_images": "img", "image_stride": "istride", "d_state": "st", "d_out_init": "init"}[which]
            b[key] = a[key] + off
            if entry == "fieldpass":
                rc = L.crthip_fieldpass(r.g.ctx, C.byref(b["p"]), 2, vp(b["img"]), b["istride"], vp(b["out"]), b["ostride"], vp(b["st"]))
            elif entry == "sequence":
                rc = L.crthip_sequence(r.g.ctx, C.byref(b["p"]), 2, vp(b["img"]), b["istride"], vp(b["out"]), b["ostride"], vp(b["init"]), vp(b["st"]), None)
            elif entry == "sequence_sets":
                rc = L.crthip_sequence_sets(r.g.ctx, C.byref(b["p"]), 1, (C.c_int * 2)(0, 2), vp(b["img"]), b["istride"], vp(b["out"]), b["ostride"],
                                            vp(b["init"]), 0, vp(b["st"]), None)
            else:
                sched = (crtlib.Pass * 2)()
                rc = L.crthip_stills(r.g.ctx, C.byref(b["p"]), 2, vp(b["img"]), b["istride"], vp(b["out"]), b["ostride"], vp(b["st"]), 2, sched)
            _refused_and_untouched(r, crtlib, rc, "%s %s + %d" % (entry, which, off))
        if entry == "sequence_sets" and which == "d_out_init":
            rc = L.crthip_sequence_sets(r.g.ctx, C.byref(a["p"]), 1, (C.c_int * 2)(0, 2), vp(a["img"]), a["istride"], vp(a["out"]), a["ostride"],
                                        vp(a["init"]), r.bufs["out_init"].stride + 2, vp(a["st"]), None)
            _refused_and_untouched(r, crtlib, rc, "sequence_sets out_init_stride + 2")
    finally:
        r.close()


def test_misaligned_stage_level_arguments_are_refused(crtlib):
    c = FC.C("refusal-stage", kind="stage", w=17, h=7, n=2, img=(8, 4, False), out=(8, 4))
    r = Run(crtlib, c, 4711)
    try:
        g, s, L, vp = r.g, r.s, r.g.L, C.c_void_p
        p = g.params(s, 12)
        g._load_field_state(s)
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        img, ist, an, inp, st, ln, out, ost = (s.data.data_ptr(), g._image_stride(s), g.analog.data_ptr(), g.inp.data_ptr(), g.state.data_ptr(),
                                               g.line_table.data_ptr(), g.out.data_ptr(), g.out.stride(0))
        for off in BAD4:
            for what, call in [
                ("modulate d_images", lambda: L.crthip_modulate(g.ctx, C.byref(p), 2, vp(img + off), ist, vp(an), vp(st))),
                ("modulate image_stride", lambda: L.crthip_modulate(g.ctx, C.byref(p), 2, vp(img), ist + off, vp(an), vp(st))),
                ("modulate d_analog", lambda: L.crthip_modulate(g.ctx, C.byref(p), 2, vp(img), ist, vp(an + off), vp(st))),
                ("modulate d_state", lambda: L.crthip_modulate(g.ctx, C.byref(p), 2, vp(img), ist, vp(an), vp(st + off))),
                ("noise d_inp", lambda: L.crthip_noise(g.ctx, C.byref(p), 2, vp(an), vp(inp + off), vp(st))),
                ("sync d_lines", lambda: L.crthip_sync(g.ctx, C.byref(p), 2, vp(inp), vp(st), vp(ln + off))),
                ("decode d_out", lambda: L.crthip_decode(g.ctx, C.byref(p), 2, vp(inp), vp(ln), vp(out + off), ost)),
                ("decode out_stride", lambda: L.crthip_decode(g.ctx, C.byref(p), 2, vp(inp), vp(ln), vp(out), ost + off)),
                ("decode d_lines", lambda: L.crthip_decode(g.ctx, C.byref(p), 2, vp(inp), vp(ln + off), vp(out), ost)),
            ]:
                _refused_and_untouched(r, crtlib, call(), "%s + %d" % (what, off))
    finally:
        r.close()


def test_misaligned_knob_records_and_ppu_pixels_are_refused(crtlib):
    c = FC.C("refusal-knobs", w=17, h=7, n=2, img=(8, 4, False), out=(8, 4), triples=[(12, 0, 10), (3, 5, 9)])
    r = Run(crtlib, c, 99)
    try:
        g, s, L, vp = r.g, r.s, r.g.L, C.c_void_p
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        for off in BAD4:
            rc = L.crthip_fieldpass_knobs(g.ctx, C.byref(r.params), 2, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()), g.out.stride(0),
                                          vp(g.state.data_ptr()), vp(g.knob_recs.data_ptr() + off), C.byref(g._knob_env))
            _refused_and_untouched(r, crtlib, rc, "fieldpass_knobs d_recs + %d" % off)
    finally:
        r.close()
    r = _refusal_setup(crtlib, "nes", R.FMT_BGRA, R.FMT_BGRA)
    try:
        a = _args(r, crtlib)
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        L, vp = r.g.L, C.c_void_p
        for di, ds in ((1, 0), (0, 1), (3, 0), (0, 3)):
            rc = L.crthip_fieldpass(r.g.ctx, C.byref(a["p"]), 2, vp(a["img"] + di), a["istride"] + ds, vp(a["out"]), a["ostride"], vp(a["st"]))
            _refused_and_untouched(r, crtlib, rc, "nes fieldpass d_images + %d, image_stride + %d" % (di, ds))
    finally:
        r.close()


def test_3_byte_pixels_take_any_base_and_stride_but_records_do_not(crtlib):
    """RGB on both sides: bytewise kernels, every base and stride is in the contract (the cases above run them); the state records
    still need their 4 bytes"""
    r = _refusal_setup(crtlib, "ntsc", R.FMT_RGB, R.FMT_RGB)
    try:
        a = _args(r, crtlib)
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        L, vp = r.g.L, C.c_void_p
        rc = L.crthip_fieldpass(r.g.ctx, C.byref(a["p"]), 2, vp(a["img"] + 1), a["istride"], vp(a["out"] + 1), a["ostride"], vp(a["st"] + 2))
        _refused_and_untouched(r, crtlib, rc, "rgb fieldpass d_state + 2")
    finally:
        r.close()


def test_misaligned_stage_level_inputs_and_states_are_refused(crtlib):
    """the read-only sides of the stage-level calls, and the NES's PPU pixels on crthip_modulate"""
    c = FC.C("refusal-stage-inputs", kind="stage", w=17, h=7, n=2, img=(8, 4, False), out=(8, 4))
    r = Run(crtlib, c, 4712)
    try:
        g, s, L, vp = r.g, r.s, r.g.L, C.c_void_p
        p = g.params(s, 12)
        g._load_field_state(s)
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        an, inp, st, ln, out, ost = (g.analog.data_ptr(), g.inp.data_ptr(), g.state.data_ptr(), g.line_table.data_ptr(), g.out.data_ptr(), g.out.stride(0))
        for off in BAD4:
            for what, call in [
                ("noise d_analog", lambda: L.crthip_noise(g.ctx, C.byref(p), 2, vp(an + off), vp(inp), vp(st))),
                ("noise d_state", lambda: L.crthip_noise(g.ctx, C.byref(p), 2, vp(an), vp(inp), vp(st + off))),
                ("sync d_inp", lambda: L.crthip_sync(g.ctx, C.byref(p), 2, vp(inp + off), vp(st), vp(ln))),
                ("sync d_state", lambda: L.crthip_sync(g.ctx, C.byref(p), 2, vp(inp), vp(st + off), vp(ln))),
                ("decode d_inp", lambda: L.crthip_decode(g.ctx, C.byref(p), 2, vp(inp + off), vp(ln), vp(out), ost)),
            ]:
                _refused_and_untouched(r, crtlib, call(), "%s + %d" % (what, off))
    finally:
        r.close()
    c = FC.C("refusal-stage-nes", kind="stage", name="nes", w=256, h=240, n=2, img=(2, 2, False), out=(8, 4))
    r = Run(crtlib, c, 4713)
    try:
        g, s, L, vp = r.g, r.s, r.g.L, C.c_void_p
        p = g.params(s, 12)
        g._load_field_state(s)
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        for di, ds in ((1, 0), (0, 1), (3, 0), (0, 3)):
            rc = L.crthip_modulate(g.ctx, C.byref(p), 2, vp(s.data.data_ptr() + di), g._image_stride(s) + ds, vp(g.analog.data_ptr()), vp(g.state.data_ptr()))
            _refused_and_untouched(r, crtlib, rc, "nes modulate d_images + %d, image_stride + %d" % (di, ds))
    finally:
        r.close()


def test_misaligned_signal_copy_is_refused(crtlib):
    """crthip_fieldpass_signal after a field-pass that went through: d_inp_flat off its 4 bytes"""
    r = Run(crtlib, FC.C("refusal-signal", w=17, h=7, n=2, img=(8, 4, False), out=(8, 4)), 4714)
    try:
        r.call()
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        for off in BAD4:
            rc = r.g.L.crthip_fieldpass_signal(r.g.ctx, 2, C.c_void_p(r.bufs["signal"].ptr() + off), None)
            _refused_and_untouched(r, crtlib, rc, "fieldpass_signal d_inp_flat + %d" % off)
    finally:
        r.close()


def test_misaligned_vhs_histories_and_chain_states_are_refused(crtlib):
    r = Run(crtlib, FC.C("refusal-vhs", name="vhs", w=17, h=7, n=2, noise=12, img=(8, 4, False), out=(8, 4), shape=0), 4715)
    try:
        g, L, vp = r.g, r.g.L, C.c_void_p
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        for off in BAD4:
            _refused_and_untouched(r, crtlib, L.crthip_vhs_bind_history(g.ctx, vp(r.bufs["hist"].ptr() + off)), "vhs_bind_history d_hist + %d" % off)
            _refused_and_untouched(r, crtlib, L.crthip_vhs_chain(g.ctx, 2, vp(g.state.data_ptr() + off), 0), "vhs_chain d_state + %d" % off)
        # the refused binds left the binding alone: the field-pass still runs on the fenced histories
        r.call()
        for k, f in r.bufs.items():
            f.assert_fence_intact(r.pre[k])
    finally:
        r.close()


def test_misaligned_knob_records_of_the_sequence_calls_are_refused(crtlib):
    c = FC.C("refusal-seq-knobs", kind="sequence", w=17, h=7, n=2, img=(8, 4, False), out=(8, 4), init="loose", triples=[(12, 0, 10), (3, 5, 9)])
    r = Run(crtlib, c, 4716)
    try:
        g, s, L, vp = r.g, r.s, r.g.L, C.c_void_p
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        img, ist, out, ost, init, st, recs, env = (s.data.data_ptr(), g._image_stride(s), g.out.data_ptr(), g.out.stride(0), r.init.data_ptr(),
                                                   g.state.data_ptr(), g.knob_recs.data_ptr(), C.byref(g._knob_env))
        for off in BAD4:
            for what, call in [
                ("sequence_knobs d_recs", lambda: L.crthip_sequence_knobs(g.ctx, C.byref(r.params), 2, vp(img), ist, vp(out), ost, vp(init), vp(st),
                                                                          vp(recs + off), env, None)),
                ("sequence_sets_knobs d_recs", lambda: L.crthip_sequence_sets_knobs(g.ctx, C.byref(r.params), 1, (C.c_int * 2)(0, 2), vp(img), ist, vp(out), ost,
                                                                                    vp(init), 0, vp(st), vp(recs + off), env, None)),
                ("seq_bind_knobs d_recs", lambda: L.crthip_seq_bind_knobs(g.ctx, vp(recs + off), env)),
            ]:
                _refused_and_untouched(r, crtlib, call(), "%s + %d" % (what, off))
    finally:
        r.close()


def test_misaligned_arguments_of_the_sequence_phases_are_refused(crtlib):
    """crthip_seq_encode / _sync / _decode / _weave, each for the device pointers it takes (the workspace reserved first, so that
    nothing but the alignment stands in the way)"""
    r = _refusal_setup(crtlib, "ntsc", R.FMT_BGRA, R.FMT_BGRA)
    try:
        a = _args(r, crtlib)
        g, L, vp, p = r.g, r.g.L, C.c_void_p, a["p"]
        g.reserve(2)
        r.snap = {k: f.host() for k, f in r.bufs.items()}
        ho, vo, ps = C.c_int(0), C.c_int(0), C.c_int(0)
        for off in BAD4:
            for what, call in [
                ("seq_encode d_images", lambda: L.crthip_seq_encode(g.ctx, C.byref(p), 2, 0, 194, vp(a["img"] + off), a["istride"], vp(a["st"]))),
                ("seq_encode image_stride", lambda: L.crthip_seq_encode(g.ctx, C.byref(p), 2, 0, 194, vp(a["img"]), a["istride"] + off, vp(a["st"]))),
                ("seq_encode d_state", lambda: L.crthip_seq_encode(g.ctx, C.byref(p), 2, 0, 194, vp(a["img"]), a["istride"], vp(a["st"] + off))),
                ("seq_sync d_state", lambda: L.crthip_seq_sync(g.ctx, C.byref(p), 2, vp(a["st"] + off), 0, 0, C.byref(ho), C.byref(vo), C.byref(ps))),
                ("seq_decode d_out", lambda: L.crthip_seq_decode(g.ctx, C.byref(p), 2, vp(a["out"] + off), a["ostride"], vp(a["st"]))),
                ("seq_decode out_stride", lambda: L.crthip_seq_decode(g.ctx, C.byref(p), 2, vp(a["out"]), a["ostride"] + off, vp(a["st"]))),
                ("seq_decode d_state", lambda: L.crthip_seq_decode(g.ctx, C.byref(p), 2, vp(a["out"]), a["ostride"], vp(a["st"] + off))),
                ("seq_weave d_out", lambda: L.crthip_seq_weave(g.ctx, C.byref(p), 2, vp(a["out"] + off), a["ostride"], vp(a["init"]), 0)),
                ("seq_weave out_stride", lambda: L.crthip_seq_weave(g.ctx, C.byref(p), 2, vp(a["out"]), a["ostride"] + off, vp(a["init"]), 0)),
                ("seq_weave d_out_init", lambda: L.crthip_seq_weave(g.ctx, C.byref(p), 2, vp(a["out"]), a["ostride"], vp(a["init"] + off), 0)),
            ]:
                _refused_and_untouched(r, crtlib, call(), "%s + %d" % (what, off))
    finally:
        r.close()

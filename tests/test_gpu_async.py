"""Call chains enqueued without host synchronisation.  Every other GPU test waits on the host between library calls, so the suite
proves that a result does not depend on which calls came before -- never that it does not depend on whether the host WAITED for them.
bench.py, a video player and a kept graph between eager calls all enqueue call after call; what orders their work is the library's
own plumbing: the internal stream and its events, tables rewritten in place, one workspace for every entry point, record buffers the
caller rewrites between calls ("Asynchronous call chains").

The chains of tests/async_cases.py run twice on fresh contexts:
  waited   a host synchronisation after every call, as the rest of the suite does (three times: the median host time of enqueuing the
           chain sizes the plug);
  chained  no host synchronisation from the first call to the last.  Everything the chain needs is on the device before it starts;
           calls go through params= / the C ABI, so nothing is copied from pageable host memory; per-step records are put in place
           by device-to-device copies on the context's stream; after every call the pictures and states are copied into preallocated
           snapshots on the same stream (which also tests that the library joined its internal stream before the caller's next
           operation).  The first thing on the stream is THE PLUG: a device-side delay (torch.cuda._sleep, calibrated once per
           module) of 3 x the measured enqueue time, at most 0.5 s, with an event behind it.  THE NO-WAIT CONDITION: after every call
           that the chain declares asynchronous, and after the last snapshot, that event has not completed -- the host provably
           never waited for the GPU and every call was enqueued while all earlier work was pending.  A plug that has ended FAILS the
           test; it never passes on a chain that was in fact serialised.  A call that waits by design (workspace growth, sequence mode's sync loop) is declared
           in the table with its source line; behind it the assertion resumes with a fresh plug.

Compared: every field of every snapshot of the chained run with the oracle at tolerance 0 -- picture, hsync, vsync, rn, for the VHS
chain the generator (next rand()), for the layout chain the signal --, and the chained run byte for byte with the waited one (all
36 state words, whole histories).  The second comparison is diagnostic: it tells an ordering fault from a plain one."""
import ctypes as C
import time

import numpy as np
import pytest

import async_cases as AC
import crtref as R

pytestmark = pytest.mark.gpu
PLUG_FACTOR, PLUG_CAP_S = 3.0, 0.5


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


@pytest.fixture(scope="module")
def cycles_per_s(crtlib):
    """torch.cuda._sleep counts device clock ticks: how many make a second, from two timed events"""
    import torch
    assert hasattr(torch.cuda, "_sleep"), "the plug needs torch.cuda._sleep"
    torch.cuda._sleep(1000000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ticks = 20000000
    a.record()
    torch.cuda._sleep(ticks)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.5, "torch.cuda._sleep(%d) took %.3f ms: no usable delay" % (ticks, ms)
    return ticks / (ms * 1e-3)


_IMAGES = {}


def _device_images(ch):
    """[N, h + 1, w(, 4)]: field k shows its class's image, followed by a readable row (crt_ntsc.c:263); shared by every run"""
    import torch
    key = AC.is_nes(ch)
    if key not in _IMAGES:
        img = AC.images(ch)
        img = img.astype(np.int16) if key else img
        per_cls = np.stack([np.concatenate([img[AC.class_image(c)], img[AC.class_image(c)][-1:]], axis=0) for c in range(AC.NCLS)])
        dev = torch.from_numpy(per_cls).to("cuda:0")
        _IMAGES[key] = dev[torch.arange(AC.N, device="cuda:0") % AC.NCLS].contiguous()
    return _IMAGES[key]


class _Run:
    """one run of a chain on fresh contexts"""

    def __init__(self, crtlib, ch, overlap, kind):
        import torch
        self.crtlib, self.ch, self.torch = crtlib, ch, torch
        self.stream = torch.cuda.Stream() if kind == "own" else torch.cuda.current_stream()
        steps, n = ch["steps"], AC.N
        full = _device_images(ch)
        self.data = full[:, :full.shape[1] - 1]
        par = [AC.class_parity(AC.class_of(k)) for k in range(n)]
        self.gs = []
        for _ in range(ch["contexts"]):
            g = crtlib.CRT(n, AC.OUTW, AC.OUTH, crtlib.FMT_BGRA, ch["name"], device=0)
            g.set_shape(ch["shape"])
            g.set_overlap(overlap)
            g.reserve(ch["reserve"])
            g._load_field_state(self._settings({}, par))
            if any(st["call"] == "stages" for st in steps):
                g.analog, g.inp, g.line_table            # (the stage-level buffers: allocated before the chain)
            if any(st["call"] == "stills" for st in steps):
                g.stills_reserve(len(AC.STILLS_SCHED))
            if g.vhs_hist is not None:
                g.srand([AC.VHS_SEEDS[AC.class_image(AC.class_of(k))] for k in range(n)])
            g.knob_recs = torch.zeros((n, crtlib.KNOB_REC_INTS), dtype=torch.int32, device="cuda:0")
            g.level_recs = torch.zeros((n, crtlib.LEVEL_REC_INTS), dtype=torch.int32, device="cuda:0")
            g.hue_recs = torch.zeros((n, crtlib.HUE_REC_INTS), dtype=torch.int32, device="cuda:0")
            self.gs.append(g)
        # per call: settings, blob and records -- made on the host and uploaded BEFORE the chain
        self.calls = [self._prepare(st, par) for st in steps]
        # the (field, frame, aux) columns of the state: the classes' for every call but the sequence calls, whose fields are
        # consecutive fields of their sets; put in place on-stream before every call (stills and sequence mode leave their own)
        self.par_cls = self.gs[0].state[:, :3].clone()
        self.par_seq = {}
        for i, st in enumerate(steps):
            if st["call"] in ("sequence", "sequence_sets"):
                cols = self.par_cls.clone()
                for lo, hi in AC.seq_sets(st):
                    for k in range(lo, hi):
                        cols[k, 0], cols[k, 1] = AC.seq_parity(k - lo)
                self.par_seq[i] = cols
        self.seq_init = torch.from_numpy(AC.seq_init().reshape(AC.OUTH, AC.OUTW, 4)).to("cuda:0") if AC.has_seq(ch) else None
        ns = len(steps)
        self.snap_out = torch.zeros((ns, n, AC.OUTH, AC.OUTW, 4), dtype=torch.uint8, device="cuda:0")
        self.snap_state = torch.zeros((ns, n, crtlib.STATE_INTS), dtype=torch.int32, device="cuda:0")
        self.snap_hist = torch.zeros((ns, n, 32), dtype=torch.int32, device="cuda:0") if AC.is_vhs(ch) else None
        self.snap_sig = {i: torch.zeros((n, self.gs[0].fstride), dtype=torch.int8, device="cuda:0") for i, st in enumerate(steps) if st["signal"] is not None}
        self.padded = {}
        self.state0 = self.gs[0].state.clone()
        self.graph = None
        torch.cuda.synchronize()
        if ch["capture"] is not None:
            g = self.gs[0]
            s, p, _ = self._prepare(ch["capture"], par)
            cap = self.stream if kind == "own" else torch.cuda.Stream()
            g.use_stream(cap)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=cap):
                self._fieldpass(g, s, p, n)
            self.graph_settings = s                    # (the graph reads s.data: kept alive, never written)
            torch.cuda.synchronize()
        for g in self.gs:
            g.use_stream(self.stream)
        torch.cuda.synchronize()

    def _settings(self, sk, par):
        crtlib = self.crtlib
        geo = dict(hue=sk.get("hue", 0), xoffset=sk.get("xoffset", 0), yoffset=sk.get("yoffset", 0))
        if AC.is_nes(self.ch):
            return crtlib.Settings(self.data, dot_crawl_offset=[p[2] for p in par], border_color=sk.get("border_color", 0), **geo)
        return crtlib.Settings(self.data, format=crtlib.FMT_BGRA, as_color=1, field=[p[0] for p in par], frame=[p[1] for p in par], **geo)

    def _prepare(self, st, par):
        """(settings, blob, records) of a call.  records: None, or the device copies of the call's knob / level / hue records with
        their host-side bounds"""
        crtlib, torch = self.crtlib, self.torch
        if st["call"] == "replay":
            return None, None, None
        sk, kn, noise = AC.step_params(self.ch, st)
        g = self.gs[st["ctx"]]
        for name, v in kn.items():
            setattr(g, name, v)
        s = self._settings(sk, par)                    # (a fresh one per call: the NES's CRTHIP_F_NES_SETUP in every blob)
        if st["call"] == "sizes":
            s.spare_row, s.data = True, None
            p = g.sizes_params(s, noise)
            buf, sizes = AC.sizes_layout(self.ch)
            g.upload_sizes((torch.from_numpy(buf).to("cuda:0"), sizes), p)
            return s, p, None
        if st["call"] != "knobs":
            return s, g.params(s, noise), None
        p = g.params(s, 0)
        rows = AC.knob_rows(st)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")
        if rows.shape[1] == 8:
            recs, levs, hues, env, lenv, henv = crtlib.knobs_prepare8(p, rows)
            return s, p, dict(recs=dev(recs), env=env, levs=dev(levs), lenv=lenv, hues=dev(hues), henv=henv)
        recs, env = crtlib.knobs_prepare(p, rows)
        return s, p, dict(recs=dev(recs), env=env, levs=None)

    def _fieldpass(self, g, s, p, m):
        vp = C.c_void_p
        g._check(g.L.crthip_fieldpass(g.ctx, C.byref(p), m, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()), g.out.stride(0),
                                      vp(g.state.data_ptr())), "crthip_fieldpass")

    def _call(self, i):
        st = self.ch["steps"][i]
        g = self.gs[st["ctx"]]
        s, p, r = self.calls[i]
        vp = C.c_void_p
        m = AC.fields_of(st)
        if st["call"] != "replay":                     # (a graph reads the columns as they are: the classes')
            g.state[:, :3].copy_(self.par_seq.get(i, self.par_cls))
        if st["call"] == "replay":
            self.graph.replay()
        elif st["call"] == "fieldpass":
            self._fieldpass(g, s, p, m)
        elif st["call"] == "stages":
            L, b = g.L, C.byref(p)
            an, inp, ln, state = (vp(t.data_ptr()) for t in (g.analog, g.inp, g.line_table, g.state))
            g._check(L.crthip_modulate(g.ctx, b, m, vp(s.data.data_ptr()), g._image_stride(s), an, state), "crthip_modulate")
            g._check(L.crthip_noise(g.ctx, b, m, an, inp, state), "crthip_noise")
            g._check(L.crthip_sync(g.ctx, b, m, inp, state, ln), "crthip_sync")
            g._check(L.crthip_decode(g.ctx, b, m, inp, ln, vp(g.out.data_ptr()), g.out.stride(0)), "crthip_decode")
        elif st["call"] == "stills":
            buf = g._stills_passes(True, 0, 4, AC.STILLS_SCHED)
            g._check(g.L.crthip_stills(g.ctx, C.byref(p), m, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()), g.out.stride(0),
                                       vp(g.state.data_ptr()), len(buf), buf), "crthip_stills")
        elif st["call"] == "sizes":
            g._check(g.L.crthip_fieldpass_sizes(g.ctx, C.byref(p), m, vp(g._size_buf.data_ptr()), vp(g.out.data_ptr()), g.out.stride(0),
                                                vp(g.state.data_ptr()), vp(g.size_recs.data_ptr()), C.byref(g._size_env)), "crthip_fieldpass_sizes")
        elif st["call"] == "sequence":
            passes = C.c_int(0)
            g._check(g.L.crthip_sequence(g.ctx, C.byref(p), m, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()), g.out.stride(0),
                                         vp(self.seq_init.data_ptr()), vp(g.state.data_ptr()), C.byref(passes)), "crthip_sequence")
        elif st["call"] == "sequence_sets":
            passes, first = C.c_int(0), AC.SETS_FIRST
            g._check(g.L.crthip_sequence_sets(g.ctx, C.byref(p), len(first) - 1, (C.c_int * len(first))(*first), vp(s.data.data_ptr()),
                                              g._image_stride(s), vp(g.out.data_ptr()), g.out.stride(0), vp(self.seq_init.data_ptr()), 0,
                                              vp(g.state.data_ptr()), C.byref(passes)), "crthip_sequence_sets")
        else:
            # the caller's record buffers rewritten on-stream behind the previous call, the binds changed on the host
            g.knob_recs.copy_(r["recs"])
            g._knob_env = r["env"]
            if r["levs"] is not None:
                g.level_recs.copy_(r["levs"])
                g.hue_recs.copy_(r["hues"])
                g._check(g.L.crthip_bind_levels(g.ctx, vp(g.level_recs.data_ptr()), C.byref(r["lenv"])), "crthip_bind_levels")
                g._check(g.L.crthip_bind_hues(g.ctx, vp(g.hue_recs.data_ptr()), C.byref(r["henv"])), "crthip_bind_hues")
            else:
                g.level_recs.fill_(0x5a5a5a5a)         # unbound: no later call may read them
                g.hue_recs.fill_(0x5a5a5a5a)
                g._check(g.L.crthip_bind_levels(g.ctx, None, None), "crthip_bind_levels")
                g._check(g.L.crthip_bind_hues(g.ctx, None, None), "crthip_bind_hues")
            g.fieldpass_knobs(s, None, params=p)
        if st["signal"] is not None:
            padded = C.c_int(-1)
            g._check(g.L.crthip_fieldpass_signal(g.ctx, AC.N, vp(self.snap_sig[i].data_ptr()), C.byref(padded)), "crthip_fieldpass_signal")
            self.padded[i] = bool(padded.value)
        # the snapshot: the caller's next operation on its stream
        self.snap_out[i].copy_(g.out)
        self.snap_state[i].copy_(g.state)
        if self.snap_hist is not None:
            self.snap_hist[i].copy_(g.vhs_hist)

    def _plug(self, seconds, cycles_per_s):
        torch = self.torch
        torch.cuda._sleep(int(seconds * cycles_per_s))
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def run_waited(self):
        """-> host seconds spent enqueuing the chain: every call with its record copies and its snapshot; the waits between the calls
        are not counted"""
        torch = self.torch
        spent = 0.0
        with torch.cuda.stream(self.stream):
            for i in range(len(self.ch["steps"])):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                self._call(i)
                spent += time.perf_counter() - t0
                torch.cuda.synchronize()
        return spent

    def run_chained(self, plug_s, cycles_per_s):
        """-> (host seconds from the first call to the last snapshot, GPU milliseconds from the plug's end to the last snapshot)"""
        torch = self.torch
        steps, what = self.ch["steps"], self.ch["id"]
        lost = ("%s: the plug (%.3f ms) had ended %s, %.3f ms of host time after it was enqueued: the host waited for the GPU, or was "
                "slower than %g x its median -- this run does not show that the calls were enqueued on pending work")
        with torch.cuda.stream(self.stream):
            torch.cuda.synchronize()
            t0 = t_plug = time.perf_counter()
            first = ev = self._plug(plug_s, cycles_per_s)
            for i, st in enumerate(steps):
                self._call(i)
                if st["waits"] is None:
                    assert not ev.query(), lost % (what, plug_s * 1e3, "after call %d (%s)" % (i, st["call"]), (time.perf_counter() - t_plug) * 1e3, PLUG_FACTOR)
                else:                                  # a host wait by design: a fresh plug behind it
                    t_plug = time.perf_counter()
                    ev = self._plug(plug_s, cycles_per_s)
            if steps[-1]["waits"] is None:
                assert not ev.query(), lost % (what, plug_s * 1e3, "after the last snapshot", (time.perf_counter() - t_plug) * 1e3, PLUG_FACTOR)
            host = time.perf_counter() - t0
            end = torch.cuda.Event(enable_timing=True)
            end.record()
            torch.cuda.synchronize()
        return host, first.elapsed_time(end)

    def close(self):
        self.torch.cuda.synchronize()
        self.graph = None
        for g in self.gs:
            g.close()


_EXPECTED = {}


def _expected_on_device(crtlib, cid):
    """(unit of every field [N], per call: (takes part [U], pictures [U, bytes], (hsync, vsync, rn) [U, 3], inp [U, bytes] or None))
    of the oracle, on the device; computed once per chain"""
    import torch
    if cid not in _EXPECTED:
        ch = AC.get(cid)
        exp, nxt = AC.expected(cid)
        us = AC.units(ch)
        unit_of = np.zeros(AC.N, dtype=np.int64)
        for u, (_cls, _part, fields) in enumerate(us):
            unit_of[fields] = u
        per_call = []
        for i, st in enumerate(ch["steps"]):
            per = [exp[u][i] for u in range(len(us))]
            assert not any(w is not None and w["ub"] for w in per), "%s: a field under the reference-UB rule (tests/test_async_cpu.py)" % cid
            some = next(w for w in per if w is not None)
            part = np.array([w is not None for w in per])
            out = np.stack([w["out"] if w is not None else np.zeros_like(some["out"]) for w in per])
            state = np.array([[w["hsync"], w["vsync"], w["rn"]] if w is not None else [0, 0, 0] for w in per], dtype=np.int64).astype(np.uint32).view(np.int32)
            inp = torch.from_numpy(np.stack([w["inp"] for w in per])).to("cuda:0") if st["signal"] is not None else None
            per_call.append((torch.from_numpy(part).to("cuda:0"), torch.from_numpy(out).to("cuda:0"), torch.from_numpy(state).to("cuda:0"), inp))
        _EXPECTED[cid] = (torch.from_numpy(unit_of).to("cuda:0"), per_call, nxt)
    return _EXPECTED[cid]


def _against_oracle(crtlib, run, cid):
    """-> the list of what differs from the oracle (empty: every field of every snapshot agrees)"""
    import torch
    ch = AC.get(cid)
    unit_of, per_call, nxt = _expected_on_device(crtlib, cid)
    cols = torch.tensor([crtlib.ST_HSYNC, crtlib.ST_VSYNC, crtlib.ST_RN], device="cuda:0")
    bad = []

    def first_bad(eq_rows, among):
        wrong = among & ~eq_rows
        k = int(wrong.nonzero()[0])
        return "%d of %d fields, the first: field %d (class %d)" % (int(wrong.sum()), int(among.sum()), k, AC.class_of(k))

    for i, st in enumerate(ch["steps"]):
        what = "%s call %d (%s)" % (cid, i, st["call"])
        part_u, out, state, inp = per_call[i]
        part = part_u[unit_of]
        got_out = run.snap_out[i].reshape(AC.N, -1)
        got_st = run.snap_state[i]
        checks = [("(hsync, vsync, rn)", (got_st[:, cols] == state[unit_of]).all(dim=1)), ("the picture", (got_out == out[unit_of]).all(dim=1))]
        if st["signal"] is not None:
            if run.padded[i] != st["signal"]:
                bad.append(what + ": the workspace's layout is reported as padded=%s" % run.padded[i])
            checks.append(("the signal", (run.snap_sig[i][:, :inp.shape[1]] == inp[unit_of]).all(dim=1)))
        if run.snap_hist is not None:
            h = run.snap_hist[i].cpu().numpy().view(np.uint32).astype(np.uint64)
            got_next = ((h[:, 0] + h[:, 28]) & 0xffffffff) >> 1
            want = np.array([nxt[(AC.class_of(k), i)] for k in range(AC.N)], dtype=np.uint64)
            checks.append(("the generator (next rand())", torch.from_numpy(got_next == want).to("cuda:0")))
        for name, eq in checks:
            if not bool((eq | ~part).all()):
                bad.append("%s: %s of %s" % (what, name, first_bad(eq, part)))
        # a call over fewer fields leaves the others as they were: as the previous snapshot of this context's sets has them (before
        # the first call: zeros and the start state); the (field, frame, aux) columns are the test's own
        if not bool(part.all()):
            prev = [j for j in range(i) if ch["steps"][j]["ctx"] == st["ctx"]]
            out0 = run.snap_out[prev[-1]].reshape(AC.N, -1) if prev else torch.zeros_like(got_out)
            st0 = run.snap_state[prev[-1]] if prev else run.state0
            eq = (got_out == out0).all(dim=1) & (got_st[:, 3:] == st0[:, 3:]).all(dim=1)
            if not bool((eq | part).all()):
                bad.append("%s: a call over %d fields wrote pictures or states of %s" % (what, AC.fields_of(st), first_bad(eq, ~part)))
    return bad


def _runs_differ(a, b):
    import torch
    bad = []
    for i in range(a.snap_out.shape[0]):
        for name, x, y in (("pictures", a.snap_out[i], b.snap_out[i]), ("states", a.snap_state[i], b.snap_state[i])):
            if not torch.equal(x, y):
                bad.append("call %d: %s" % (i, name))
        if a.snap_hist is not None and not torch.equal(a.snap_hist[i], b.snap_hist[i]):
            bad.append("call %d: generator histories" % i)
        if i in a.snap_sig and not torch.equal(a.snap_sig[i], b.snap_sig[i]):
            bad.append("call %d: signal" % i)
    return bad


@pytest.mark.parametrize("cid,overlap,kind", AC.GPU_IDS, ids=["%s-ov%d-%s" % t for t in AC.GPU_IDS])
def test_a_chain_enqueued_without_waiting_gives_what_the_waited_one_gives(crtlib, cycles_per_s, cid, overlap, kind):
    ch = AC.get(cid)
    _expected_on_device(crtlib, cid)
    waited, times = None, []
    for _ in range(3):
        if waited is not None:
            waited.close()
        waited = _Run(crtlib, ch, overlap, kind)
        times.append(waited.run_waited())
    chained = None
    try:
        waited_bad = _against_oracle(crtlib, waited, cid)
        enqueue = sorted(times)[1]
        plug_s = min(PLUG_FACTOR * enqueue, PLUG_CAP_S)
        chained = _Run(crtlib, ch, overlap, kind)
        host, gpu_ms = chained.run_chained(plug_s, cycles_per_s)
        print("ASYNC_PROFILE %s-ov%d-%s: host enqueue %.3f ms (median of %s), plug %.3f ms, chained: host %.3f ms, GPU %.3f ms behind the plug"
              % (cid, overlap, kind, enqueue * 1e3, " ".join("%.3f" % (t * 1e3) for t in times), plug_s * 1e3, host * 1e3, gpu_ms))
        chained_bad = _against_oracle(crtlib, chained, cid)
        differ = _runs_differ(chained, waited)
        verdict = ("the waited run agrees with the oracle: an ORDERING fault" if not waited_bad else
                   "the waited run differs from the oracle too (%s): not only ordering" % "; ".join(waited_bad[:3]))
        assert not chained_bad, "%s\n%s\nchained against waited: %s" % ("\n".join(chained_bad[:8]), verdict, "; ".join(differ) or "equal")
        assert not waited_bad, "the waited run differs from the oracle: " + "\n".join(waited_bad[:8])
        assert not differ, "the chained run differs from the waited one: " + "; ".join(differ)
    finally:
        waited.close()
        if chained is not None:
            chained.close()

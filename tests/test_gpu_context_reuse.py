"""A long-lived context: what a call computes must not depend on what the context did before.  bench.py, the drop-in layer, a video
player and tools/node_bench.c keep one crthip context for the life of the process, and a context carries a lot from call to call: the
signal workspace shared by the flat and the padded layout (zeroed once, when it is reserved), the encoder's cached tables, the layout
of the last pass, the bloom decoder's sort scratch.  Every other GPU test works on a fresh context.

The call programs of tests/reuse_cases.py run here on ONE context each.  After every call: the picture, hsync, vsync, rn and the burst
integrators of every field against the oracle at tolerance 0, and for a fused field-pass its signal (crthip_fieldpass_signal, repacked
to the reference's layout) against the oracle's inp[] and the `padded` flag against the program.  The same program runs a second time
with a fresh context for every call, on television sets of its own that are carried over in the same way: byte equality of the two
runs on every field localises a failure to the context's history rather than to a kernel.  A field for which the reference itself
reads past inp[] + 16 (crtref.reads_past_inp) leaves both comparisons from that call on; how many may is a cap set on the oracle
alone (tests/test_context_reuse_cpu.py asserts the same caps without a GPU)."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import reuse_cases as RC
import seqsets_cases as SC

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


def _settings(crtlib, prog, si):
    """device settings of call si (every image followed by a readable row: crt_ntsc.c:263)"""
    import torch
    st, n = prog["steps"][si], prog["n"]
    imgs, sk = RC.images(prog, st), st["sk"]
    if st["call"] in ("sequence", "sequence_sets"):
        case = RC.seq_case(prog, st)
        par = [(a, b, d) for (a, b), d in zip(SC.parities(case), SC.dot_crawl(case))]
    else:
        par = [RC.parity(prog, si, k) for k in range(n)]
    geo = dict(hue=sk.get("hue", 0), xoffset=sk.get("xoffset", 0), yoffset=sk.get("yoffset", 0))
    h = imgs.shape[1]
    if RC.is_nes(prog):
        full = torch.zeros((n, h + 1, imgs.shape[2]), dtype=torch.int16, device="cuda:0")
        full[:, :h] = _to_dev(imgs.astype(np.int16))
        full[:, h] = full[:, h - 1]
        return crtlib.Settings(full[:, :h], dot_crawl_offset=[p[2] for p in par], border_color=sk.get("border_color", 0), **geo)
    full = torch.zeros((n, h + 1) + tuple(imgs.shape[2:]), dtype=torch.uint8, device="cuda:0")
    full[:, :h] = _to_dev(imgs)
    full[:, h] = full[:, h - 1]
    dot = R.SYSTEMS[prog["name"]][0] in R.DOT_CRAWL_SYSTEMS
    return crtlib.Settings(full[:, :h], format=crtlib.FMT_BGRA, as_color=sk.get("as_color", 1), field=[p[0] for p in par],
                           frame=[p[1] for p in par], dot_crawl_offset=[p[2] for p in par] if dot else 0, **geo)


class _Side:
    """one batch of television sets -- state and pictures belong to the test and are carried from call to call -- and the context
    its calls go through: one for the whole program (reuse) or a fresh one per call"""

    def __init__(self, crtlib, prog, reuse):
        import torch
        self.crtlib, self.prog, self.reuse = crtlib, prog, reuse
        n = prog["n"]
        self.out = torch.zeros((n, prog["outh"], prog["outw"], R.bpp4fmt(prog["ofmt"])), dtype=torch.uint8, device="cuda:0")
        self.state = torch.zeros((n, crtlib.STATE_INTS), dtype=torch.int32, device="cuda:0")
        self.power_on()
        start = [RC.start_state(prog, k) for k in range(n)]
        self.state[:, crtlib.ST_HSYNC] = torch.tensor([a for a, _ in start], dtype=torch.int32, device="cuda:0")
        self.state[:, crtlib.ST_VSYNC] = torch.tensor([b for _, b in start], dtype=torch.int32, device="cuda:0")
        self.stream = torch.cuda.Stream() if prog["stream"] else None
        self.g, self.graph, self.sw = None, None, {}

    def power_on(self):
        """crt_init for the television sets; the context is not told"""
        self.state.zero_()
        self.state[:, self.crtlib.ST_RN] = 194
        self.out.zero_()

    def context(self, st):
        prog = self.prog
        self.sw.update(st["sw"])
        if self.g is None or not self.reuse:
            self.close()
            g = self.crtlib.CRT(prog["n"], prog["outw"], prog["outh"], prog["ofmt"], prog["name"], device=0, out=self.out)
            g.state = self.state
            g.set_shape(prog["shape"])
            g.reserve(prog["n"])
            if self.stream is not None:
                g.use_stream(self.stream)
            self.g = g
        for name, v in self.sw.items():
            getattr(self.g, "set_" + name)(v)
        for name, v in RC.knobs_of(prog, st).items():
            setattr(self.g, name, v)
        return self.g

    def close(self):
        self.graph = None
        if self.g is not None:
            self.g.synchronize()
            self.g.close()
            self.g = None


def _partial_fieldpass(g, s, noise, m, what):
    """a call with m fields on a context reserved for more (legal in the C ABI; crtlib.CRT.fieldpass always passes its n)"""
    import torch
    p = g.params(s, noise)
    g._load_field_state(s)
    torch.cuda.synchronize()
    out_behind, state_behind = g.out[m:].clone(), g.state[m:].clone()
    rc = g.L.crthip_fieldpass(g.ctx, C.byref(p), m, C.c_void_p(s.data.data_ptr()), g._image_stride(s), C.c_void_p(g.out.data_ptr()),
                              g.out.stride(0), C.c_void_p(g.state.data_ptr()))
    g._check(rc, "crthip_fieldpass")
    torch.cuda.synchronize()
    assert torch.equal(g.out[m:], out_behind), "%s: a call with %d fields wrote pictures behind them" % (what, m)
    assert torch.equal(g.state[m:], state_behind), "%s: a call with %d fields wrote states behind them" % (what, m)


def _signal(g, m):
    import torch
    dst = torch.zeros((m, g.fstride), dtype=torch.int8, device=g.dev)
    padded = C.c_int(0)
    torch.cuda.synchronize()
    g._check(g.L.crthip_fieldpass_signal(g.ctx, m, C.c_void_p(dst.data_ptr()), C.byref(padded)), "crthip_fieldpass_signal")
    torch.cuda.synchronize()
    return dst.cpu().numpy(), bool(padded.value)


def _check_signal(g, m, want, padded_want, what):
    sig, padded = _signal(g, m)
    assert padded == padded_want, "%s: the workspace's layout is reported as padded=%s" % (what, padded)
    for k, w in want.items():
        if w is not None:
            np.testing.assert_array_equal(sig[k, :w["inp"].size], w["inp"], err_msg="%s field %d: inp of the fused path" % (what, k))


def _call(side, si, what, last_good):
    """call si of the program through the side's context.  last_good: (oracle results, fields, padded) of the last pass that succeeded"""
    import torch
    crtlib, prog = side.crtlib, side.prog
    st = prog["steps"][si]
    g = side.context(st)
    call, m, noise = st["call"], RC.fields_of(prog, st), RC.noise_of(prog, st)
    if st["reset"] or call in ("sequence", "sequence_sets"):
        side.power_on()
    if call == "capture" and not side.reuse:
        return                                          # (the fresh side runs the replays as eager passes)
    s = _settings(crtlib, prog, si)
    torch.cuda.synchronize()
    if call == "fieldpass":
        if m == prog["n"] and side.stream is None:
            g.fieldpass(s, noise)
        elif m == prog["n"]:
            # the context launches on a stream of its own: the state columns (written on torch's stream) are loaded first
            p = g.params(s, noise)
            g._load_field_state(s)
            torch.cuda.synchronize()
            g.fieldpass(s, noise, params=p)
        else:
            _partial_fieldpass(g, s, noise, m, what)
    elif call == "stages":
        g.modulate(s)
        g.demodulate(noise)
    elif call in ("sequence", "sequence_sets"):
        case = RC.seq_case(prog, st)
        for (lo, _hi), (hs, vs, rn) in zip(SC.sets_of(case), SC.incoming(case)):
            side.state[lo, crtlib.ST_HSYNC] = hs
            side.state[lo, crtlib.ST_VSYNC] = vs
            side.state[lo, crtlib.ST_RN] = rn if rn < 2 ** 31 else rn - 2 ** 32
        init = _to_dev(RC.seq_init(prog))
        torch.cuda.synchronize()
        if call == "sequence":
            g.sequence(s, noise, out_init=init)
        else:
            g.sequence_sets(s, noise, st["set_first"], out_init=init)
    elif call == "capture":
        p = g.params(s, noise)
        g._load_field_state(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side.stream):
            g.fieldpass(s, noise, params=p)
        side.graph = (graph, s)                         # (the graph reads s.data: kept alive, never written)
    elif call == "replay":
        if side.reuse:
            g._load_field_state(side.graph[1])
            torch.cuda.synchronize()
            side.graph[0].replay()
        else:
            p = g.params(s, noise)
            g._load_field_state(s)
            torch.cuda.synchronize()
            g.fieldpass(s, noise, params=p)
    elif call == "refused_encoder":
        # check_encoder's CRTHIP_E_ARG on the host: no kernel is launched
        g._load_field_state(s)
        torch.cuda.synchronize()
        out0, state0 = side.out.clone(), side.state.clone()
        with pytest.raises(RuntimeError, match="out of contract"):
            g.fieldpass(s, noise)
        torch.cuda.synchronize()
        assert torch.equal(side.out, out0) and torch.equal(side.state, state0), "%s: a refused call wrote pictures or states" % what
        if side.reuse:                                  # the signal of the last successful pass, with its own flag
            _check_signal(g, last_good[1], last_good[0], last_good[2], what + ": signal after the refusal")
        else:
            with pytest.raises(RuntimeError):
                _signal(g, m)
    elif call == "refused_decoder":
        # the decoder's argument checks come after the encoder and the sync chain have been enqueued: the workspace holds a
        # signal, but of no pass that went through -- crthip_fieldpass_signal has nothing to report
        p = g.params(s, noise)
        p.eq_g[0][1] += 1
        g._load_field_state(s)
        torch.cuda.synchronize()
        out0, state0 = side.out.clone(), side.state.clone()
        with pytest.raises(RuntimeError, match="equaliser gains"):
            g.fieldpass(s, noise, params=p)
        torch.cuda.synchronize()
        assert torch.equal(side.out, out0), "%s: the refused call wrote pictures" % what
        with pytest.raises(RuntimeError, match="no field-pass"):
            _signal(g, m)
        side.state.copy_(state0)                        # the sync chain of the refused pass ran: the test puts its sets back
    else:
        raise ValueError(call)
    torch.cuda.synchronize()


def _check_against_oracle(side, want, what):
    import torch
    crtlib = side.crtlib
    orc = R.Oracle(side.prog["name"])
    ks = sorted(want)
    out = side.out[torch.tensor(ks, device="cuda:0")].cpu().numpy()
    state = side.state.cpu().numpy()
    for j, k in enumerate(ks):
        w = want[k]
        if w is None:
            continue                                    # the reference reads past inp[] here: undefined, not compared
        msg = "%s field %d" % (what, k)
        got = (int(state[k, crtlib.ST_HSYNC]), int(state[k, crtlib.ST_VSYNC]), int(state[k, crtlib.ST_RN]))
        assert got == (w["hsync"], w["vsync"], w["rn"]), "%s: (hsync, vsync, rn) %s, oracle %s" % (msg, got, (w["hsync"], w["vsync"], w["rn"]))
        if "ccf" in w:
            ccf = state[k, crtlib.ST_CCF:crtlib.ST_CCF + 25].reshape(5, 5)[:orc.vper, :orc.ccs]
            np.testing.assert_array_equal(ccf, w["ccf"], err_msg=msg + " ccf")
        np.testing.assert_array_equal(out[j].reshape(-1), w["out"], err_msg=msg + " out")


def _check_sides_agree(old, fresh, want, what):
    for k in sorted(want):
        if want[k] is None:
            continue
        assert bool((old.state[k] == fresh.state[k]).all()), "%s field %d: the state depends on the context's history" % (what, k)
        assert bool((old.out[k] == fresh.out[k]).all()), "%s field %d: the picture depends on the context's history" % (what, k)


@pytest.mark.parametrize("pid", RC.PROGRAM_IDS)
def test_results_do_not_depend_on_what_the_context_did_before(crtlib, pid):
    prog = RC.program(pid)
    oracle = RC.OracleRun(prog)
    old, fresh = _Side(crtlib, prog, True), _Side(crtlib, prog, False)
    last_good = None
    try:
        for si, st in enumerate(prog["steps"]):
            what = "%s call %d (%s, %d fields)" % (pid, si, st["call"], RC.fields_of(prog, st))
            want = oracle.run(si)
            _call(old, si, what + " on the old context", last_good)
            _call(fresh, si, what + " on a fresh context", last_good)
            if not want:
                continue
            _check_against_oracle(old, want, what + " on the old context")
            if st["call"] == "fieldpass":
                _check_signal(old.g, RC.fields_of(prog, st), want, st["expect"][0], what + " on the old context")
                _check_signal(fresh.g, RC.fields_of(prog, st), want, st["expect"][0], what + " on a fresh context")
                last_good = (want, RC.fields_of(prog, st), st["expect"][0])
            _check_against_oracle(fresh, want, what + " on a fresh context")
            _check_sides_agree(old, fresh, want, what)
    finally:
        old.close()
        fresh.close()
    print("%s: %d of %d (field, call) pairs compared, %d under the reference-UB rule" % (pid, oracle.kept, oracle.total, oracle.total - oracle.kept))
    if prog["keep"] == 1.0:
        assert oracle.kept == oracle.total, "%s: %d pairs fell under the UB rule, none may" % (pid, oracle.total - oracle.kept)
    else:
        assert oracle.kept >= prog["keep"] * oracle.total, "%s: only %d of %d pairs compared" % (pid, oracle.kept, oracle.total)

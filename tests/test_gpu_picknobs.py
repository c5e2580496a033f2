"""The picture knobs on the GPU: brightness and contrast per field (crthip_knobs_prepare5) through all six per-field-knob entry points,
bit for bit against the oracle run per field with its five knobs, or -- sequence mode -- the reference's serial loop on ONE struct CRT
whose knobs are turned between the fields (tests/picknobs_cases.py): the picture, inp[] where the entry point exposes it, and
hsync / vsync / rn / ccf.  The case rows sit on the bounds the decoder tiers branch on, neighbours on opposite sides; no field of any
case is excluded (none falls into the reference's undefined over-read: tests/test_picknobs_cpu.py, and asserted here)."""
import ctypes as C
import os

import numpy as np
import pytest

import crtref as R
import knobs_cases as KC
import picknobs_cases as PK
import seqknobs_cases as SK
from test_gpu_knobs import _compare, _device_images, _next_parity
from test_gpu_seqknobs import _compare as _seq_compare, _inits, _make as _seq_make, _same, _set_incoming, _snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_knobs_prepare5")
    return crtlib


def _make(crtlib, name, geo, n, crt_knobs=None, shape=1, sig_pad=1, exact=0, dec_float=None, fmt=None, seeds=None, wide_lpw=0):
    """a fresh context (CRTHIP_DEC_FLOAT is read when a context is created; the environment is restored) + its settings"""
    old = os.environ.get("CRTHIP_DEC_FLOAT")
    if dec_float is not None:
        os.environ["CRTHIP_DEC_FLOAT"] = "1" if dec_float else "0"
    try:
        g = crtlib.CRT(n, geo["outw"], geo["outh"], crtlib.FMT_BGRA if fmt is None else fmt,
                       name[:4] if name.startswith("ntscfir") else name, device=0)
    finally:
        if dec_float is not None:
            if old is None:
                del os.environ["CRTHIP_DEC_FLOAT"]
            else:
                os.environ["CRTHIP_DEC_FLOAT"] = old
    g.eq_fir = R.EQ_KERNEL.get(name, 0)
    g.scanlines = 1
    for a, v in (crt_knobs or {}).items():
        setattr(g, a, v)
    g.set_shape(shape)
    g.set_signal_layout(sig_pad)
    g.set_exact(exact)
    g.set_wide_lpw(wide_lpw)
    if seeds is not None:
        g.srand(seeds)
    par = [KC.parity(k) for k in range(n)]
    dc = R.Oracle(name).system in R.DOT_CRAWL_SYSTEMS
    s = crtlib.Settings(_device_images(name, geo, n), format=crtlib.FMT_BGRA, as_color=1,
                        field=[a for a, _ in par], frame=[b for _, b in par],
                        dot_crawl_offset=[KC.dot_crawl(name, k) for k in range(n)] if dc else 0)
    return g, s


def _bounds_want(cid, fmt=R.FMT_BGRA, geo=PK.SMALL):
    return PK.expected(("ntsc", cid, 2) if (fmt, geo) == (R.FMT_BGRA, PK.SMALL) else ("ntsc", cid, 2, fmt, geo["outw"], geo["outh"]),
                       lambda: PK.oracle_fields5("ntsc", geo, PK.BOUND_CASES[cid], steps=2, fmt=fmt))


# (shape, padded signal lines, set_exact, float stages switch): both kernel shapes x both signal layouts; the exact kernels; the float
# switch on and off (a picture-knob call runs the integer stages either way and must say so)
CONFIGS = [(1, 1, 0, True), (1, 0, 0, True), (2, 1, 0, True), (2, 0, 0, True), (1, 1, 1, True), (2, 1, 1, True), (1, 1, 0, False),
           (1, 1, 2, True), (1, 1, 3, True)]


@pytest.mark.parametrize("shape,sig_pad,exact,dec_float", CONFIGS)
@pytest.mark.parametrize("cid", sorted(PK.BOUND_CASES))
def test_fieldpass_knobs_at_the_bounds(crtlib, cid, shape, sig_pad, exact, dec_float):
    """two field-passes in a row per table; every field against its own oracle run"""
    rows = PK.BOUND_CASES[cid]
    want = _bounds_want(cid)
    g, s = _make(crtlib, "ntsc", PK.SMALL, len(rows), shape=shape, sig_pad=sig_pad, exact=exact, dec_float=dec_float)
    for step in range(2):
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, step, "%s shape %d pad %d exact %d float %d" % (cid, shape, sig_pad, exact, dec_float))
        assert g.float_stages_used() == 0                   # picture-knob calls take the integer stages
        _next_parity(s, step)
    assert g._knob_env.pic == 1
    g.close()


@pytest.mark.parametrize("shape", [1, 2])
@pytest.mark.parametrize("cid", ["bright", "allfive"])
def test_three_byte_output(crtlib, cid, shape):
    """101 x 77 RGB: the 3-byte instantiations, an odd width wider than one pixel tile"""
    geo = dict(PK.SMALL, outw=101, outh=77)
    rows = PK.BOUND_CASES[cid]
    want = _bounds_want(cid, R.FMT_RGB, geo)
    g, s = _make(crtlib, "ntsc", geo, len(rows), shape=shape, fmt=crtlib.FMT_RGB)
    for step in range(2):
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, step, "%s rgb shape %d" % (cid, shape))
        _next_parity(s, step)
    g.close()


@pytest.mark.parametrize("lpw", [8, 16])
@pytest.mark.parametrize("cid", ["bright", "both"])
def test_wide_run_decoder(crtlib, cid, lpw):
    """a picture 1700 wide takes the wide-run decoder for its tier-0 / 1 groups (both instantiations pinned), k_decode's PK
    instantiations for the rest: 240 lines = 3.75 groups of 64 per field, so groups straddle the fields of different floors"""
    geo = dict(PK.SMALL, outw=1700, outh=48)
    rows = PK.BOUND_CASES[cid]
    want = _bounds_want(cid, R.FMT_BGRA, geo)
    g, s = _make(crtlib, "ntsc", geo, len(rows), shape=1, wide_lpw=lpw)
    g.fieldpass_knobs(s, np.array(rows))
    _compare(g, want, 0, "%s 1700x48 lpw %d" % (cid, lpw))
    g.close()


@pytest.mark.parametrize("name,n", [("nes", 6), ("vhs", 5), ("vhslcg", 6), ("ntscbloom", 6), ("ntscfir7", 4), ("snes", 5)])
def test_one_case_per_system_and_build(crtlib, name, n):
    """NES, the rand()-noise VHS build, VHS with the LCG noise, a bloom build (the beam-width sort gathers lines of different fields
    into one wavefront), the 7-tap FIR decoder (floors -> its tiers 4 / 5), a system with per-line-class carriers"""
    geo = dict(w=256, h=240, outw=320, outh=240) if name == "nes" else PK.SMALL
    rows = PK.per_system(name, n)
    seeds = [3 + 11 * k for k in range(n)] if name == "vhs" else None
    want = PK.oracle_fields5(name, geo, rows, steps=2, seeds=seeds)
    g, s = _make(crtlib, name, geo, n, seeds=seeds)
    for step in range(2):
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, step, name)
        _next_parity(s, step)
    g.close()


def test_bloom_build_on_the_scanline_parallel_shape(crtlib):
    rows = PK.per_system("ntscbloom", 6)
    want = PK.oracle_fields5("ntscbloom", PK.SMALL, rows, steps=1)
    g, s = _make(crtlib, "ntscbloom", PK.SMALL, 6, shape=2)
    g.fieldpass_knobs(s, np.array(rows))
    _compare(g, want, 0, "bloom rows")
    g.close()


# --- sequence mode ---------------------------------------------------------------------------------------------------------------
def _rows(case, lo=0, hi=None):
    return np.array(case["rows"][lo:hi])


@pytest.mark.parametrize("cid,shape", [("ramp", 1), ("ramp", 2), ("ramp-blend", 0), ("ramp-fade", 0)])
def test_sequence_knobs_ramp_and_step(crtlib, cid, shape):
    """a brightness ramp and a contrast step that cross the tier bounds mid-video, with and without blend, with the phosphor fade,
    against the serial loop on one struct CRT"""
    case = PK.SEQ_CASES[cid]
    g, s = _seq_make(crtlib, case, shape=shape, state_in=SK.incoming(case)[0])
    g.brightness, g.contrast = 77, 3                    # ignored: the records carry them
    g.sequence_knobs(s, _rows(case), out_init=_inits(case)[0])
    snap = _snapshot(g)
    g.close()
    _seq_compare(snap, PK.seq_expected(case), cid)


def test_sequence_sets_knobs_ragged_sets(crtlib):
    """three sets of 1, 4 and 2 fields, per-set incoming states and pictures: the oracle's loop per set"""
    case = PK.SEQ_CASES["sets"]
    g, s = _seq_make(crtlib, case)
    for (lo, _), inc in zip(SK.sets_of(case), SK.incoming(case)):
        _set_incoming(crtlib, g, lo, inc)
    g.sequence_sets_knobs(s, _rows(case), case["set_first"], out_init=_inits(case))
    snap = _snapshot(g)
    g.close()
    _seq_compare(snap, PK.seq_expected(case), "sets")


def test_phases_with_bound_picture_knobs_over_two_contexts(crtlib):
    """a video of 6 fields cut into shards of 4 and 2 on two contexts, every shard with ITS records bound (crthip_seq_bind_knobs)"""
    case = PK.SEQ_CASES["ramp"]
    want = PK.seq_expected(case)
    inc = SK.incoming(case)[0]
    prev_pic = _inits(case)[0]
    hv = inc[:2]
    for lo, hi in ((0, 4), (4, 6)):
        g, s = _seq_make(crtlib, case, lo, hi)
        g.seq_bind_knobs(_rows(case, lo, hi))
        g.seq_encode(s, 0, lo, inc[2])
        hv = g.seq_sync(*hv)
        g.seq_decode()
        g.seq_weave(out_init=prev_pic)
        _seq_compare(_snapshot(g), want, "shard %d..%d" % (lo, hi), lo=lo)
        prev_pic = g.out[hi - lo - 1].clone()
        g.close()


# --- nothing else changes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 2])
def test_the_params_own_picture_values_equal_the_three_knob_and_the_uniform_call(crtlib, shape):
    """all fields at the blob's brightness and contrast: byte for byte the (n, 3) call; all five uniform: the uniform call"""
    import torch
    knobs = dict(hue=-33, saturation=14, brightness=-12, contrast=222)
    res = []
    for which in ("uniform", "three", "five"):
        g, s = _make(crtlib, "ntsc", PK.SMALL, 6, crt_knobs=knobs, shape=shape)
        for step in range(2):
            if which == "uniform":
                g.fieldpass(s, 24)
            elif which == "three":
                g.fieldpass_knobs(s, np.array([(24, -33, 14)] * 6))
            else:
                g.fieldpass_knobs(s, np.array([(24, -33, 14, -12, 222)] * 6))
            _next_parity(s, step)
        g.synchronize()
        res.append((g.out.clone(), g.state.clone(), g.fieldpass_signal()[0].clone()))
        g.close()
    for other in res[1:]:
        for a, b, what in zip(res[0], other, ("out", "state", "signal")):
            assert torch.equal(a, b), what


def test_a_picture_knob_call_between_uniform_and_three_knob_calls_leaves_nothing_behind(crtlib):
    """one long-lived context: uniform, (n, 3), (n, 5), (n, 3), uniform -- each equal to the same call on a fresh context (the float
    stages come back for the calls that had them)"""
    import torch
    n = 6
    rows = np.array(PK.ALL_FIVE)

    def call(g, s, which):
        g.state.zero_()
        g.state[:, crtlib.ST_RN] = 194
        g.out.zero_()
        if which == "five":
            g.fieldpass_knobs(s, rows)
        elif which == "three":
            g.fieldpass_knobs(s, rows[:, :3])
        else:
            g.hue, g.saturation = which
            g.fieldpass(s, 30)
        g.synchronize()
        return g.out.clone(), g.state.clone(), g.float_stages_used()
    order = [(0, 10), "three", "five", "three", (25, 13)]
    fresh = {}
    for which in order:
        if which not in fresh:
            g, s = _make(crtlib, "ntsc", PK.SMALL, n)
            fresh[which] = call(g, s, which)
            g.close()
    assert fresh["five"][2] == 0
    g, s = _make(crtlib, "ntsc", PK.SMALL, n)
    for which in order:
        out, state, fl = call(g, s, which)
        assert torch.equal(out, fresh[which][0]) and torch.equal(state, fresh[which][1]) and fl == fresh[which][2], which
    g.close()
    want = _bounds_want("allfive")
    np.testing.assert_array_equal(fresh["five"][0][4].cpu().numpy().reshape(-1), want[4][0]["out"])


def test_graph_capture_reads_the_records_at_replay(crtlib):
    """capture one call; between the replays the record buffer is rewritten: a field moves from tier 0 to the exact tier and back
    (the env's bounds -- the smallest floor among them -- stay what the graph was captured with)"""
    import torch
    first = PK.BRIGHT_BOUNDS
    moved = list(first)
    moved[0], moved[7] = first[7], first[0]               # field 0: tier 0 -> exact; field 7: exact -> tier 0
    seq = [first, moved, first]
    want = {id(first): _bounds_want("bright"),
            id(moved): PK.expected("bright-moved", lambda: PK.oracle_fields5("ntsc", PK.SMALL, moved, steps=1))}
    n = len(first)
    g, s = _make(crtlib, "ntsc", PK.SMALL, n)
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
    for r, rows in enumerate(seq):
        env2 = g.upload_knobs(np.array(rows), p)
        assert bytes(env2) == bytes(env)
        g.state.copy_(state0)
        g.out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _compare(g, want[id(rows)], 0, "replay %d" % r, signal=False)
    del graph
    g.close()


def test_refusals_leave_out_and_state_untouched(crtlib):
    """the PV-1000; an env whose picture words do not belong to the records' kind (flag cleared over floors that are set, floors out
    of range, the smallest above the largest); an env of crthip_knobs_prepare5 passed with n off by one"""
    import torch
    n = 4
    g, s = _make(crtlib, "pv1k", PK.SMALL, n)
    g.out.fill_(37)
    g._load_field_state(s)
    state = g.state.clone()
    with pytest.raises(RuntimeError, match="PV-1000"):
        g.fieldpass_knobs(s, np.array(PK.BRIGHT_BOUNDS[:n]))
    g.synchronize()
    assert torch.equal(g.state, state) and bool((g.out == 37).all())
    g.close()

    g, s = _make(crtlib, "ntsc", PK.SMALL, n)
    L = g.L
    p = g.params(s, 0)
    g._load_field_state(s)
    g.out.fill_(91)
    torch.cuda.synchronize()
    state = g.state.clone()
    g.upload_knobs(np.array(PK.BRIGHT_BOUNDS[:n]), p)

    def call(env, count=n):
        return L.crthip_fieldpass_knobs(g.ctx, C.byref(p), count, C.c_void_p(s.data.data_ptr()), g._image_stride(s),
                                        C.c_void_p(g.out.data_ptr()), g.out.stride(0), C.c_void_p(g.state.data_ptr()),
                                        C.c_void_p(g.knob_recs.data_ptr()), C.byref(env))
    good = g._knob_env
    assert (good.pic, good.tier_floor_min, good.tier_floor_max) == (1, 0, 2)

    bad_n = crtlib.KnobsEnv.from_buffer_copy(bytes(good))
    bad_n.n = n - 1
    assert call(bad_n) == -1 and b"number of fields" in L.crthip_error_string(g.ctx)
    assert call(good, n - 1) == -1 and b"number of fields" in L.crthip_error_string(g.ctx)
    mism =[crtlib.KnobsEnv.from_buffer_copy(bytes(good)) for _ in range(4)]
    mism[0].reserved[0] = 0                                # flag cleared, floors still set
    mism[1].reserved[0] = 2                                # no such flag
    mism[2].reserved[1] = 0 | (4 << 8)                     # a floor that does not exist
    mism[3].reserved[1] = 2 | (0 << 8)                     # the smallest above the largest
    for e in mism:
        assert call(e) == -1 and b"picture words" in L.crthip_error_string(g.ctx)
    assert L.crthip_seq_bind_knobs(g.ctx, C.c_void_p(g.knob_recs.data_ptr()), C.byref(mism[0])) == -1
    g.synchronize()
    assert torch.equal(g.state, state) and bool((g.out == 91).all())
    assert call(good) == 0
    g.synchronize()
    assert not bool((g.out == 91).all())
    g.close()

"""Sequence mode with per-field knobs on the GPU (crthip_sequence_knobs / crthip_sequence_sets_knobs / crthip_seq_bind_knobs): one
running television set whose channel noise, monitor hue and saturation change from field to field, against the oracle driven field
by field on ONE CRT (tests/seqknobs_cases.py).  Every comparison covers the picture of every image and hsync / vsync / rn / ccf of
every field; no field of any case is excluded (none falls into the reference's undefined over-read: tests/test_seqknobs_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import knobs_cases as KC
import seqknobs_cases as SK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    L = crtlib.load_library()
    assert hasattr(L, "crthip_sequence_knobs") and hasattr(L, "crthip_sequence_sets_knobs") and hasattr(L, "crthip_seq_bind_knobs")
    return crtlib


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device_images(case, lo, hi):
    """fields [lo, hi) of the case, every image followed by one more readable row (the reference reads row h, crt_ntsc.c:263)"""
    import torch
    n = hi - lo
    if SK.is_nes(case):
        ppu = np.stack([SK.frame(case, k) for k in range(lo, hi)]).astype(np.int16)
        full = torch.zeros((n, 241, 256), dtype=torch.int16, device="cuda:0")
        full[:, :240] = _to_dev(ppu)
        full[:, 240] = full[:, 239]
        return full[:, :240]
    h, w = case["geo"]["h"], case["geo"]["w"]
    full = torch.zeros((n, h + 1, w, 4), dtype=torch.uint8, device="cuda:0")
    full[:, :h] = _to_dev(np.stack([SK.frame(case, k) for k in range(lo, hi)]))
    full[:, h] = full[:, h - 1]
    return full[:, :h]


def _make(crtlib, case, lo=0, hi=None, shape=0, state_in=None):
    """a CRT object + settings for fields [lo, hi) of the case; state_in: (hsync, vsync, rn) of the slice's set before its first field"""
    hi = SK.n_fields(case) if hi is None else hi
    name = case["name"]
    g = crtlib.CRT(hi - lo, case["geo"]["outw"], case["geo"]["outh"], crtlib.FMT_BGRA, name[:4] if name.startswith("ntscfir") else name,
                   device=0)
    g.eq_fir = R.EQ_KERNEL.get(name, 0)
    g.scanlines = 1
    for a, v in case["knobs"].items():
        setattr(g, a, v)
    g.phosphor = case["mode"]
    g.set_shape(shape)
    if case["seed"] is not None:
        g.srand([case["seed"]] * (hi - lo))                # entry 0 is the one that counts
    par, dco = SK.parities(case)[lo:hi], SK.dot_crawl(case)[lo:hi]
    s = crtlib.Settings(_device_images(case, lo, hi), format=crtlib.FMT_BGRA, as_color=1, hue=0,
                        field=[a for a, _ in par], frame=[b for _, b in par], dot_crawl_offset=dco if SK.is_nes(case) else 0)
    s.draw_aberration = case["aberration"]
    if state_in is not None:
        _set_incoming(crtlib, g, 0, state_in)
    return g, s


def _set_incoming(crtlib, g, k, state_in):
    g.state[k, crtlib.ST_HSYNC] = state_in[0]
    g.state[k, crtlib.ST_VSYNC] = state_in[1]
    g.state[k, crtlib.ST_RN] = state_in[2] if state_in[2] < 2 ** 31 else state_in[2] - 2 ** 32


def _knobs(case, lo=0, hi=None):
    return np.array(case["triples"][lo:hi])


def _inits(case):
    init = SK.init_pictures(case)
    return None if init is None else _to_dev(init)


def _snapshot(g):
    g.synchronize()
    return g.out.cpu().numpy(), g.get("hsync"), g.get("vsync"), g.get("rn"), g.ccf


def _compare(snap, want, what, lo=0):
    """every field of a snapshot against fields lo ... of the expected list"""
    out, hs, vs, rn, ccf = snap
    for j in range(out.shape[0]):
        w = want[lo + j]
        tag = "%s field %d" % (what, lo + j)
        assert w["undefined"] is False, tag + ": inside the reference's undefined over-read -- choose other knobs, exclude nothing"
        assert (hs[j], vs[j], rn[j]) == (w["hsync"], w["vsync"], w["rn"]), tag + " hsync / vsync / rn"
        np.testing.assert_array_equal(ccf[j, :w["ccf"].shape[0], :w["ccf"].shape[1]], w["ccf"], err_msg=tag + " ccf")
        np.testing.assert_array_equal(out[j].reshape(-1), w["out"], err_msg=tag + " out")


def _same(a, b, what):
    """two snapshots, byte for byte"""
    for x, y, part in zip(a, b, ("out", "hsync", "vsync", "rn", "ccf")):
        assert np.array_equal(np.asarray(x), np.asarray(y)), "%s: %s differs" % (what, part)


def _run_single(crtlib, case, shape=0):
    """crthip_sequence_knobs over a one-set case -> (snapshot, passes)"""
    assert len(case["set_first"]) == 2
    g, s = _make(crtlib, case, shape=shape, state_in=SK.incoming(case)[0])
    init = _inits(case)
    passes = g.sequence_knobs(s, _knobs(case), out_init=None if init is None else init[0])
    snap = _snapshot(g)
    g.close()
    return snap, passes


def _run_sets(crtlib, case, shape=0):
    """crthip_sequence_sets_knobs over the whole case -> (snapshot, passes)"""
    g, s = _make(crtlib, case, shape=shape)
    for (lo, _), inc in zip(SK.sets_of(case), SK.incoming(case)):
        _set_incoming(crtlib, g, lo, inc)
    passes = g.sequence_sets_knobs(s, _knobs(case), case["set_first"], out_init=_inits(case))
    snap = _snapshot(g)
    g.close()
    return snap, passes


# --- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 2])
def test_six_fields_six_triples_on_one_set(crtlib, shape):
    """a clean field in the middle, saturations on both sides of tier 0's chroma bound, hues that flip tier flags inside one
    wavefront, noise that keeps the sync fixed point going for more than two passes (the records are re-read on every pass); both
    kernel shapes"""
    case = SK.case("six")
    snap, passes = _run_single(crtlib, case, shape)
    print("six fields, shape %d: %d sync passes" % (shape, passes))
    _compare(snap, SK.expected(case), "six shape %d" % shape)
    assert passes > 2


# --- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["six-blend", "six-fade", "six-clear", "six-blend-fade", "six-blend-clear"])
def test_blend_and_the_display_modes(crtlib, cid):
    """blend = 1 at the smallest outh the blend rule accepts; phosphor fade and clear, with and without blend"""
    case = SK.case(cid)
    snap, _ = _run_single(crtlib, case)
    _compare(snap, SK.expected(case), cid)


# --- 3 -------------------------------------------------------------------------------------------------------------------------
def test_seventy_fields_every_one_its_own_triple(crtlib):
    """more than one wavefront of fields in the per-field kernels and a ragged last one; triples from a fixed seed"""
    case = SK.case("seventy")
    snap, passes = _run_single(crtlib, case)
    print("seventy fields: %d sync passes" % passes)
    _compare(snap, SK.expected(case), "seventy")


# --- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,shape", [("bloom", 0), ("bloom", 1), ("fir7", 0), ("nes", 0)])
def test_bloom_fir_and_nes(crtlib, cid, shape):
    """the bloom build with per-field noise (max_e from the field's noise; also through the beam-width sort of shape 1), the 7-tap
    FIR decoder, and the NES with dot_crawl_offset cycling"""
    case = SK.case(cid)
    snap, _ = _run_single(crtlib, case, shape)
    _compare(snap, SK.expected(case), "%s shape %d" % (cid, shape))


# --- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["vhs", "vhs-aberration"])
def test_vhs_rand_noise_on_one_set(crtlib, cid):
    """the rand()-noise VHS build: the fields share one rand() stream, per-field noise; with CRTHIP_F_VHS_DRAW_ABERRATION the
    aberration heights are drawn from it as well"""
    case = SK.case(cid)
    snap, _ = _run_single(crtlib, case)
    _compare(snap, SK.expected(case), cid)


def test_vhs_lcg_noise_through_the_sets_call(crtlib):
    case = SK.case("vhslcg-sets")
    snap, _ = _run_sets(crtlib, case)
    _compare(snap, SK.expected(case), "vhslcg sets")


# --- 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["sets", "sets-blend-fade"])
def test_sets_equal_the_single_set_call_per_set_and_the_oracle(crtlib, cid):
    """three sets of lengths 1, 4 and 2 with per-set initial pictures and incoming states: the oracle's loop per set, and
    crthip_sequence_knobs called once per set on the set's slices of images, output, state AND records"""
    case = SK.case(cid)
    snap, passes = _run_sets(crtlib, case)
    _compare(snap, SK.expected(case), cid)
    init, inc = _inits(case), SK.incoming(case)
    per_set_passes = []
    for si, (lo, hi) in enumerate(SK.sets_of(case)):
        g, s = _make(crtlib, case, lo, hi, state_in=inc[si])
        per_set_passes.append(g.sequence_knobs(s, _knobs(case, lo, hi), out_init=init[si]))
        one = _snapshot(g)
        g.close()
        _same(tuple(np.asarray(x)[lo:hi] for x in snap), one, "%s set %d" % (cid, si))
    assert passes == max(per_set_passes)


def test_one_set_through_the_sets_call_equals_the_single_set_call(crtlib):
    case = SK.case("six-blend-fade")
    a, pa = _run_single(crtlib, case)
    b, pb = _run_sets(crtlib, case)
    _same(a, b, "one set")
    assert pa == pb


# --- 7 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["six-blend-fade", "sets"])
def test_uniform_knobs_equal_the_uniform_entry_point(crtlib, cid):
    """all records equal: byte for byte crthip_sequence / crthip_sequence_sets with those values in the parameter blob"""
    case = SK.case(cid)
    noise, hue, sat = 30, -33, 14
    n = SK.n_fields(case)
    res = []
    for knobs in (False, True):
        g, s = _make(crtlib, case)
        for (lo, _), inc in zip(SK.sets_of(case), SK.incoming(case)):
            _set_incoming(crtlib, g, lo, inc)
        init = _inits(case)
        single = len(case["set_first"]) == 2
        if knobs:
            trip = np.array([(noise, hue, sat)] * n)
            g.hue, g.saturation = 200, 3                    # ignored by the knob entry points
            passes = g.sequence_knobs(s, trip, out_init=init[0]) if single else g.sequence_sets_knobs(s, trip, case["set_first"], out_init=init)
        else:
            g.hue, g.saturation = hue, sat
            passes = g.sequence(s, noise, out_init=init[0]) if single else g.sequence_sets(s, noise, case["set_first"], out_init=init)
        res.append((_snapshot(g), passes))
        g.close()
    _same(res[0][0], res[1][0], cid + " uniform")
    assert res[0][1] == res[1][1]


# --- 8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["six", "six-blend-fade"])
def test_phases_with_bound_knobs_over_two_contexts(crtlib, cid):
    """a video of 6 fields cut into shards of 4 and 2 on two contexts: first_index, the predecessor's final hsync / vsync and its
    last picture as d_out_init, every shard with ITS records bound -- equal to the single call (and the oracle)"""
    case = SK.case(cid)
    whole, _ = _run_single(crtlib, case)
    _compare(whole, SK.expected(case), cid)
    inc = SK.incoming(case)[0]
    init = _inits(case)
    prev_pic = None if init is None else init[0]
    hv = inc[:2]
    for lo, hi in ((0, 4), (4, 6)):
        g, s = _make(crtlib, case, lo, hi)
        g.seq_bind_knobs(_knobs(case, lo, hi))
        g.seq_encode(s, 0, lo, inc[2])                      # (the blob's own noise is ignored once records are bound)
        hv = g.seq_sync(*hv)
        g.seq_decode()
        g.seq_weave(out_init=prev_pic)
        shard = _snapshot(g)
        _same(tuple(np.asarray(x)[lo:hi] for x in whole), shard, "%s shard %d..%d" % (cid, lo, hi))
        prev_pic = g.out[hi - lo - 1].clone()
        g.close()


def test_bound_phases_require_the_shards_field_count(crtlib):
    case = SK.case("six")
    g, s = _make(crtlib, case, 0, 4)
    g2, s2 = _make(crtlib, case, 0, 3)                      # records prepared for another number of fields
    env = g2.upload_knobs(_knobs(case, 0, 3), g2.params(s2, 0))
    assert g.L.crthip_seq_bind_knobs(g.ctx, C.c_void_p(g2.knob_recs.data_ptr()), C.byref(env)) == 0
    with pytest.raises(RuntimeError, match="number of fields"):
        g.seq_encode(s, 0, 0, 194)
    g.seq_bind_knobs(None)
    g.seq_encode(s, 24, 0, 194)                             # unbound: the uniform phase
    g.synchronize()
    g.close()
    g2.close()


# --- 9 -------------------------------------------------------------------------------------------------------------------------
def test_context_reuse_nothing_leaks_between_the_calls(crtlib):
    """one context: records bound but unused, then crthip_sequence, crthip_sequence_knobs, crthip_fieldpass -- each equal to the
    same call on a fresh context, and the knob call to the oracle"""
    import torch
    case = SK.case("six")
    other = np.array([(90, 111, 33)] * 6)                   # what is bound: never the knobs of any call below

    def call(g, s, which):
        g.state.zero_()
        g.state[:, crtlib.ST_RN] = 194
        g.out.zero_()
        g._load_field_state(s)
        if which == "sequence":
            g.hue, g.saturation = 25, 13
            g.sequence(s, 30)
        elif which == "knobs":
            g.sequence_knobs(s, _knobs(case))
        else:
            g.hue, g.saturation = 0, 10
            g.fieldpass(s, 24)
        return _snapshot(g)
    order = ["sequence", "knobs", "fieldpass"]
    fresh = []
    for which in order:
        g, s = _make(crtlib, case)
        fresh.append(call(g, s, which))
        g.close()
    _compare(fresh[1], SK.expected(case), "fresh knobs")
    g, s = _make(crtlib, case)
    bound = torch.zeros((6, crtlib.KNOB_REC_INTS), dtype=torch.int32, device="cuda:0")
    recs, env = crtlib.knobs_prepare(g.params(s, 0), other)
    bound.copy_(torch.from_numpy(recs))
    assert g.L.crthip_seq_bind_knobs(g.ctx, C.c_void_p(bound.data_ptr()), C.byref(env)) == 0
    for which, want in zip(order, fresh):
        _same(call(g, s, which), want, "reused context: " + which)
    g.close()


# --- 10 ------------------------------------------------------------------------------------------------------------------------
def _refused(crtlib, g, s, fn, match):
    import torch
    g._load_field_state(s)
    g.out.fill_(91)
    torch.cuda.synchronize()
    state = g.state.clone()
    rc = fn()
    g.synchronize()
    assert rc == -1, rc
    msg = g.L.crthip_error_string(g.ctx)
    assert match in msg, msg
    assert torch.equal(g.state, state) and bool((g.out == 91).all())


def _raw_calls(crtlib, g, s, set_first=None):
    """the two C entry points on g's buffers: call(params, env) -> rc"""
    L = g.L
    vp = C.c_void_p

    def single(p, env, count=None):
        return L.crthip_sequence_knobs(g.ctx, C.byref(p), g.n if count is None else count, vp(s.data.data_ptr()), g._image_stride(s),
                                       vp(g.out.data_ptr()), g.out.stride(0), None, vp(g.state.data_ptr()),
                                       vp(g.knob_recs.data_ptr()), C.byref(env), None)

    def sets(p, env):
        first = (C.c_int * len(set_first))(*set_first)
        return L.crthip_sequence_sets_knobs(g.ctx, C.byref(p), len(set_first) - 1, first, vp(s.data.data_ptr()), g._image_stride(s),
                                            vp(g.out.data_ptr()), g.out.stride(0), None, 0, vp(g.state.data_ptr()),
                                            vp(g.knob_recs.data_ptr()), C.byref(env), None)
    return single, sets


@pytest.mark.parametrize("entry", ["single", "sets"])
def test_refusals_leave_out_and_state_untouched(crtlib, entry):
    case = SK.case("sets")
    n = SK.n_fields(case)
    g, s = _make(crtlib, case)
    p = g.params(s, 0)
    g.upload_knobs(_knobs(case), p)
    single, sets = _raw_calls(crtlib, g, s, case["set_first"])
    call = single if entry == "single" else sets
    good = g._knob_env
    bad_n = crtlib.KnobsEnv.from_buffer_copy(bytes(good))
    bad_n.n = n - 1
    bad_magic = crtlib.KnobsEnv.from_buffer_copy(bytes(good))
    bad_magic.magic = 0
    both = crtlib.Params.from_buffer_copy(bytes(p))
    both.flags |= crtlib.PHOSPHOR_FLAGS["fade"] | crtlib.PHOSPHOR_FLAGS["clear"]
    g.blend = 1                                             # outh 120 + v_fac 0 < CRT_LINES
    blend = g.params(s, 0)
    g.blend = 0
    _refused(crtlib, g, s, lambda: call(p, bad_n), b"number of fields")
    _refused(crtlib, g, s, lambda: call(p, bad_magic), b"crthip_knobs_prepare")
    _refused(crtlib, g, s, lambda: call(both, good), b"phosphor")
    _refused(crtlib, g, s, lambda: call(blend, good), b"blend")
    assert call(p, good) == 0                               # and the same arguments with the right env go through
    g.synchronize()
    assert not bool((g.out == 91).all())
    g.close()


def test_pv1000_is_refused(crtlib):
    case = dict(SK.case("sets"), name="pv1k")
    g, s = _make(crtlib, case)
    p = g.params(s, 0)
    g.upload_knobs(_knobs(case), p)
    single, sets = _raw_calls(crtlib, g, s, case["set_first"])
    _refused(crtlib, g, s, lambda: single(p, g._knob_env), b"PV-1000")
    _refused(crtlib, g, s, lambda: sets(p, g._knob_env), b"PV-1000")
    assert g.L.crthip_seq_bind_knobs(g.ctx, C.c_void_p(g.knob_recs.data_ptr()), C.byref(g._knob_env)) == -1
    assert g.sequence(s, 24) >= 1                           # the uniform entry point still takes the system
    g.synchronize()
    g.close()


def test_vhs_rand_noise_is_refused_in_the_sets_call(crtlib):
    case = dict(SK.case("sets"), name="vhs", seed=7)
    g, s = _make(crtlib, case)
    p = g.params(s, 0)
    g.upload_knobs(_knobs(case), p)
    _, sets = _raw_calls(crtlib, g, s, case["set_first"])
    _refused(crtlib, g, s, lambda: sets(p, g._knob_env), b"rand()")
    g.close()

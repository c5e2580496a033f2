"""The level knobs on the GPU: black point and white point per field (crthip_knobs_prepare7 + crthip_bind_levels) through all six
per-field-knob entry points, bit for bit against the oracle run per field with its seven knobs, or -- sequence mode -- the
reference's serial loop on ONE struct CRT whose knobs are turned between the fields (tests/levels_cases.py): the picture, inp[]
where the entry point exposes it, and hsync / vsync / rn / ccf.  The rows sit on the encoder's fast-path bound (|white|, |ire_base|
8191 | 8192), neighbours on opposite sides, and differ from field to field so that the wavefronts that straddle two fields hold
rows of different levels; no field of any case is excluded (tests/test_levels_cpu.py, and asserted here)."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import fence as F
import knobs_cases as KC
import levels_cases as LV
import seqknobs_cases as SK
from test_gpu_knobs import _compare, _next_parity
from test_gpu_seqknobs import _compare as _seq_compare, _inits, _make as _seq_make, _set_incoming, _snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_knobs_prepare7"), "no crthip_knobs_prepare7 / crthip_bind_levels in this build"
    return crtlib


def _dev_images(images):
    """every image followed by one more readable row (the reference reads row h, crt_ntsc.c:263)"""
    import torch
    a = np.stack(images)
    n, h = a.shape[0], a.shape[1]
    full = torch.zeros((n, h + 1) + a.shape[2:], dtype=torch.uint8, device="cuda:0")
    full[:, :h] = torch.from_numpy(a).to("cuda:0")
    full[:, h] = full[:, h - 1]
    return full[:, :h]


def _make(crtlib, name, geo, n, images=None, shape=1, sig_pad=1, exact=0, fmt=None, ifmt=None, seeds=None, sig_tile=0, pix_tile=0,
          crt_knobs=None, overlap=None):
    g = crtlib.CRT(n, geo["outw"], geo["outh"], crtlib.FMT_BGRA if fmt is None else fmt,
                   name[:4] if name.startswith("ntscfir") else name, device=0)
    g.eq_fir = R.EQ_KERNEL.get(name, 0)
    g.scanlines = 1
    for a, v in (crt_knobs or {}).items():
        setattr(g, a, v)
    g.set_shape(shape)
    g.set_signal_layout(sig_pad)
    g.set_exact(exact)
    g.set_signal_tile(sig_tile)
    g.set_pixel_tile(pix_tile)
    if overlap:
        g.set_overlap(overlap)
    if seeds is not None:
        g.srand(seeds)
    par = [KC.parity(k) for k in range(n)]
    dc = R.Oracle(name).system in R.DOT_CRAWL_SYSTEMS
    s = crtlib.Settings(_dev_images(images if images is not None else LV.default_images(geo, n)),
                        format=crtlib.FMT_BGRA if ifmt is None else ifmt, as_color=1,
                        field=[a for a, _ in par], frame=[b for _, b in par],
                        dot_crawl_offset=[KC.dot_crawl(name, k) for k in range(n)] if dc else 0)
    return g, s


def _batches():
    out = dict(LV.BATCHES)
    out.update({"bound-" + k: v for k, v in LV.bound_batches("ntsc").items()})
    out["corners"] = LV.corner_rows("ntsc")
    return out


def _images_of(cid):
    return LV.corner_images(LV.SMALL) if cid == "corners" else None


def _want(cid):
    return LV.expected(("ntsc", cid, 2), lambda: LV.oracle_fields7("ntsc", LV.SMALL, _batches()[cid], steps=2, images=_images_of(cid)))


# (shape, padded signal lines, set_exact, signal tile, image tile): both kernel shapes x both signal layouts, the exact kernels on
# both shapes, the large signal tiles beside the narrow and the wide image tile, the wide image tile with the small signal tile
CONFIGS = [(1, 1, 0, 0, 0), (1, 0, 0, 0, 0), (2, 1, 0, 0, 0), (2, 0, 0, 0, 0), (1, 1, 1, 0, 0), (2, 1, 1, 0, 0),
           (1, 1, 0, 32, 0), (1, 1, 0, 64, 32), (1, 0, 0, 0, 32)]
BOUND_IDS = sorted(k for k in _batches() if k.startswith("bound-") or k == "corners")
OTHER_IDS = sorted(k for k in _batches() if k not in BOUND_IDS)


def _run_batch(crtlib, cid, shape, sig_pad, exact, sig_tile, pix_tile, steps=2):
    rows = _batches()[cid]
    want = _want(cid)
    g, s = _make(crtlib, "ntsc", LV.SMALL, len(rows), images=_images_of(cid), shape=shape, sig_pad=sig_pad, exact=exact,
                 sig_tile=sig_tile, pix_tile=pix_tile)
    for step in range(steps):
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, step, "%s shape %d pad %d exact %d tiles %d/%d" % (cid, shape, sig_pad, exact, sig_tile, pix_tile))
        _next_parity(s, step)
    assert g._knob_env.pic == 1 and g._levels_bound
    g.close()


@pytest.mark.parametrize("shape,sig_pad,exact,sig_tile,pix_tile", CONFIGS)
@pytest.mark.parametrize("cid", BOUND_IDS)
def test_fieldpass_knobs_at_the_fast_path_bound(crtlib, cid, shape, sig_pad, exact, sig_tile, pix_tile):
    """fields ON the last fast values, and batches with a single field outside (the whole call on the exact kernels): identical
    samples either way, set_exact 0 and 1, both shapes, both layouts, every tile pair; the cube corners at the bound"""
    _run_batch(crtlib, cid, shape, sig_pad, exact, sig_tile, pix_tile)


@pytest.mark.parametrize("shape,sig_pad,exact,sig_tile,pix_tile", [CONFIGS[0], CONFIGS[3], CONFIGS[4], CONFIGS[7]])
@pytest.mark.parametrize("cid", OTHER_IDS)
def test_fieldpass_knobs_straddle_edges_and_the_other_five(crtlib, cid, shape, sig_pad, exact, sig_tile, pix_tile):
    """distinct pairs in one wavefront; white point 0 and negative, black point of both signs and across the decoder's tier bound;
    a clean field in a noisy batch and a contrast above the 24-bit tier with levels of their own"""
    _run_batch(crtlib, cid, shape, sig_pad, exact, sig_tile, pix_tile)


@pytest.mark.parametrize("shape", [1, 2])
def test_noise_free_batch_takes_the_level_kernels_without_noise(crtlib, shape):
    """the batch's largest noise is 0: the LV instantiations without the noise term (also what the clean field of the rand()-noise
    VHS build runs)"""
    rows = [r[:0] + (0,) + r[1:] for r in LV.STRADDLE]
    want = LV.expected(("ntsc", "straddle-clean", 1), lambda: LV.oracle_fields7("ntsc", LV.SMALL, rows, steps=1))
    for exact in (0, 1):
        g, s = _make(crtlib, "ntsc", LV.SMALL, len(rows), shape=shape, exact=exact)
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, 0, "clean shape %d exact %d" % (shape, exact))
        g.close()


@pytest.mark.parametrize("shape", [1, 2])
def test_three_byte_formats(crtlib, shape):
    """RGB in (the bytewise pixel path of k_active) and RGB out, 101 x 77"""
    geo = dict(LV.SMALL, outw=101, outh=77)
    rows = LV.bound_batches("ntsc")["inside"]
    images = [np.ascontiguousarray(KC.image(LV.SMALL, k)[..., 2::-1]) for k in range(len(rows))]      # BGRA -> RGB
    want = LV.expected(("ntsc", "rgb", 1), lambda: LV.oracle_fields7("ntsc", geo, rows, steps=1, fmt=R.FMT_RGB, images=images, ifmt=R.FMT_RGB))
    for exact in (0, 1):
        g, s = _make(crtlib, "ntsc", geo, len(rows), images=images, shape=shape, exact=exact, fmt=crtlib.FMT_RGB, ifmt=crtlib.FMT_RGB)
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, 0, "rgb shape %d exact %d" % (shape, exact))
        g.close()


@pytest.mark.parametrize("name,n", [("vhs", 5), ("vhslcg", 6), ("snes", 5), ("temp", 5), ("nesrgb", 5), ("ntscp0", 4), ("ntscbloom", 6), ("ntscfir7", 4)])
def test_one_case_per_system_and_build(crtlib, name, n):
    """both VHS noise models, the systems with per-line-class carriers, NES-RGB, the other chroma pattern, a bloom build, the FIR
    decoder: level pairs that differ per field, one field on the system's own fast bound"""
    rows = LV.per_system(name, n)
    seeds = [3 + 11 * k for k in range(n)] if name == "vhs" else None
    want = LV.oracle_fields7(name, LV.SMALL, rows, steps=2, seeds=seeds)
    g, s = _make(crtlib, name, LV.SMALL, n, seeds=seeds)
    for step in range(2):
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, step, name)
        _next_parity(s, step)
    g.close()


def test_overlap_chunks_point_every_chunk_at_its_own_records(crtlib):
    """1024 fields in 4 chunks (the smallest batch the chunked path takes), 16 distinct images and rows: fields of every chunk
    against the oracle"""
    n, distinct = 1024, 16
    base = (LV.STRADDLE + LV.COMBINED + LV.bound_batches("ntsc")["inside"])[:distinct]
    rows = [base[k % distinct] for k in range(n)]
    images = [KC.image(LV.SMALL, k % distinct) for k in range(n)]
    check = [0, 1, 255, 256, 257, 511, 512, 700, 767, 768, 1023]
    g, s = _make(crtlib, "ntsc", LV.SMALL, n, images=images, shape=1, overlap=4)
    g.fieldpass_knobs(s, np.array(rows))
    g.synchronize()
    got, rn = g.out.cpu().numpy(), g.get("rn")
    g.close()
    for k in check:
        w = _one_field(rows[k], images[k], k)
        assert rn[k] == w["rn"], k
        np.testing.assert_array_equal(got[k].reshape(-1), w["out"], err_msg="field %d" % k)


def _one_field(row, image, k):
    """the oracle on one field with the parity of batch position k"""
    orc = R.Oracle("ntsc")
    c = orc.new_crt(LV.SMALL["outw"], LV.SMALL["outh"], R.FMT_BGRA)
    c.set("scanlines", 1)
    for a, v in zip(("hue", "saturation", "brightness", "contrast", "black_point", "white_point"), row[1:]):
        c.set(a, v)
    field, frame = KC.parity(k)
    c.settings(np.concatenate([image, image[-1:]], axis=0), format=R.FMT_BGRA, w=LV.SMALL["w"], h=LV.SMALL["h"], as_color=1,
               field=field, frame=frame)
    c.modulate()
    c.demodulate(row[0])
    return dict(out=c.out.copy(), rn=c.get("rn"))


# --- sequence mode ---------------------------------------------------------------------------------------------------------------
def _rows(case, lo=0, hi=None):
    return np.array(case["rows"][lo:hi])


@pytest.mark.parametrize("cid,shape", [("levels", 1), ("levels", 2), ("levels-blend", 0)])
def test_sequence_knobs_levels_turned_mid_video(crtlib, cid, shape):
    """both levels turned between the fields of one running set, with and without blend, against the serial loop on one struct CRT"""
    case = LV.SEQ_CASES[cid]
    g, s = _seq_make(crtlib, case, shape=shape, state_in=SK.incoming(case)[0])
    g.black_point, g.white_point = 33, 7                   # ignored: the records carry them
    g.sequence_knobs(s, _rows(case), out_init=_inits(case)[0])
    snap = _snapshot(g)
    g.close()
    _seq_compare(snap, LV.seq_expected(case), cid)


@pytest.mark.parametrize("cid", ["levels-sets", "levels-sets-blend"])
def test_sequence_sets_knobs_ragged_sets(crtlib, cid):
    """three sets of 1, 4 and 2 fields, per-set incoming states and pictures: the oracle's loop per set"""
    case = LV.SEQ_CASES[cid]
    g, s = _seq_make(crtlib, case)
    for (lo, _), inc in zip(SK.sets_of(case), SK.incoming(case)):
        _set_incoming(crtlib, g, lo, inc)
    g.sequence_sets_knobs(s, _rows(case), case["set_first"], out_init=_inits(case))
    snap = _snapshot(g)
    g.close()
    _seq_compare(snap, LV.seq_expected(case), cid)


def test_phases_with_bound_levels_over_two_shards(crtlib):
    """a video of 6 fields cut into shards of 4 and 2 on two contexts, every shard with ITS slice of both record arrays bound"""
    case = LV.SEQ_CASES["levels"]
    want = LV.seq_expected(case)
    inc = SK.incoming(case)[0]
    prev_pic = _inits(case)[0]
    hv = inc[:2]
    for lo, hi in ((0, 4), (4, 6)):
        g, s = _seq_make(crtlib, case, lo, hi)
        g.seq_bind_knobs(_rows(case, lo, hi))
        assert g._levels_bound
        g.seq_encode(s, 0, lo, inc[2])
        hv = g.seq_sync(*hv)
        g.seq_decode()
        g.seq_weave(out_init=prev_pic)
        _seq_compare(_snapshot(g), want, "shard %d..%d" % (lo, hi), lo=lo)
        prev_pic = g.out[hi - lo - 1].clone()
        g.close()


# --- graphs, refusals, nothing else changes ------------------------------------------------------------------------------------
def test_graph_capture_reads_the_level_records_at_replay(crtlib):
    """capture one call; between the replays BOTH record buffers are rewritten inside the captured bounds (the fields trade places)"""
    import torch
    first = LV.bound_batches("ntsc")["inside"]
    moved = first[::-1]
    want = {0: _want("bound-inside"),
            1: LV.expected("bound-inside-reversed", lambda: LV.oracle_fields7("ntsc", LV.SMALL, moved, steps=1))}
    n = len(first)
    g, s = _make(crtlib, "ntsc", LV.SMALL, n)
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
    for r, which in enumerate((0, 1, 0)):
        env2 = g.upload_knobs(np.array(first if which == 0 else moved), p)
        assert bytes(env2) == bytes(env) and bytes(env2.lenv) == bytes(env.lenv)
        g.state.copy_(state0)
        g.out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _compare(g, want[which], 0, "replay %d" % r, signal=False)
    del graph
    g.close()


def _untouched_after(g, fn, match, fill=91):
    import torch
    g.out.fill_(fill)
    torch.cuda.synchronize()
    state = g.state.clone()
    rc = fn()
    g.synchronize()
    msg = g.L.crthip_error_string(g.ctx)
    assert rc == -1 and match in msg, (rc, msg)
    assert torch.equal(g.state, state) and bool((g.out == fill).all())


def test_refusals_leave_out_and_state_untouched(crtlib):
    import torch
    vp = C.c_void_p
    n = 4
    rows = np.array(LV.STRADDLE[:n])
    g, s = _make(crtlib, "ntsc", LV.SMALL, n)
    L = g.L
    p = g.params(s, 0)
    g._load_field_state(s)
    g.upload_knobs(rows, p)
    env, lenv = g._knob_env, g._knob_env.lenv

    def call(e=env, count=n, params=p):
        return L.crthip_fieldpass_knobs(g.ctx, C.byref(params), count, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()),
                                        g.out.stride(0), vp(g.state.data_ptr()), vp(g.knob_recs.data_ptr()), C.byref(e))

    def bind(le, ptr=None):
        return L.crthip_bind_levels(g.ctx, vp(g.level_recs.data_ptr() if ptr is None else ptr), C.byref(le))
    # a wrong magic, bounds that no prepare call gives, records off their alignment, one of the two arguments missing: the binding
    bad = crtlib.LevelsEnv.from_buffer_copy(bytes(lenv))
    bad.magic ^= 1
    _untouched_after(g, lambda: bind(bad), b"crthip_knobs_prepare7")
    bad = crtlib.LevelsEnv.from_buffer_copy(bytes(lenv))
    bad.white_abs_max = -1
    _untouched_after(g, lambda: bind(bad), b"bounds")
    _untouched_after(g, lambda: bind(lenv, g.level_recs.data_ptr() + 2), b"d_levs")
    _untouched_after(g, lambda: L.crthip_bind_levels(g.ctx, vp(g.level_recs.data_ptr()), None), b"go together")
    # ... the refused bindings left the good one in place; a lenv for another number of fields; an env without picture words
    bad = crtlib.LevelsEnv.from_buffer_copy(bytes(lenv))
    bad.n = n - 1
    assert bind(bad) == 0
    _untouched_after(g, call, b"number of fields")
    single = lambda: L.crthip_sequence_knobs(g.ctx, C.byref(p), n, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()),
                                             g.out.stride(0), None, vp(g.state.data_ptr()), vp(g.knob_recs.data_ptr()), C.byref(env), None)
    _untouched_after(g, single, b"number of fields")
    first = (C.c_int * 3)(0, 1, n)
    sets = lambda: L.crthip_sequence_sets_knobs(g.ctx, C.byref(p), 2, first, vp(s.data.data_ptr()), g._image_stride(s),
                                                vp(g.out.data_ptr()), g.out.stride(0), None, 0, vp(g.state.data_ptr()),
                                                vp(g.knob_recs.data_ptr()), C.byref(env), None)
    _untouched_after(g, sets, b"number of fields")
    assert L.crthip_seq_bind_knobs(g.ctx, vp(g.knob_recs.data_ptr()), C.byref(env)) == 0
    _untouched_after(g, lambda: L.crthip_seq_encode(g.ctx, C.byref(p), n, 0, 194, vp(s.data.data_ptr()), g._image_stride(s),
                                                    vp(g.state.data_ptr())), b"number of fields")
    assert L.crthip_seq_bind_knobs(g.ctx, None, None) == 0
    assert bind(lenv) == 0
    recs3, env3 = crtlib.knobs_prepare(p, rows[:, :3])
    _untouched_after(g, lambda: call(env3), b"crthip_knobs_prepare7")
    # and the good call goes through
    assert call() == 0
    g.synchronize()
    assert not bool((g.out == 91).all())
    g.close()

    # the NES (one sample table per pair), its NES_BORDER build (the border colour is baked into the cached skeleton with one pair)
    # and the PV-1000 (no per-field knobs at all)
    nes_geo = dict(w=256, h=240, outw=320, outh=240)
    for name, geo, match in (("nes", nes_geo, b"512 x 12 table"), ("nesborder", nes_geo, b"NES_BORDER"), ("pv1k", LV.SMALL, b"PV-1000")):
        g = crtlib.CRT(n, geo["outw"], geo["outh"], crtlib.FMT_BGRA, name, device=0)
        if name.startswith("nes"):
            data = torch.zeros((n, 241, 256), dtype=torch.int16, device="cuda:0")[:, :240]
        else:
            data = _dev_images(LV.default_images(geo, n))
        s = crtlib.Settings(data, format=crtlib.FMT_BGRA, as_color=1)
        g._load_field_state(s)

        def knob_call():
            try:
                g.fieldpass_knobs(s, rows)
            except RuntimeError as e:
                assert match.decode() in str(e), str(e)
                return -1
            return 0
        _untouched_after(g, knob_call, match, fill=37)
        g.close()


@pytest.mark.parametrize("shape", [1, 2])
def test_bound_levels_leave_the_other_calls_alone(crtlib, shape):
    """with levels bound: a uniform crthip_fieldpass and crthip_stills give what they give on a fresh context, and so does the (n, 5)
    call that follows (its upload unbinds); all fields at the blob's own levels = the (n, 5) call, byte for byte"""
    import torch
    n = 6
    rows7 = np.array(LV.COMBINED)
    rows5 = rows7[:, :5].copy()
    vp = C.c_void_p

    def reset(g):
        g.state.zero_()
        g.state[:, crtlib.ST_RN] = 194
        g.out.zero_()

    def calls(g, s, bound):
        res = {}
        reset(g)
        g.fieldpass(s, 24)
        g.synchronize()
        res["uniform"] = (g.out.clone(), g.state.clone(), g.fieldpass_signal()[0].clone())
        reset(g)
        g.blend, g.scanlines = 1, 1
        g.stills(s, 0)
        g.synchronize()
        g.blend = 0
        res["stills"] = (g.out.clone(), g.state.clone())
        assert g._levels_bound == bound
        reset(g)
        g.fieldpass_knobs(s, rows5)                         # (the (n, 5) upload unbinds)
        g.synchronize()
        assert not g._levels_bound
        res["five"] = (g.out.clone(), g.state.clone(), g.fieldpass_signal()[0].clone())
        return res
    g, s = _make(crtlib, "ntsc", LV.SMALL, n, shape=shape, crt_knobs=dict(black_point=-4, white_point=93))
    fresh = calls(g, s, False)
    g.close()
    g, s = _make(crtlib, "ntsc", LV.SMALL, n, shape=shape, crt_knobs=dict(black_point=-4, white_point=93))
    g.fieldpass_knobs(s, rows7)
    assert g._levels_bound
    got = calls(g, s, True)
    for k in fresh:
        for a, b in zip(fresh[k], got[k]):
            assert torch.equal(a, b), k
    # all seven uniform and equal to the blob's: the (n, 5) call, byte for byte
    reset(g)
    g.fieldpass_knobs(s, np.concatenate([rows5, np.tile([[-4, 93]], (n, 1))], axis=1))
    g.synchronize()
    assert g._levels_bound
    assert torch.equal(g.out, fresh["five"][0]) and torch.equal(g.state, fresh["five"][1])
    assert torch.equal(g.fieldpass_signal()[0], fresh["five"][2])
    g.close()


@pytest.mark.parametrize("shape", [1, 2])
def test_fenced_record_buffers(crtlib, shape):
    """d_levs, d_recs, d_state and d_out in fenced allocations -- offset bases, a loose out_stride (the records' strides are fixed by
    the contract), two fills: equal payloads, equal to the plain run, and no byte outside a payload changes"""
    import torch
    n = 5
    rows = np.array(LV.STRADDLE)
    vp = C.c_void_p
    g, s = _make(crtlib, "ntsc", LV.SMALL, n, shape=shape)
    g.fieldpass_knobs(s, rows)
    g.synchronize()
    plain_out, plain_state = g.out.cpu().numpy().reshape(n, -1), g.state.cpu().numpy()
    p = g.params(s, 0)
    recs, levs, env, lenv = crtlib.knobs_prepare7(p, rows)
    obytes = LV.SMALL["outw"] * LV.SMALL["outh"] * 4
    pay = []
    for seed in (11, 20261):
        bufs = dict(levs=F.Fenced(n, 16, base_off=4, device="cuda:0", name="d_levs"),
                    recs=F.Fenced(n, 32, base_off=12, device="cuda:0", name="d_recs"),
                    state=F.Fenced(n, 144, base_off=8, device="cuda:0", name="d_state"),
                    out=F.Fenced(n, obytes, stride=obytes + 4 * 37, base_off=16, pitch=LV.SMALL["outw"] * 4, device="cuda:0", name="d_out"))
        g._load_field_state(s)
        g.state[:, crtlib.ST_HSYNC:crtlib.ST_RN] = 0
        g.state[:, crtlib.ST_RN] = 194
        g.state[:, crtlib.ST_CCF:] = 0
        torch.cuda.synchronize()
        pre = dict(levs=bufs["levs"].prefill(seed, levs), recs=bufs["recs"].prefill(seed + 1, recs),
                   state=bufs["state"].prefill(seed + 2, g.state.cpu().numpy()),
                   out=bufs["out"].prefill(seed + 3, np.zeros((n, obytes), dtype=np.uint8)))
        assert g.L.crthip_bind_levels(g.ctx, vp(bufs["levs"].ptr()), C.byref(lenv)) == 0
        rc = g.L.crthip_fieldpass_knobs(g.ctx, C.byref(p), n, vp(s.data.data_ptr()), g._image_stride(s), vp(bufs["out"].ptr()),
                                        bufs["out"].stride, vp(bufs["state"].ptr()), vp(bufs["recs"].ptr()), C.byref(env))
        assert rc == 0, g.L.crthip_error_string(g.ctx)
        g.synchronize()
        bufs["levs"].assert_unchanged(pre["levs"])
        bufs["recs"].assert_unchanged(pre["recs"])
        bufs["state"].assert_fence_intact(pre["state"])
        bufs["out"].assert_fence_intact(pre["out"])
        pay.append((bufs["out"].payloads(), bufs["state"].payloads()))
    g.close()
    for a, b in zip(pay[0], pay[1]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(pay[0][0], plain_out)
    np.testing.assert_array_equal(pay[0][1], plain_state.view(np.uint8).reshape(n, -1))

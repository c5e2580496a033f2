"""The hue knob on the GPU: the ENCODER hue per field (crthip_knobs_prepare8 + crthip_bind_hues) through all six per-field-knob
entry points, bit for bit against the oracle run per field with its eight knobs, or -- sequence mode -- the reference's serial loop
on ONE struct CRT whose knobs are turned between the fields (tests/hues_cases.py): inp[] where the entry point exposes it (the
margins' burst samples and the active video), hsync / vsync / rn / ccf, and the picture.  No field of any case is excluded
(tests/test_hues_cpu.py, and asserted here)."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
import fence as F
import hues_cases as HU
import knobs_cases as KC
import seqknobs_cases as SK
from test_gpu_knobs import _compare, _next_parity
from test_gpu_levels import CONFIGS, _dev_images, _untouched_after
from test_gpu_seqknobs import _compare as _seq_compare, _inits, _make as _seq_make, _set_incoming, _snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_knobs_prepare8"), "no crthip_knobs_prepare8 / crthip_bind_hues in this build"
    return crtlib


def _make(crtlib, name, geo, n, images=None, shape=1, sig_pad=1, exact=0, fmt=None, ifmt=None, seeds=None, sig_tile=0, pix_tile=0,
          crt_knobs=None, overlap=None, hue=0):
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
    s = crtlib.Settings(_dev_images(images if images is not None else HU.default_images(geo, n)),
                        format=crtlib.FMT_BGRA if ifmt is None else ifmt, as_color=1, hue=hue,
                        field=[a for a, _ in par], frame=[b for _, b in par],
                        dot_crawl_offset=[HU.dot_crawl(name, k) for k in range(n)] if dc else 0)
    return g, s


def _want(cid):
    return HU.expected(("ntsc", cid, 2), lambda: HU.oracle_fields8("ntsc", HU.SMALL, HU.BATCHES[cid], steps=2))


@pytest.mark.parametrize("shape,sig_pad,exact,sig_tile,pix_tile", CONFIGS)
@pytest.mark.parametrize("cid", ["a", "b"])
def test_fieldpass_knobs_named_hues(crtlib, cid, shape, sig_pad, exact, sig_tile, pix_tile):
    """0, +-1, 33, 90, 180, 359, +-360, 405, -90, -123: both kernel shapes, both signal layouts, set_exact 0 and 1, every signal and
    pixel tile the level tests parametrise; this CRT's own hue (77) is ignored"""
    rows = HU.BATCHES[cid]
    g, s = _make(crtlib, "ntsc", HU.SMALL, len(rows), shape=shape, sig_pad=sig_pad, exact=exact, sig_tile=sig_tile, pix_tile=pix_tile, hue=77)
    for step in range(2):
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, _want(cid), step, "%s shape %d pad %d exact %d tiles %d/%d" % (cid, shape, sig_pad, exact, sig_tile, pix_tile))
        _next_parity(s, step)
    assert g._hues_bound and g._levels_bound
    g.close()


@pytest.mark.parametrize("shape,sig_pad,exact,sig_tile,pix_tile", [CONFIGS[0], CONFIGS[3], CONFIGS[4], CONFIGS[7]])
@pytest.mark.parametrize("cid", ["straddle", "combined"])
def test_fieldpass_knobs_straddle_and_the_other_seven(crtlib, cid, shape, sig_pad, exact, sig_tile, pix_tile):
    """distinct hues in one wavefront; the hue beside a clean field in a noisy batch, a contrast above the 24-bit tier and levels of
    their own (the COMBINED rows of tests/levels_cases.py)"""
    rows = HU.BATCHES[cid]
    g, s = _make(crtlib, "ntsc", HU.SMALL, len(rows), shape=shape, sig_pad=sig_pad, exact=exact, sig_tile=sig_tile, pix_tile=pix_tile)
    for step in range(2):
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, _want(cid), step, cid)
        _next_parity(s, step)
    g.close()


@pytest.mark.parametrize("sig_pad", [1, 0])
@pytest.mark.parametrize("shape", [1, 2])
def test_noise_free_batch(crtlib, shape, sig_pad):
    """the batch's largest noise is 0: the HU instantiations without the noise term -- margins included (also what the clean field of
    the rand()-noise VHS build runs)"""
    rows = [(0,) + r[1:] for r in HU.BATCHES["straddle"]]
    want = HU.expected(("ntsc", "straddle-clean", 1), lambda: HU.oracle_fields8("ntsc", HU.SMALL, rows, steps=1))
    for exact in (0, 1):
        g, s = _make(crtlib, "ntsc", HU.SMALL, len(rows), shape=shape, sig_pad=sig_pad, exact=exact)
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, 0, "clean shape %d pad %d exact %d" % (shape, sig_pad, exact))
        g.close()


@pytest.mark.parametrize("shape", [1, 2])
def test_three_byte_formats(crtlib, shape):
    """RGB in (the bytewise pixel path of k_active) and RGB out, 101 x 77"""
    geo = dict(HU.SMALL, outw=101, outh=77)
    rows = HU.BATCHES["b"]
    images = [np.ascontiguousarray(KC.image(HU.SMALL, k)[..., 2::-1]) for k in range(len(rows))]      # BGRA -> RGB
    want = HU.expected(("ntsc", "rgb", 1), lambda: HU.oracle_fields8("ntsc", geo, rows, steps=1, fmt=R.FMT_RGB, images=images, ifmt=R.FMT_RGB))
    for exact in (0, 1):
        g, s = _make(crtlib, "ntsc", geo, len(rows), images=images, shape=shape, exact=exact, fmt=crtlib.FMT_RGB, ifmt=crtlib.FMT_RGB)
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, 0, "rgb shape %d exact %d" % (shape, exact))
        g.close()


@pytest.mark.parametrize("sig_pad", [1, 0])
@pytest.mark.parametrize("name,n", [("vhs", 5), ("vhslcg", 6), ("snes", 6), ("temp", 6), ("nesrgb", 6), ("ntscp0", 4), ("ntscbloom", 6), ("ntscfir7", 4)])
def test_one_case_per_system_and_build(crtlib, name, n, sig_pad):
    """both VHS noise models (the rand() build's clean field goes through the noise-free HU kernels, flat lines), the systems with
    per-line-class carriers at dot crawl offsets 0..5 beside negative hues, NES-RGB (only its burst turns), the other chroma
    pattern, a bloom build, the FIR decoder"""
    rows = HU.per_system(name, n)
    seeds = [3 + 11 * k for k in range(n)] if name == "vhs" else None
    want = HU.expected((name, "system", 2), lambda: HU.oracle_fields8(name, HU.SMALL, rows, steps=2, seeds=seeds))
    g, s = _make(crtlib, name, HU.SMALL, n, seeds=seeds, sig_pad=sig_pad)
    for step in range(2):
        g.fieldpass_knobs(s, np.array(rows))
        _compare(g, want, step, name)
        _next_parity(s, step)
    g.close()


@pytest.mark.parametrize("shape", [1, 2])
def test_hue_only_binding(crtlib, shape):
    """hues bound, levels not: p->white and p->ire_base apply (this CRT's black point -4 and white point 93, which the rows repeat
    for the decoder's bright), the HU instantiations without LV"""
    import torch
    vp = C.c_void_p
    rows = [r[:5] + (-4, 93) + r[7:] for r in HU.BATCHES["straddle"]]
    n = len(rows)
    want = HU.expected(("ntsc", "hue-only", 1), lambda: HU.oracle_fields8("ntsc", HU.SMALL, rows, steps=1))
    for noisy in (True, False):
        use = rows if noisy else [(0,) + r[1:] for r in rows]
        w = want if noisy else HU.expected(("ntsc", "hue-only-clean", 1), lambda: HU.oracle_fields8("ntsc", HU.SMALL, use, steps=1))
        g, s = _make(crtlib, "ntsc", HU.SMALL, n, shape=shape, crt_knobs=dict(black_point=-4, white_point=93))
        p = g.params(s, 0)
        g._load_field_state(s)
        g.upload_knobs(np.array(use), p)
        assert g.L.crthip_bind_levels(g.ctx, None, None) == 0
        rc = g.L.crthip_fieldpass_knobs(g.ctx, C.byref(p), n, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()),
                                        g.out.stride(0), vp(g.state.data_ptr()), vp(g.knob_recs.data_ptr()), C.byref(g._knob_env))
        assert rc == 0, g.L.crthip_error_string(g.ctx)
        _compare(g, w, 0, "hue only shape %d noisy %d" % (shape, noisy))
        g.close()
    del torch


def _one_field(row, image, k):
    """the oracle on one field with the parity of batch position k"""
    orc = R.Oracle("ntsc")
    c = orc.new_crt(HU.SMALL["outw"], HU.SMALL["outh"], R.FMT_BGRA)
    c.set("scanlines", 1)
    for a, v in zip(("hue", "saturation", "brightness", "contrast", "black_point", "white_point"), row[1:7]):
        c.set(a, v)
    field, frame = KC.parity(k)
    c.settings(np.concatenate([image, image[-1:]], axis=0), format=R.FMT_BGRA, w=HU.SMALL["w"], h=HU.SMALL["h"], as_color=1,
               field=field, frame=frame)
    c.sset("hue", row[7])
    c.modulate()
    c.demodulate(row[0])
    return dict(out=c.out.copy(), rn=c.get("rn"), ccf=c.ccf.copy())


def test_overlap_chunks_point_every_chunk_at_its_own_records(crtlib):
    """1024 fields in 4 chunks (the smallest batch the chunked path takes), 16 distinct images and rows -- fields of every chunk
    against the oracle: every chunk reads its own slice of all three record arrays"""
    n, distinct = 1024, 16
    base = (HU.BATCHES["straddle"] + HU.BATCHES["combined"] + HU.BATCHES["b"])[:distinct]
    rows = [base[(k + k // 256) % distinct] for k in range(n)]
    images = [KC.image(HU.SMALL, k % distinct) for k in range(n)]
    check = [0, 1, 255, 256, 257, 511, 512, 700, 767, 768, 1023]
    g, s = _make(crtlib, "ntsc", HU.SMALL, n, images=images, shape=1, overlap=4)
    g.fieldpass_knobs(s, np.array(rows))
    g.synchronize()
    got, rn, ccf = g.out.cpu().numpy(), g.get("rn"), g.ccf
    g.close()
    for k in check:
        w = _one_field(rows[k], images[k], k)
        assert rn[k] == w["rn"], k
        np.testing.assert_array_equal(ccf[k, :w["ccf"].shape[0], :w["ccf"].shape[1]], w["ccf"], err_msg="field %d ccf" % k)
        np.testing.assert_array_equal(got[k].reshape(-1), w["out"], err_msg="field %d" % k)


# --- sequence mode ---------------------------------------------------------------------------------------------------------------
def _rows(case, lo=0, hi=None):
    return np.array(case["rows"][lo:hi])


@pytest.mark.parametrize("cid,shape", [("hues", 1), ("hues", 2), ("hues-blend", 0), ("hues-fade", 0)])
def test_sequence_knobs_hue_turned_mid_video(crtlib, cid, shape):
    """the hue turned between the fields of one running set, with and without blend, with a phosphor flag, against the serial loop
    on one struct CRT: sequence mode needs no arithmetic of its own for it -- confirmed here, not argued"""
    case = HU.SEQ_CASES[cid]
    g, s = _seq_make(crtlib, case, shape=shape, state_in=SK.incoming(case)[0])
    g.sequence_knobs(s, _rows(case), out_init=_inits(case)[0])
    snap = _snapshot(g)
    assert g._hues_bound
    g.close()
    _seq_compare(snap, HU.seq_expected(case), cid)


@pytest.mark.parametrize("cid", ["hues-sets", "hues-sets-blend"])
def test_sequence_sets_knobs_ragged_sets(crtlib, cid):
    """three sets of 1, 4 and 2 fields, per-set incoming states and pictures: the oracle's loop per set"""
    case = HU.SEQ_CASES[cid]
    g, s = _seq_make(crtlib, case)
    for (lo, _), inc in zip(SK.sets_of(case), SK.incoming(case)):
        _set_incoming(crtlib, g, lo, inc)
    g.sequence_sets_knobs(s, _rows(case), case["set_first"], out_init=_inits(case))
    snap = _snapshot(g)
    g.close()
    _seq_compare(snap, HU.seq_expected(case), cid)


def test_phases_with_bound_hues_over_two_shards(crtlib):
    """a video of 6 fields cut into shards of 4 and 2 on two contexts, every shard with ITS slice of all three record arrays bound"""
    case = HU.SEQ_CASES["hues"]
    want = HU.seq_expected(case)
    inc = SK.incoming(case)[0]
    prev_pic = _inits(case)[0]
    hv = inc[:2]
    for lo, hi in ((0, 4), (4, 6)):
        g, s = _seq_make(crtlib, case, lo, hi)
        g.seq_bind_knobs(_rows(case, lo, hi))
        assert g._levels_bound and g._hues_bound
        g.seq_encode(s, 0, lo, inc[2])
        hv = g.seq_sync(*hv)
        g.seq_decode()
        g.seq_weave(out_init=prev_pic)
        _seq_compare(_snapshot(g), want, "shard %d..%d" % (lo, hi), lo=lo)
        prev_pic = g.out[hi - lo - 1].clone()
        g.close()


# --- graphs, refusals, nothing else changes ------------------------------------------------------------------------------------
def test_graph_capture_reads_the_hue_records_at_replay(crtlib):
    """capture one call; between the replays all three record buffers are rewritten (the fields trade places).  The cached skeleton
    is neither rebuilt nor invalidated by any of it: crthip_table_generation stays where the first uniform call left it"""
    import torch
    first = HU.BATCHES["b"]
    moved = first[::-1]
    want = {0: _want("b"), 1: HU.expected("b-reversed", lambda: HU.oracle_fields8("ntsc", HU.SMALL, moved, steps=1))}
    n = len(first)
    g, s = _make(crtlib, "ntsc", HU.SMALL, n)
    g.reserve(n)
    g.fieldpass(s, 24)                                     # a uniform call builds the skeleton variants (this CRT's hue: 0)
    g.synchronize()
    gen = g.L.crthip_table_generation(g.ctx)
    side = torch.cuda.Stream()
    g.use_stream(side)
    p = g.params(s, 0)
    g._load_field_state(s)
    g.state[:, crtlib.ST_HSYNC:crtlib.ST_RN] = 0
    g.state[:, crtlib.ST_RN] = 194
    g.state[:, crtlib.ST_CCF:] = 0
    torch.cuda.synchronize()
    state0 = g.state.clone()
    env = g.upload_knobs(np.array(first), p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g.fieldpass_knobs(s, None, params=p)
    for r, which in enumerate((0, 1, 0)):
        env2 = g.upload_knobs(np.array(first if which == 0 else moved), p)
        assert bytes(env2) == bytes(env) and bytes(env2.henv) == bytes(env.henv)
        g.state.copy_(state0)
        g.out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _compare(g, want[which], 0, "replay %d" % r, signal=False)
        assert g.L.crthip_table_generation(g.ctx) == gen
    del graph
    g.use_stream(None)
    g._load_field_state(s)
    g.fieldpass(s, 24)                                     # ... and the uniform call after it finds its skeleton as it left it
    g.synchronize()
    assert g.L.crthip_table_generation(g.ctx) == gen
    g.close()


def test_refusals_leave_out_and_state_untouched(crtlib):
    import torch
    vp = C.c_void_p
    n = 4
    rows = np.array(HU.BATCHES["straddle"][:n])
    g, s = _make(crtlib, "ntsc", HU.SMALL, n)
    L = g.L
    p = g.params(s, 0)
    g._load_field_state(s)
    g.upload_knobs(rows, p)
    env, henv = g._knob_env, g._knob_env.henv

    def call(e=env, count=n, params=p):
        return L.crthip_fieldpass_knobs(g.ctx, C.byref(params), count, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()),
                                        g.out.stride(0), vp(g.state.data_ptr()), vp(g.knob_recs.data_ptr()), C.byref(e))

    def bind(he, ptr=None):
        return L.crthip_bind_hues(g.ctx, vp(g.hue_recs.data_ptr() if ptr is None else ptr), C.byref(he))
    bad = crtlib.HuesEnv.from_buffer_copy(bytes(henv))
    bad.magic ^= 1
    _untouched_after(g, lambda: bind(bad), b"crthip_knobs_prepare8")
    bad = crtlib.HuesEnv.from_buffer_copy(bytes(henv))
    bad.n = 0
    _untouched_after(g, lambda: bind(bad), b"bounds")
    _untouched_after(g, lambda: bind(henv, g.hue_recs.data_ptr() + 2), b"d_hues")
    _untouched_after(g, lambda: L.crthip_bind_hues(g.ctx, vp(g.hue_recs.data_ptr()), None), b"go together")
    # ... the refused bindings left the good one in place; a henv for another number of fields: all six entry points
    bad = crtlib.HuesEnv.from_buffer_copy(bytes(henv))
    bad.n = n - 1
    assert bind(bad) == 0
    _untouched_after(g, call, b"hues: the bound crthip_hues_env")
    single = lambda: L.crthip_sequence_knobs(g.ctx, C.byref(p), n, vp(s.data.data_ptr()), g._image_stride(s), vp(g.out.data_ptr()),
                                             g.out.stride(0), None, vp(g.state.data_ptr()), vp(g.knob_recs.data_ptr()), C.byref(env), None)
    _untouched_after(g, single, b"hues: the bound crthip_hues_env")
    first = (C.c_int * 3)(0, 1, n)
    sets = lambda: L.crthip_sequence_sets_knobs(g.ctx, C.byref(p), 2, first, vp(s.data.data_ptr()), g._image_stride(s),
                                                vp(g.out.data_ptr()), g.out.stride(0), None, 0, vp(g.state.data_ptr()),
                                                vp(g.knob_recs.data_ptr()), C.byref(env), None)
    _untouched_after(g, sets, b"hues: the bound crthip_hues_env")
    assert L.crthip_seq_bind_knobs(g.ctx, vp(g.knob_recs.data_ptr()), C.byref(env)) == 0
    _untouched_after(g, lambda: L.crthip_seq_encode(g.ctx, C.byref(p), n, 0, 194, vp(s.data.data_ptr()), g._image_stride(s),
                                                    vp(g.state.data_ptr())), b"hues: the bound crthip_hues_env")
    assert L.crthip_seq_bind_knobs(g.ctx, None, None) == 0
    assert bind(henv) == 0
    assert call() == 0                                     # and the good call goes through
    g.synchronize()
    assert not bool((g.out == 91).all())
    g.close()

    # the NES (its PPU encoder has no per-field instantiation) and the PV-1000 (no per-field knobs at all).  The NES refuses the
    # (n, 8) array on the host already (crthip_knobs_prepare8); records bound by hand are refused by the call
    nes_geo = dict(w=256, h=240, outw=320, outh=240)
    g = crtlib.CRT(n, nes_geo["outw"], nes_geo["outh"], crtlib.FMT_BGRA, "nes", device=0)
    s = crtlib.Settings(torch.zeros((n, 241, 256), dtype=torch.int16, device="cuda:0")[:, :240], format=crtlib.FMT_BGRA, as_color=1)
    g._load_field_state(s)
    with pytest.raises(ValueError):
        g.fieldpass_knobs(s, rows)
    hues = torch.zeros((n, crtlib.HUE_REC_INTS), dtype=torch.int32, device="cuda:0")
    assert g.L.crthip_bind_hues(g.ctx, vp(hues.data_ptr()), C.byref(henv)) == 0

    def nes_call():
        try:
            g.fieldpass_knobs(s, rows[:, :3])
        except RuntimeError as e:
            assert "hues: the NES encoder" in str(e), str(e)
            return -1
        return 0
    _untouched_after(g, nes_call, b"hues: the NES encoder", fill=37)
    g.close()
    g = crtlib.CRT(n, HU.SMALL["outw"], HU.SMALL["outh"], crtlib.FMT_BGRA, "pv1k", device=0)
    s = crtlib.Settings(_dev_images(HU.default_images(HU.SMALL, n)), format=crtlib.FMT_BGRA, as_color=1)
    g._load_field_state(s)

    def pv_call():
        try:
            g.fieldpass_knobs(s, rows)
        except RuntimeError as e:
            assert "PV-1000" in str(e), str(e)
            return -1
        return 0
    _untouched_after(g, pv_call, b"PV-1000", fill=37)
    g.close()


@pytest.mark.parametrize("shape", [1, 2])
def test_bound_hues_leave_the_other_calls_alone(crtlib, shape):
    """with hues bound: a uniform crthip_fieldpass, crthip_stills and the (n, 3) / (n, 5) / (n, 7) calls give what they give on a
    context that never bound one (their uploads unbind); a batch whose eight columns are all the blob's own values = crthip_fieldpass,
    byte for byte (signal, state, picture)"""
    import torch
    n = 6
    rows8 = np.array(HU.BATCHES["combined"])
    own = dict(black_point=-4, white_point=93, hue=15, saturation=12, brightness=3, contrast=170)

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
        assert g._hues_bound == bound
        for width in (7, 5, 3):
            reset(g)
            g.fieldpass_knobs(s, rows8[:, :width].copy())  # (the upload unbinds the hues)
            g.synchronize()
            assert not g._hues_bound
            res[width] = (g.out.clone(), g.state.clone(), g.fieldpass_signal()[0].clone())
        return res
    g, s = _make(crtlib, "ntsc", HU.SMALL, n, shape=shape, crt_knobs=own, hue=-50)
    fresh = calls(g, s, False)
    g.close()
    g, s = _make(crtlib, "ntsc", HU.SMALL, n, shape=shape, crt_knobs=own, hue=-50)
    g.fieldpass_knobs(s, rows8)
    assert g._hues_bound
    got = calls(g, s, True)
    for k in fresh:
        for a, b in zip(fresh[k], got[k]):
            assert torch.equal(a, b), k
    # all eight uniform and equal to the blob's: crthip_fieldpass, byte for byte
    reset(g)
    g.fieldpass_knobs(s, np.tile([[24, own["hue"], own["saturation"], own["brightness"], own["contrast"], -4, 93, -50]], (n, 1)))
    g.synchronize()
    assert g._hues_bound and g._levels_bound
    assert torch.equal(g.out, fresh["uniform"][0]) and torch.equal(g.state, fresh["uniform"][1])
    assert torch.equal(g.fieldpass_signal()[0], fresh["uniform"][2])
    g.close()


@pytest.mark.parametrize("shape", [1, 2])
def test_fenced_record_buffers(crtlib, shape):
    """d_hues, d_levs, d_recs, d_state and d_out in fenced allocations -- offset bases, a loose out_stride (the records' strides are
    fixed by the contract), two fills: equal payloads, equal to the plain run, and no byte outside a payload changes"""
    import torch
    n = 5
    rows = np.array(HU.BATCHES["straddle"])
    vp = C.c_void_p
    g, s = _make(crtlib, "ntsc", HU.SMALL, n, shape=shape)
    g.fieldpass_knobs(s, rows)
    g.synchronize()
    plain_out, plain_state = g.out.cpu().numpy().reshape(n, -1), g.state.cpu().numpy()
    p = g.params(s, 0)
    recs, levs, hues, env, lenv, henv = crtlib.knobs_prepare8(p, rows)
    obytes = HU.SMALL["outw"] * HU.SMALL["outh"] * 4
    pay = []
    for seed in (11, 20261):
        bufs = dict(hues=F.Fenced(n, 640, base_off=20, device="cuda:0", name="d_hues"),
                    levs=F.Fenced(n, 16, base_off=4, device="cuda:0", name="d_levs"),
                    recs=F.Fenced(n, 32, base_off=12, device="cuda:0", name="d_recs"),
                    state=F.Fenced(n, 144, base_off=8, device="cuda:0", name="d_state"),
                    out=F.Fenced(n, obytes, stride=obytes + 4 * 37, base_off=16, pitch=HU.SMALL["outw"] * 4, device="cuda:0", name="d_out"))
        g._load_field_state(s)
        g.state[:, crtlib.ST_HSYNC:crtlib.ST_RN] = 0
        g.state[:, crtlib.ST_RN] = 194
        g.state[:, crtlib.ST_CCF:] = 0
        torch.cuda.synchronize()
        pre = dict(hues=bufs["hues"].prefill(seed + 4, hues), levs=bufs["levs"].prefill(seed, levs),
                   recs=bufs["recs"].prefill(seed + 1, recs), state=bufs["state"].prefill(seed + 2, g.state.cpu().numpy()),
                   out=bufs["out"].prefill(seed + 3, np.zeros((n, obytes), dtype=np.uint8)))
        assert g.L.crthip_bind_levels(g.ctx, vp(bufs["levs"].ptr()), C.byref(lenv)) == 0
        assert g.L.crthip_bind_hues(g.ctx, vp(bufs["hues"].ptr()), C.byref(henv)) == 0
        rc = g.L.crthip_fieldpass_knobs(g.ctx, C.byref(p), n, vp(s.data.data_ptr()), g._image_stride(s), vp(bufs["out"].ptr()),
                                        bufs["out"].stride, vp(bufs["state"].ptr()), vp(bufs["recs"].ptr()), C.byref(env))
        assert rc == 0, g.L.crthip_error_string(g.ctx)
        g.synchronize()
        bufs["hues"].assert_unchanged(pre["hues"])
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

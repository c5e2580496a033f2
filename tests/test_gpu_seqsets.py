"""GPU parity of the many-sets sequence mode (crthip_sequence_sets / CRT.sequence_sets, include/crt_hip.h): n_sets independent
television sets, each a run of consecutive fields of the batch, in one call.  Every picture and every (hsync, vsync, rn) of every
field against the oracle running the reference's serial loop once per set (tests/seqsets_cases.py; the compiled reference runs the
same loops in tests/test_seqsets_cpu.py, which also shows that every case can tell a set boundary from none).  Bit-exact."""
import ctypes as C

import numpy as np
import pytest

import crtref as R
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


def _settings(crtlib, case, lo=0, hi=None):
    """device settings of fields [lo, hi) of the case (every image followed by a readable row: crt_ntsc.c:263)"""
    import torch
    hi = SC.n_fields(case) if hi is None else hi
    fr, par, dco = SC.frames(case)[lo:hi], SC.parities(case)[lo:hi], SC.dot_crawl(case)[lo:hi]
    n = hi - lo
    sysid = R.SYSTEMS[case["name"]][0]
    if sysid == R.SYS_NES:
        full = torch.zeros((n, 241, 256), dtype=torch.int16, device="cuda:0")
        full[:, :240] = torch.from_numpy(fr.astype(np.int16)).to("cuda:0")
        return crtlib.Settings(full[:, :240], hue=0, dot_crawl_offset=dco)
    h = fr.shape[1]
    full = torch.zeros((n, h + 1) + tuple(fr.shape[2:]), dtype=torch.uint8, device="cuda:0")
    full[:, :h] = _to_dev(fr)
    full[:, h] = full[:, h - 1]
    return crtlib.Settings(full[:, :h], format=crtlib.FMT_BGRA, field=[a for a, _ in par], frame=[b for _, b in par],
                           dot_crawl_offset=dco if sysid in R.DOT_CRAWL_SYSTEMS else 0)


def _context(crtlib, case, n, shape):
    g = crtlib.CRT(n, case["outw"], case["outh"], case["ofmt"], case["name"], device=0)
    for k, v in case["knobs"].items():
        setattr(g, k, v)
    g.phosphor = case["mode"]
    g.set_shape(shape)
    return g


def _run_sets(crtlib, case, shape):
    """one CRT.sequence_sets call over the whole case -> (pictures, [(hsync, vsync, rn)], passes)"""
    n = SC.n_fields(case)
    g = _context(crtlib, case, n, shape)
    for s, (lo, _hi) in enumerate(SC.sets_of(case)):
        hs, vs, rn = SC.incoming(case)[s]
        g.state[lo, crtlib.ST_HSYNC] = hs
        g.state[lo, crtlib.ST_VSYNC] = vs
        g.state[lo, crtlib.ST_RN] = rn if rn < 2 ** 31 else rn - 2 ** 32
    init = SC.init_pictures(case)
    passes = g.sequence_sets(_settings(crtlib, case), case["noise"], case["set_first"], out_init=None if init is None else _to_dev(init))
    g.synchronize()
    out = g.out.cpu().numpy()
    st = list(zip(g.get("hsync"), g.get("vsync"), g.get("rn")))
    g.close()
    return out, st, passes


def _compare(case, want, out, st, what):
    for k in range(SC.n_fields(case)):
        o, hs, vs, rn = want[k]
        assert st[k] == (hs, vs, rn), "%s: state after field %d" % (what, k)
        np.testing.assert_array_equal(out[k].reshape(-1), o, err_msg="%s: picture of field %d" % (what, k))


@pytest.mark.parametrize("cid", SC.CASE_IDS)
def test_sequence_sets_equals_the_serial_loop_per_set(crtlib, cid):
    """ragged and uniform sets; ntsc / nes / pv1k / bloom / vhslcg; BGRA, RGB, ARGB; scanlines 0 and 1; v_fac 240; blend 0 and 1;
    keep / fade / clear; the kernel shapes; the wide-run decoder; out_init NULL, shared and per set; a set longer than the phosphor
    depth behind a short one"""
    case = SC.case(cid)
    want = SC.expected(case)
    longest = max(hi - lo for lo, hi in SC.sets_of(case))
    for shape in case["shapes"]:
        out, st, passes = _run_sets(crtlib, case, shape)
        print("%s shape %d: %d passes" % (cid, shape, passes))
        assert 1 <= passes <= longest + 1
        _compare(case, want, out, st, "%s shape %d" % (cid, shape))


def test_sets_that_need_different_numbers_of_passes(crtlib):
    """noise 120: the sets' sync chains converge after different numbers of passes (counted by the oracle, set by set); the joint
    fixed point runs as many as the slowest set needs and every set's result is still exact"""
    case = SC.case(SC.NOISY)
    want = SC.expected(case)
    per_set = [SC.sync_passes_of_set(case, s, want) for s in range(len(SC.sets_of(case)))]
    assert len(set(per_set)) > 1, per_set
    out, st, passes = _run_sets(crtlib, case, 0)
    print("passes per set (oracle): %s, joint: %d" % (per_set, passes))
    assert passes == max(per_set)
    assert passes <= max(hi - lo for lo, hi in SC.sets_of(case)) + 1
    _compare(case, want, out, st, SC.NOISY)


@pytest.mark.parametrize("cid", ["ntsc-keep-shapes", "ntsc-rgb-blend-duprows", "ntsc-small-argb-fade-noise120"])
def test_one_set_equals_sequence(crtlib, cid):
    """n_sets = 1: the oracle's pictures, and (library against library, as an extra) what CRT.sequence gives on the same inputs"""
    case = dict(SC.case(cid))
    n = 7
    case["set_first"] = [0, n]
    want = SC.expected(case)
    out, st, passes = _run_sets(crtlib, case, 0)
    _compare(case, want, out, st, cid + " as one set")
    g = _context(crtlib, case, n, 0)
    hs, vs, rn = SC.incoming(case)[0]
    g.state[0, crtlib.ST_HSYNC], g.state[0, crtlib.ST_VSYNC], g.state[0, crtlib.ST_RN] = hs, vs, rn
    p1 = g.sequence(_settings(crtlib, case), case["noise"], out_init=_to_dev(SC.init_of_set(case, SC.init_pictures(case), 0)))
    g.synchronize()
    assert p1 == passes
    np.testing.assert_array_equal(g.out.cpu().numpy(), out)
    assert list(zip(g.get("hsync"), g.get("vsync"), g.get("rn"))) == st
    g.close()


def _raw_call(crtlib, g, p, s, set_first, n_sets=None):
    first = (C.c_int * len(set_first))(*set_first)
    return g.L.crthip_sequence_sets(g.ctx, C.byref(p), len(set_first) - 1 if n_sets is None else n_sets, first,
                                    C.c_void_p(s.data.data_ptr()), g._image_stride(s), C.c_void_p(g.out.data_ptr()), g.out.stride(0),
                                    None, 0, C.c_void_p(g.state.data_ptr()), None)


def test_refused_set_tables(crtlib):
    """set_first[0] != 0, an empty set, a descending table, no sets: CRTHIP_E_ARG with a message, d_out untouched"""
    case = dict(SC.case("ntsc-keep-shapes"))
    case["set_first"] = [0, 6]
    g = _context(crtlib, case, 6, 0)
    s = _settings(crtlib, case)
    p = g.params(s, 24)
    g.out.fill_(0x5a)
    for bad in ([1, 6], [0, 3, 3, 6], [0, 4, 2, 6], [0, 0, 6]):
        assert _raw_call(crtlib, g, p, s, bad) == -1, bad
        assert b"set_first" in g.L.crthip_error_string(g.ctx)
    assert _raw_call(crtlib, g, p, s, [0, 6], n_sets=0) == -1
    assert g.L.crthip_sequence_sets(g.ctx, C.byref(p), 1, None, C.c_void_p(s.data.data_ptr()), g._image_stride(s),
                                    C.c_void_p(g.out.data_ptr()), g.out.stride(0), None, 0, C.c_void_p(g.state.data_ptr()), None) == -1
    with pytest.raises(ValueError):
        g.sequence_sets(s, 24, [0, 5])                     # does not cover the batch
    with pytest.raises(RuntimeError):
        g.sequence_sets(s, 24, [0, 3, 3, 6])
    g.synchronize()
    assert bool((g.out == 0x5a).all())
    assert _raw_call(crtlib, g, p, s, [0, 2, 6]) == 0      # and the context still works
    g.synchronize()
    assert not bool((g.out == 0x5a).all())
    g.close()


@pytest.mark.parametrize("name,draw", [("vhs", 0), ("vhslcg", 1)])
def test_refused_vhs_rand_streams(crtlib, name, draw):
    """the VHS build with rand() noise, and CRTHIP_F_VHS_DRAW_ABERRATION (which draws from that stream): CRTHIP_E_ARG, d_out untouched"""
    case = dict(SC.case("vhslcg-keep"))
    case["name"] = name
    case["set_first"] = [0, 2, 4]
    g = _context(crtlib, case, 4, 0)
    s = _settings(crtlib, case)
    s.draw_aberration = draw
    p = g.params(s, 24)
    assert bool(p.flags & crtlib.F_VHS_DRAW_ABERRATION) == bool(draw)
    g.out.fill_(0x5a)
    assert _raw_call(crtlib, g, p, s, [0, 2, 4]) == -1
    assert b"rand()" in g.L.crthip_error_string(g.ctx)
    with pytest.raises(RuntimeError):
        g.sequence_sets(s, 24, [0, 2, 4])
    g.synchronize()
    assert bool((g.out == 0x5a).all())
    g.close()

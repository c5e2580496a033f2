"""GPU parity of the many-sets sequence mode on the stock VHS build (crthip_sequence_sets / _sets_knobs with CRTHIP_F_VHS_SET_STREAMS;
CRT.sequence_sets(..., vhs_streams=True)): every set owns one rand() stream.  Every picture, every (hsync, vsync, rn), the aberration
heights and where every set's generator stands afterwards, against the oracle running the reference's serial loop once per set under
srand(the set's seed) (tests/vhs_sets_cases.py; tests/test_vhs_sets_cpu.py runs the compiled reference on the same loops and shows
that every case can tell per-set streams from one stream).  Bit-exact.  With do_aberration the last 12 output rows are outside the
contract (vhs_sets_cases.ABERRATION_ROWS, as in test_gpu_parity.py); nothing else is excluded."""
import ctypes as C

import numpy as np
import pytest

import vhs_sets_cases as VC

pytestmark = pytest.mark.gpu

_EXPECTED = {}


def _expected(case):
    """the oracle's loops, once per case; read-only"""
    if case["id"] not in _EXPECTED:
        _EXPECTED[case["id"]] = VC.expected(case)
    return _EXPECTED[case["id"]]


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    assert crtlib.F_VHS_SET_STREAMS == 0x20000
    return crtlib


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _settings(crtlib, case, lo=0, hi=None):
    """device settings of fields [lo, hi) of the case (every image followed by a readable row: crt_ntsc.c:263)"""
    import torch
    hi = VC.n_fields(case) if hi is None else hi
    fr, par = VC.frames(case)[lo:hi], VC.parities(case)[lo:hi]
    full = torch.zeros((hi - lo, VC.H + 1, VC.W, 4), dtype=torch.uint8, device="cuda:0")
    full[:, :VC.H] = _to_dev(fr)
    full[:, VC.H] = full[:, VC.H - 1]
    s = crtlib.Settings(full[:, :VC.H], format=crtlib.FMT_BGRA, field=[a for a, _ in par], frame=[b for _, b in par])
    s.draw_aberration = case["aberration"]
    return s


def _context(crtlib, case, n, shape):
    g = crtlib.CRT(n, VC.OUTW, VC.OUTH, crtlib.FMT_BGRA, case["name"], device=0)
    for k, v in case["knobs"].items():
        setattr(g, k, v)
    g.phosphor = case["mode"]
    g.set_shape(shape)
    return g


def _load_sets(crtlib, g, case):
    """every set's incoming pair and seed at its first field; everywhere else values that must not matter (the incoming rn too)"""
    n = VC.n_fields(case)
    field_seeds = [900 + k for k in range(n)]
    g.state[:, crtlib.ST_HSYNC] = -77
    g.state[:, crtlib.ST_VSYNC] = 9
    for s, (lo, _hi) in enumerate(VC.sets_of(case)):
        g.state[lo, crtlib.ST_HSYNC], g.state[lo, crtlib.ST_VSYNC] = VC.incoming(case)[s]
        g.state[lo, crtlib.ST_RN] = VC.RN_IN[s % 4]
        field_seeds[lo] = VC.seeds(case)[s]
    g.srand(field_seeds)


def _init(case):
    init = VC.init_pictures(case)
    return None if init is None else _to_dev(init)


def _snapshot(crtlib, g):
    g.synchronize()
    st = g.state.cpu().numpy()
    return dict(out=g.out.cpu().numpy(), st=[tuple(int(v) for v in r) for r in st[:, [crtlib.ST_HSYNC, crtlib.ST_VSYNC, crtlib.ST_RN]]],
                aux=[int(v) for v in st[:, crtlib.ST_AUX]], hist=g.vhs_hist.cpu().numpy().view(np.uint32)[:, :31].copy())


def _run_sets(crtlib, case, shape=0, g=None):
    """one sets call with per-set streams over the whole case -> (snapshot, passes)"""
    own = g is None
    g = g or _context(crtlib, case, VC.n_fields(case), shape)
    _load_sets(crtlib, g, case)
    s = _settings(crtlib, case)
    if case["triples"]:
        passes = g.sequence_sets_knobs(s, np.array(case["triples"]), case["set_first"], out_init=_init(case), vhs_streams=True)
    else:
        passes = g.sequence_sets(s, case["noise"], case["set_first"], out_init=_init(case), vhs_streams=True)
    snap = _snapshot(crtlib, g)
    if own:
        g.close()
    return snap, passes


def _compare(case, want, snap, what):
    keep = VC.kept_rows(case)
    for k in range(VC.n_fields(case)):
        o, hs, vs, rn, aux = want[k]
        assert snap["st"][k] == (hs, vs, rn), "%s: (hsync, vsync, rn) after field %d" % (what, k)
        if case["aberration"]:
            assert snap["aux"][k] == aux, "%s: aberration height of field %d" % (what, k)
        np.testing.assert_array_equal(snap["out"][k][:keep], o.reshape(VC.OUTH, VC.OUTW, 4)[:keep], err_msg="%s: picture of field %d" % (what, k))


def _next_rand(hist_row):
    return ((int(hist_row[0]) + int(hist_row[28])) & 0xffffffff) >> 1


def _same(a, b, what, rows=VC.OUTH, lo=0, hi=None):
    """snapshot a, fields [lo, hi), against the whole snapshot b, byte for byte"""
    hi = len(a["st"]) if hi is None else hi
    assert a["st"][lo:hi] == b["st"], what + ": states"
    assert a["aux"][lo:hi] == b["aux"], what + ": aux"
    np.testing.assert_array_equal(a["hist"][lo:hi], b["hist"], err_msg=what + ": histories")
    np.testing.assert_array_equal(a["out"][lo:hi, :rows], b["out"][:, :rows], err_msg=what + ": pictures")


# --- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", VC.CASE_IDS)
def test_sets_with_their_own_streams_equal_the_serial_loop_per_set(crtlib, cid):
    """noise 0 and 12; aberration 0 and 1; keep / fade / clear; blend 0 and 1; kernel shapes 0, 1 and 2; out_init NULL, shared and per
    set; sets of lengths 1, 3, 5, 1"""
    case = VC.case(cid)
    want, _ = _expected(case)
    longest = max(hi - lo for lo, hi in VC.sets_of(case))
    for shape in case["shapes"]:
        snap, passes = _run_sets(crtlib, case, shape)
        print("%s shape %d: %d passes" % (cid, shape, passes))
        assert 1 <= passes <= longest + 1
        _compare(case, want, snap, "%s shape %d" % (cid, shape))


# --- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["n12-keep-shared", "n12-ab-keep-zeros", "n0-keep"])
def test_every_sets_generator_is_where_libcs_is(crtlib, cid):
    """after the call, entry `last field of set s` of the history array gives the rand() that libc gives next after set s's loop"""
    case = VC.case(cid)
    _, nxt = _expected(case)
    snap, _ = _run_sets(crtlib, case)
    for s, (_lo, hi) in enumerate(VC.sets_of(case)):
        assert _next_rand(snap["hist"][hi - 1]) == nxt[s], "%s: the generator after set %d is not where libc's is" % (cid, s)


# --- 3 -------------------------------------------------------------------------------------------------------------------------
def _run_sequence(crtlib, case, lo, hi, s_idx, shape=0):
    """CRT.sequence on a context of its own over fields [lo, hi) as set s_idx of the case"""
    g = _context(crtlib, case, hi - lo, shape)
    g.state[0, crtlib.ST_HSYNC], g.state[0, crtlib.ST_VSYNC] = VC.incoming(case)[s_idx]
    g.srand([VC.seeds(case)[s_idx]] + [900 + k for k in range(lo + 1, hi)])
    init = VC.init_pictures(case)
    passes = g.sequence(_settings(crtlib, case, lo, hi), case["noise"], out_init=None if init is None else _to_dev(VC.init_of_set(init, s_idx)))
    snap = _snapshot(crtlib, g)
    g.close()
    return snap, passes


@pytest.mark.parametrize("cid", ["n12-blend-keep", "n12-ab-keep-zeros"])
def test_one_set_equals_sequence(crtlib, cid):
    """n_sets = 1: the oracle's loop, and (library against library) CRT.sequence on the same inputs: pictures, state, histories, passes"""
    case = dict(VC.case(cid), id=cid + "-one-set", set_first=[0, 6])
    want, nxt = _expected(case)
    snap, passes = _run_sets(crtlib, case)
    _compare(case, want, snap, cid + " as one set")
    assert _next_rand(snap["hist"][5]) == nxt[0]
    one, p1 = _run_sequence(crtlib, case, 0, 6, 0)
    _same(snap, one, cid + " as one set against CRT.sequence", rows=VC.kept_rows(case))
    assert p1 == passes


@pytest.mark.parametrize("cid", ["n12-keep-shared", "n12-ab-blend-fade"])
def test_sets_equal_a_loop_of_sequence_calls(crtlib, cid):
    """the sets call against CRT.sequence once per set on the set's slices of the images, pictures, states and histories"""
    case = VC.case(cid)
    snap, passes = _run_sets(crtlib, case)
    per_set = []
    for s, (lo, hi) in enumerate(VC.sets_of(case)):
        one, p1 = _run_sequence(crtlib, case, lo, hi, s)
        per_set.append(p1)
        _same(snap, one, "%s set %d" % (cid, s), rows=VC.kept_rows(case), lo=lo, hi=hi)
    assert passes == max(per_set)


# --- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", VC.KNOB_CASE_IDS)
def test_knobs_per_field_with_per_set_streams(crtlib, cid):
    """sequence_sets_knobs(vhs_streams=True): distinct (noise, hue, saturation) per field, a noise-0 field inside a noisy set, against
    the oracle's loop with the knobs set per field"""
    case = VC.case(cid)
    assert len(set(case["triples"])) == VC.n_fields(case) and any(t[0] == 0 and lo < k < hi - 1 for lo, hi in VC.sets_of(case)
                                                                   for k, t in enumerate(case["triples"]) if lo <= k < hi)
    want, nxt = _expected(case)
    snap, _ = _run_sets(crtlib, case)
    _compare(case, want, snap, cid)
    for s, (_lo, hi) in enumerate(VC.sets_of(case)):
        assert _next_rand(snap["hist"][hi - 1]) == nxt[s]


# --- 5 -------------------------------------------------------------------------------------------------------------------------
def _raw_call(g, p, s, set_first):
    first = (C.c_int * len(set_first))(*set_first)
    return g.L.crthip_sequence_sets(g.ctx, C.byref(p), len(set_first) - 1, first, C.c_void_p(s.data.data_ptr()), g._image_stride(s),
                                    C.c_void_p(g.out.data_ptr()), g.out.stride(0), None, 0, C.c_void_p(g.state.data_ptr()), None)


@pytest.mark.parametrize("name", ["vhs", "vhslcg", "ntsc"])
def test_refusals(crtlib, name):
    """no history bound (vhs); the flag with CRTHIP_F_VHS_LCG_NOISE (vhslcg) and on another system (ntsc): CRTHIP_E_ARG with a message,
    d_out (0x5a) and d_state untouched, and the context still works afterwards"""
    case = dict(VC.case("n12-keep-shared"), name=name)
    sf = case["set_first"]
    g = _context(crtlib, case, VC.n_fields(case), 0)
    s = _settings(crtlib, case)
    if name == "vhs":
        _load_sets(crtlib, g, case)
        p = g.params(s, 12, crtlib.F_VHS_SET_STREAMS)
        assert g.L.crthip_vhs_bind_history(g.ctx, None) == 0
        word = b"crthip_vhs_bind_history"
    else:
        p = g.params(s, 12)
        p.flags |= crtlib.F_VHS_SET_STREAMS                # (crthip_params_finalize refuses the combination: set behind its back)
        word = b"CRTHIP_F_VHS_SET_STREAMS"
        with pytest.raises(ValueError):
            g.sequence_sets(s, 12, sf, vhs_streams=True)
    g._load_field_state(s)
    g.out.fill_(0x5a)
    before = g.state.clone()
    assert _raw_call(g, p, s, sf) == -1
    assert word in g.L.crthip_error_string(g.ctx), g.L.crthip_error_string(g.ctx)
    g.synchronize()
    assert bool((g.out == 0x5a).all()) and bool((g.state == before).all())
    if name == "vhs":
        assert g.L.crthip_vhs_bind_history(g.ctx, C.c_void_p(g.vhs_hist.data_ptr())) == 0
        snap, _ = _run_sets(crtlib, case, g=g)
        _compare(case, _expected(VC.case("n12-keep-shared"))[0], snap, "after the refusal")
    else:
        p.flags &= ~crtlib.F_VHS_SET_STREAMS
        assert _raw_call(g, p, s, sf) == 0
        g.synchronize()
        assert not bool((g.out == 0x5a).all())
    g.close()


def test_without_the_flag_the_stock_build_is_still_refused(crtlib):
    case = VC.case("n12-keep-shared")
    g = _context(crtlib, case, VC.n_fields(case), 0)
    s = _settings(crtlib, case)
    g.out.fill_(0x5a)
    assert _raw_call(g, g.params(s, 12), s, case["set_first"]) == -1
    assert b"rand()" in g.L.crthip_error_string(g.ctx)
    with pytest.raises(RuntimeError):
        g.sequence_sets(s, 12, case["set_first"])
    g.synchronize()
    assert bool((g.out == 0x5a).all())
    g.close()


# --- 6 -------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_contexts_history(crtlib):
    """on ONE context: a sets call with the flag, a plain crthip_sequence, a crthip_fieldpass -- each gives what a fresh context gives;
    then the reverse order on another context"""
    case = VC.case("n12-blend-fade-shared")
    n = VC.n_fields(case)
    s = _settings(crtlib, case)

    def reset(g):
        g.out.zero_()
        g.state.zero_()
        g.state[:, crtlib.ST_RN] = 194
        g.state[0, crtlib.ST_HSYNC], g.state[0, crtlib.ST_VSYNC] = 7, 2

    def op_sets(g):
        reset(g)
        return _run_sets(crtlib, case, g=g)

    def op_sequence(g):
        reset(g)
        g.srand([4711] * n)
        passes = g.sequence(s, case["noise"], out_init=_init(case))
        return _snapshot(crtlib, g), passes

    def op_fieldpass(g):
        reset(g)
        g.srand([100 + k for k in range(n)])
        g.fieldpass(s, case["noise"])
        return _snapshot(crtlib, g), 0

    ops = [("sets", op_sets), ("sequence", op_sequence), ("fieldpass", op_fieldpass)]
    fresh = {}
    for what, op in ops:
        g = _context(crtlib, case, n, 0)
        fresh[what] = op(g)
        g.close()
    _compare(case, _expected(case)[0], fresh["sets"][0], "fresh context")
    for order in (ops, ops[::-1]):
        g = _context(crtlib, case, n, 0)
        for what, op in order:
            snap, passes = op(g)
            _same(snap, fresh[what][0], "%s after %s" % (what, [w for w, _ in order]))
            assert passes == fresh[what][1]
        g.close()

"""The stage-level entry points (crthip_noise, crthip_sync, crthip_decode) and the drop-in crt_demodulate on signals the library's own
encoder never makes (tests/signal_cases.py): carrier amplitudes on and around the decoder's dispatch bounds with +-127 in the active
window, sync decisions on their edges, the noise stage's clamps.  analog[] and the start state (hsync, vsync, ccf) are written by hand,
two demodulate passes follow, and every pass is compared with the CPU oracle bit for bit: inp, the line table, hsync, vsync, rn, ccf and
every picture byte.  What the cases reach is proven without a GPU by tests/test_signals_cpu.py."""
import os

import numpy as np
import pytest

import crtref as R
import signal_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crtlib():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def _context(crtlib, cid, geom, shape=1, exact=0, dec_float=None, wide_lpw=0):
    """a fresh context (CRTHIP_DEC_FLOAT is read when a context is created; the environment is restored)"""
    case = S.ALL_CASES[cid]
    name, n = case["name"], len(case["fields"])
    saved = os.environ.get("CRTHIP_DEC_FLOAT")
    if dec_float is not None:
        os.environ["CRTHIP_DEC_FLOAT"] = "1" if dec_float else "0"
    try:
        g = crtlib.CRT(n, geom[0], geom[1], geom[2], "ntsc" if name.startswith("ntscfir") else name, device=0)
    finally:
        if saved is None:
            os.environ.pop("CRTHIP_DEC_FLOAT", None)
        else:
            os.environ["CRTHIP_DEC_FLOAT"] = saved
    g.eq_fir = R.EQ_KERNEL.get(name, 0)
    g.set_shape(shape)
    g.set_exact(exact)
    g.set_wide_lpw(wide_lpw)
    for k, v in case["knobs"].items():
        setattr(g, k, v)
    return g


def _run(crtlib, cid, geom=None, **kw):
    """-> per pass (inp, line table, state, out) and what float_stages_used said"""
    import torch
    case, built = S.ALL_CASES[cid], S.build_case(cid)
    geom = geom or S.case_geom(cid)
    g = _context(crtlib, cid, geom, **kw)
    n = g.n
    g.analog[:, :g.input_size] = torch.from_numpy(built["signals"]).to(g.dev)
    st = np.zeros((n, crtlib.STATE_INTS), dtype=np.int32)
    st[:, crtlib.ST_RN] = 194
    for k, (hs, vs, ccf) in enumerate(built["starts"]):
        st[k, crtlib.ST_HSYNC], st[k, crtlib.ST_VSYNC] = hs, vs
        full = np.zeros((5, 5), dtype=np.int32)
        full[:ccf.shape[0], :ccf.shape[1]] = ccf
        st[k, crtlib.ST_CCF:crtlib.ST_CCF + 25] = full.reshape(-1)
    g.state.copy_(torch.from_numpy(st).to(g.dev))
    per, used = [], []
    for _ in range(case["steps"]):
        g.demodulate(case["noise"])
        g.synchronize()
        used.append(g.float_stages_used())
        per.append((g.inp.cpu().numpy()[:, :g.input_size].copy(), g.line_table.cpu().numpy().copy(), g.state.cpu().numpy().copy(),
                    g.out.cpu().numpy().copy()))
    g.close()
    return per, used


def _compare(crtlib, cid, per, what, geom=None):
    case = S.ALL_CASES[cid]
    want = S.expected(cid, geom or S.case_geom(cid))
    orc = S.oracle(case["name"])
    checked = 0
    for k in range(len(case["fields"])):
        for step in range(case["steps"]):
            o = want[k][step]
            inp, lines, st, out = per[step]
            w = "%s %s field %d pass %d: " % (cid, what, k, step)
            if case["group"] == "noise" or not o["undefined"]:
                # the noise stage reads analog[] and rn and nothing else: defined whatever the sync chain does afterwards
                np.testing.assert_array_equal(inp[k], o["inp"], err_msg=w + "inp")
                assert int(st[k][crtlib.ST_RN]) == o["rn"], w + "rn"
                checked += case["group"] == "noise"
            if o["undefined"]:
                break
            tr = o["trace"]
            valid = tr[:, 0] == 1
            np.testing.assert_array_equal((lines[k][:, 4] & 0xffff) > 0, valid, err_msg=w + "valid lines")
            np.testing.assert_array_equal(lines[k][valid][:, [0, 1, 2, 3, 5, 6, 7]], tr[valid][:, [1, 2, 3, 4, 6, 7, 8]],
                                          err_msg=w + "line table (pos, wave0, wave1, beg, hsync, dx, scanl)")
            assert (int(st[k][crtlib.ST_HSYNC]), int(st[k][crtlib.ST_VSYNC])) == (o["hsync"], o["vsync"]), w + "hsync, vsync"
            np.testing.assert_array_equal(st[k][crtlib.ST_CCF:crtlib.ST_CCF + 25].reshape(5, 5)[:orc.vper, :orc.ccs], o["ccf"], err_msg=w + "ccf")
            np.testing.assert_array_equal(out[k].reshape(-1), o["out"], err_msg=w + "out")
            checked += 1
    assert checked >= len(case["fields"]), "the case checks nothing"      # (noise cases: inp and rn of every pass count)


def _floats_expected(cid):
    """the float-stage instantiation is launched for systems of 4 samples per chroma cycle with the 3-band equaliser
    while the batch is inside tiers 0 / 1, i.e. |bright| <= 2 600.  (Launched: which waves stay in it is the lines' business -- here
    only those at or below 65 532, see signal_cases.py beside the corner cases.)"""
    case = S.ALL_CASES[cid]
    if case["floats"] is not None:
        return case["floats"]
    return int(S.oracle(case["name"]).ccs == 4 and not R.EQ_KERNEL.get(case["name"], 0) and abs(S.case_bright(cid)) <= S.T0_BRIGHT_MAX)


@pytest.mark.parametrize("cid", sorted(S.ALL_CASES))
def test_signal_cases_lane_per_scanline_float_and_integer_stages(crtlib, cid):
    """the throughput shape (for the bloom build: the lane-per-scanline decoder behind its sort), float stages on and off"""
    case = S.ALL_CASES[cid]
    on, used_on = _run(crtlib, cid, shape=1, dec_float=True)
    off, used_off = _run(crtlib, cid, shape=1, dec_float=False)
    _compare(crtlib, cid, on, "float")
    _compare(crtlib, cid, off, "integer")
    assert used_on == [_floats_expected(cid)] * case["steps"], "float stages with the switch on: %s" % used_on
    assert used_off == [0] * case["steps"], "float stages with the switch off: %s" % used_off
    want = S.expected(cid, S.case_geom(cid))
    keep = [k for k in range(len(case["fields"])) if not any(r["undefined"] for r in want[k])]
    for step in range(case["steps"]):
        for a, b in zip(on[step], off[step]):
            np.testing.assert_array_equal(a[keep], b[keep], err_msg="%s pass %d: float against integer" % (cid, step))


@pytest.mark.parametrize("cid", sorted(c for c in S.ALL_CASES if not c.startswith("ntscfir")))
def test_signal_cases_scanline_parallel_shape(crtlib, cid):
    _compare(crtlib, cid, _run(crtlib, cid, shape=2)[0], "shape 2")


TIER_CASES = sorted(c for c in S.AMP_CASES if c.startswith(("ntsc-", "pv1k-", "ntscbloom-ramp", "snes-at120000")))


@pytest.mark.parametrize("shape", [1, 2])
@pytest.mark.parametrize("exact", [1, 2, 3])
@pytest.mark.parametrize("cid", TIER_CASES)
def test_signal_cases_forced_tiers(crtlib, cid, exact, shape):
    """crthip_set_exact: 1 the 32-bit multiplies everywhere, 2 no 64-bit-mad tiers, 3 never drop the I / Q low cascades"""
    _compare(crtlib, cid, _run(crtlib, cid, shape=shape, exact=exact)[0], "exact %d shape %d" % (exact, shape))


GEOM_CASES = ["ntsc-ramp", "ntsc-corner-bright+2600", "ntsc-corner-bright-2600", "ntsc-at65532", "ntsc-at524288"]


@pytest.mark.parametrize("exact", [0, 3])
@pytest.mark.parametrize("cid", GEOM_CASES)
def test_signal_cases_three_byte_output(crtlib, cid, exact):
    """101 x 77 RGB: the 3-byte instantiations, an odd width wider than one pixel tile"""
    geom = (101, 77, R.FMT_RGB)
    for dec_float in (True, False):
        per, used = _run(crtlib, cid, geom=geom, shape=1, exact=exact, dec_float=dec_float)
        _compare(crtlib, cid, per, "101x77 RGB float=%s exact=%d" % (dec_float, exact), geom=geom)
        if exact == 0:
            assert used == [int(dec_float) * _floats_expected(cid)] * 2


# the wide-run decoder keeps the waves of tiers 0 / 1, at these entry points the lines at or below 65 532: the cases that have many
# of them (the ramp's first lines; the at65532 fields up to the line above the bound); everything else goes back to k_decode
WIDE_RUN_CASES = ["ntsc-ramp", "ntsc-at65532", "ntsc-at65532-sat4", "ntsc-at65532-sat-4"]


@pytest.mark.parametrize("lpw", [8, 16])
@pytest.mark.parametrize("cid", WIDE_RUN_CASES)
def test_signal_cases_wide_run_decoder(crtlib, cid, lpw):
    """a picture 1700 wide takes the wide-run decoder (both instantiations pinned; from 1280 pixels on a picture counts as wide, and a run
    of 256 pixels must fit the decoder's ring of 128 samples, which 753 samples over 1280 pixels do not); the groups of the higher tiers stay with k_decode.
    The wide-run decoder keeps its integer stages: the same case, context and switch (float stages on) at 64 x 48 reports the float
    kernel, at 1700 x 48 it must not -- which is how the path taken shows."""
    geom = (1700, 48, R.FMT_BGRA)
    per, used = _run(crtlib, cid, geom=geom, shape=1, wide_lpw=lpw, dec_float=True)
    _compare(crtlib, cid, per, "1700x48 lpw %d" % lpw, geom=geom)
    assert _floats_expected(cid) == 1 and used == [0, 0], "the wide-run decoder was not taken: float stages %s" % used
    assert _run(crtlib, cid, shape=1, wide_lpw=lpw, dec_float=True)[1] == [1, 1]


@pytest.mark.parametrize("cid", ["ntsc-ramp", "ntsc-corner-bright+2600", "hsync-edges", "tail-128"])
def test_dropin_crt_demodulate_on_hand_made_signals(crtlib, cid):
    """libntsccrt_hip_ntsc.so: analog[] and the start state written into a host struct CRT, crt_demodulate twice, against the oracle
    (which tests/test_signals_cpu.py pins to the reference on the same cases) and, where it was built, the reference itself"""
    case, built = S.ALL_CASES[cid], S.build_case(cid)
    geom = S.case_geom(cid)
    want = S.expected(cid, geom)
    drop = R.RefLib("ntsc", dropin=True)
    ref = R.RefLib("ntsc") if R.have_ref("ntsc") else None
    for k in range(len(case["fields"])):
        got = S.run_checker(drop, built["signals"][k], case["knobs"], built["starts"][k], case["noise"], case["steps"], geom)
        theirs = S.run_checker(ref, built["signals"][k], case["knobs"], built["starts"][k], case["noise"], case["steps"], geom) if ref else None
        for step in range(case["steps"]):
            o, r = want[k][step], got[step]
            if o["undefined"]:
                break
            for other, who in ((o, "oracle"), (theirs[step] if theirs else None, "reference")):
                if other is None:
                    continue
                w = "%s field %d pass %d against the %s: " % (cid, k, step, who)
                np.testing.assert_array_equal(r["inp"], other["inp"], err_msg=w + "inp")
                np.testing.assert_array_equal(r["ccf"], other["ccf"], err_msg=w + "ccf")
                assert (r["hsync"], r["vsync"], r["rn"]) == (other["hsync"], other["vsync"], other["rn"]), w + "hsync, vsync, rn"
                np.testing.assert_array_equal(r["out"], other["out"], err_msg=w + "out")

"""What the hand-made signals of tests/signal_cases.py claim to reach, proven on the CPU oracle's trace (a case that no longer
reaches its edge fails HERE, not silently on the GPU); the oracle against the real reference on the same cases; and the host's
model of the float filter stages on the cascade inputs of the corner cases."""
import numpy as np
import pytest

import crtref as R
import signal_cases as S

needs_ref = pytest.mark.skipif(not R.have_ref("ntsc"), reason="oracle/_ref not built (no reference sources on this machine)")

AMP = sorted(S.AMP_CASES)


def _want(cid):
    return S.expected(cid, S.case_geom(cid))


@pytest.mark.parametrize("cid", AMP)
def test_amplitude_cases_reach_what_they_claim(cid):
    case = S.ALL_CASES[cid]
    name, knobs = case["name"], case["knobs"]
    sat, hue = knobs.get("saturation", 10), knobs.get("hue", 0)
    built, want = S.build_case(cid), _want(cid)
    assert 2 <= len(case["fields"]) <= 8 and case["steps"] == 2
    for k, f in enumerate(case["fields"]):
        for step in range(2):
            assert not want[k][step]["undefined"], "a case from lock excludes nothing (field %d pass %d)" % (k, step)
        r = want[k][0]
        tr = r["trace"]
        assert int(tr[:, 0].sum()) == tr.shape[0], "every line of the field is decoded"
        # the integer model of the ccf recurrence against the oracle: on the pass' own inp[] and sync chain
        geometry = S.line_geometry(name, tr, r["vsync"])
        model = S.model_waves(name, r["inp"], geometry, built["starts"][k][2], hue, sat)
        for idx, w in model.items():
            assert (w[0], w[1]) == (int(tr[idx, 2]), int(tr[idx, 3])), "%s field %d line %d: model %s, oracle %s" % (cid, k, idx, w, tr[idx, 2:4])
        if case["noise"] == 0:
            assert [g[3] for g in geometry] == [g[3] for g in built["geometry"][k]], "the rewritten regions moved the sync chain"
        amp = S.line_amplitudes(cid, k)
        if f["kind"] == "ramp":
            for bound in S.BOUNDS:
                assert (amp[amp > 0] <= bound).any() and (amp > bound).any(), "%s field %d: the ramp does not cross %d" % (cid, k, bound)
            # ... as a ramp: the lines of one 64-line wavefront fall into different tiers
            tiers = np.searchsorted(np.array(S.BOUNDS), amp, side="left")
            assert max(len(set(tiers[i:i + 64].tolist())) for i in range(0, 240, 64)) >= 3
        else:
            assert amp[S.HIT_LINE] == f["bound"], "%s field %d: amplitude %d on the line that should carry %d" % (cid, k, amp[S.HIT_LINE], f["bound"])
            assert f["bound"] < amp[S.ABOVE_LINE] <= f["bound"] + abs(sat), (cid, k, int(amp[S.ABOVE_LINE]))
            if f["bound"] == S.LOSKIP_WAVE_MAX and k == 0:
                # the first wave of 64 lines never leaves the bound (so it stays in tier 0 / the float kernel on the GPU: every other
                # line of these fields shares a wave with one above 65 532) and holds it exactly under a whole rotation of the patterns
                assert (amp[:64] <= f["bound"]).all() and (amp[20:64] == f["bound"]).all(), (cid, amp[:64].tolist())
                if f["rot"] != "blocks":
                    assert {S._pattern_of(f)(idx) for idx in range(20, 64)} == set(S.PATTERNS)
            if oracle_ccs(name) == 4:
                w = tr[S.HIT_LINE, 2 + f["dom"]]
                assert abs(int(w)) == f["bound"] and (w > 0) == (f["sign"] * sat > 0), "dominant carrier and its sign"
            # the signal on the two lines is what the field asked for: full range, sign-matched where it says so
            for idx in (S.HIT_LINE, S.ABOVE_LINE):
                pos = int(tr[idx, 1])
                s = r["inp"][pos:pos + S.oracle(name).av_len].astype(np.int64)
                assert set(np.unique(np.abs(s)).tolist()) == {127}
                if f["corner"] in ("signI", "signQ"):
                    w0, w1 = int(tr[idx, 2]), int(tr[idx, 3])
                    four = np.array([w0, w1, -w0, -w1])
                    wv = four[(np.arange(s.size) + (0 if f["corner"] == "signI" else 3)) & 3]
                    assert (s * wv >= 0).all() and ((s * wv) >> 9).max() >= (127 * f["bound"] >> 9) - 1


def oracle_ccs(name):
    return S.oracle(name).ccs


def test_every_pattern_meets_every_tier_and_the_knob_corners_exist():
    """the pattern rotation puts each active-window pattern on lines below 65 532, between the bounds and above 524 288 (ramp fields);
    the brightness corners are |bright| = 2 600 exactly and 2 601"""
    for cid in ("ntsc-ramp", "snes-ramp", "ntscp0-ramp"):
        seen = {}
        for k, f in enumerate(S.ALL_CASES[cid]["fields"]):
            amp = S.line_amplitudes(cid, k)
            of = S._pattern_of(f)
            for idx in range(240):
                if amp[idx] > 0:
                    seen.setdefault(of(idx), set()).add(int(np.searchsorted(np.array(S.BOUNDS), amp[idx], side="left")))
        assert set(seen) == set(S.PATTERNS)
        assert all(t == {0, 1, 2, 3} for t in seen.values()), seen
    assert [S.case_bright(c) for c in ("ntsc-corner-bright+2600", "ntsc-corner-bright-2600", "ntsc-corner-bright+2601",
                                       "ntsc-corner-bright-2601")] == [2600, -2600, 2601, -2601]
    assert {S.ALL_CASES[c]["knobs"].get("contrast") for c in S.AMP_CASES} >= {20, 400}
    assert {np.sign(S.ALL_CASES[c]["knobs"]["saturation"]) for c in S.AMP_CASES} == {1, -1}


def test_vsync_edges():
    cid = "vsync-edges"
    want = _want(cid)
    sd = S.oracle("ntsc").sys
    assert sd.vsync_thresh == S.T_V and sd.hres // 2 == 455
    for k, (vsync, odd) in enumerate(S.VSYNC_WANT):
        r = want[k][0]
        assert not want[k][1]["undefined"]
        assert r["vsync"] == vsync, "field %d: vsync %d" % (k, r["vsync"])
        assert int(r["trace"][0, 4]) == odd, "field %d: parity (first row of a 480-row picture)" % k
    # the running sums on the found lines are what the case names say: equal to the threshold, one above it and never below
    sig = S.build_case(cid)["signals"].astype(np.int64)
    acc = np.cumsum(sig[1][(S.VS0 - 3) * sd.hres:(S.VS0 - 2) * sd.hres])
    assert acc.min() == S.T_V and int(np.argmax(acc <= S.T_V)) == 93
    acc = np.cumsum(sig[2][(S.VS0 - 3) * sd.hres:(S.VS0 - 2) * sd.hres])
    assert acc.min() == S.T_V + 1
    for k, j in ((3, 455), (4, 456), (5, 29)):
        acc = np.cumsum(sig[k][(S.VS0 - 3) * sd.hres:(S.VS0 - 2) * sd.hres])
        assert int(np.argmax(acc <= S.T_V)) == j and acc[j - 1] > S.T_V
    for i in range(-sd.vsync_window, sd.vsync_window):
        ln = S.VS0 + i
        assert np.cumsum(sig[0][ln * sd.hres:(ln + 1) * sd.hres]).min() > S.T_V


@pytest.mark.parametrize("cid", sorted(S.HSYNC_WANT))
def test_hsync_edges_and_the_walk_over_the_line_end(cid):
    want, built = _want(cid), S.build_case(cid)
    sd = S.oracle(S.ALL_CASES[cid]["name"]).sys
    assert sd.hsync_thresh == S.T_H
    for k, d in enumerate(S.HSYNC_WANT[cid]):
        hs0 = built["starts"][k][0]
        assert int(want[k][0]["trace"][0, 6]) == (hs0 + d) % sd.hres, "field %d" % k
        assert not want[k][1]["undefined"]
    # equality: the running sum of fields 0, 1 and 3 touches the threshold and never goes below it
    for k in (0, 1, 3):
        hs0, vs0 = built["starts"][k][:2]
        at = ((sd.top + vs0) % sd.vres) * sd.hres + hs0 + sd.sync_beg - sd.hsync_window
        acc = np.cumsum(built["signals"][k][at:at + 2 * sd.hsync_window].astype(np.int64))
        assert acc.min() == S.T_H
    if cid != "hsync-edges":
        return
    # field 4: never met -- the window's width further on every line, through HRES and round
    tr = want[4][0]["trace"]
    hs = tr[:, 6].astype(np.int64)
    assert hs[0] == 110 + sd.hsync_window
    assert (np.diff(hs) % sd.hres == sd.hsync_window).all() and (np.diff(hs) < 0).sum() >= 2
    excluded = [k for k in range(len(want)) if want[k][1]["undefined"]]
    assert excluded == [4] and 4 * len(excluded) < len(want), "fewer than a quarter of the fields may drop out"
    assert not want[4][0]["undefined"]


@pytest.mark.parametrize("cid", ["tail-128", "tail-640"])
def test_tail_cases_read_the_bytes_behind_the_field(cid):
    want = _want(cid)
    orc = S.oracle("ntsc")
    sd = orc.sys
    for k in range(len(want)):
        for step in range(2):
            r = want[k][step]
            assert not r["undefined"]
            tr = r["trace"]
            last = tr[:, 1] // sd.hres == sd.vres - 1
            assert last.sum() == 1
            pos, hs = int(tr[last, 1][0]), int(tr[last, 6][0])
            assert 5 <= hs < 5 + R.ORC_TAIL and pos + sd.av_len > sd.input_size, (pos, hs)
    assert np.int8(np.uint8(S.case_geom(cid)[0] & 0xff)) == -128, "the first mirrored byte is outw's low byte"


@pytest.mark.parametrize("cid", sorted(S.NOISE_CASES))
def test_noise_cases(cid):
    case = S.ALL_CASES[cid]
    sig = S.build_case(cid)["signals"]
    want = _want(cid)
    for k in range(sig.shape[0]):
        assert {-128, -127, 0, 127} <= set(np.unique(sig[k]).tolist())
        inp = want[k][0]["inp"]
        assert inp.min() >= -127
        if case["noise"] == 0:
            np.testing.assert_array_equal(inp, np.maximum(sig[k], -127))          # -128 in, -127 out
        if abs(case["noise"]) >= 255:
            assert inp.min() == -127 and inp.max() == 127                          # both clamps


def test_exclusion_caps():
    for cid, case in S.ALL_CASES.items():
        if case["group"] == "noise":
            continue
        want = _want(cid)
        excluded = [k for k in range(len(want)) if any(r["undefined"] for r in want[k])]
        if case["group"] == "amp":
            assert not excluded, cid
        else:
            assert 4 * len(excluded) < len(want), (cid, excluded)


# The reference computes its products in `int`, and above |wave| ~ 145 000 at +-127 some of them leave 32 bits: undefined in C,
# wrapping in the oracle by contract (-fwrapv).  The reference build these tests use wraps the same way on every case here -- ramp and
# 524 288 cases included -- so no case is kept from this comparison.
@needs_ref
@pytest.mark.parametrize("cid", sorted(S.ALL_CASES))
def test_oracle_equals_the_reference(cid):
    case = S.ALL_CASES[cid]
    if not R.have_ref(case["name"]):
        pytest.skip("no reference build of " + case["name"])
    built, want = S.build_case(cid), _want(cid)
    ref = R.RefLib(case["name"])
    for k in range(len(case["fields"])):
        got = S.run_checker(ref, built["signals"][k], case["knobs"], built["starts"][k], case["noise"], case["steps"], S.case_geom(cid))
        for step in range(case["steps"]):
            o, r = want[k][step], got[step]
            if o["undefined"]:
                break
            what = "%s field %d pass %d " % (cid, k, step)
            np.testing.assert_array_equal(r["inp"], o["inp"], err_msg=what + "inp")
            np.testing.assert_array_equal(r["ccf"], o["ccf"], err_msg=what + "ccf")
            assert (r["hsync"], r["vsync"], r["rn"]) == (o["hsync"], o["vsync"], o["rn"]), what + "hsync, vsync, rn"
            np.testing.assert_array_equal(r["out"], o["out"], err_msg=what + "out")


# ---------------------------------------------------------------------------------------------------------------------------
# the host's model of the float filter stages on the corner cases' own cascade inputs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


@pytest.mark.parametrize("cid", ["ntsc-corner-bright+2600", "ntsc-corner-bright-2600", "ntsc-at120000", "snes-at120000", "ntscp0-at120000",
                                 "nes-at120000"])
def test_float_stage_model_holds_on_the_corner_inputs(lib, cid):
    """The only check of the float stages' arithmetic AT the 120 000 corner: on the GPU the stage-level entry points send every line
    above 65 532 to the 24-bit tier (signal_cases.py, beside the corner cases), so no hand-made signal reaches the float kernel there."""
    from test_float_stages_cpu import _reference, _run_cascade
    case = S.ALL_CASES[cid]
    name = case["name"]
    bright = S.case_bright(cid)
    p = lib.make_params(name, w=64, h=48, outw=64, outh=48, brightness=case["knobs"].get("brightness", 0))
    ok, f = lib.float_stages(p)
    assert ok == 1 and p.bright == bright
    want = _want(cid)
    av_len = S.oracle(name).av_len
    assert f.steps >= av_len
    # pass 0: the fifteen lines up to HIT_LINE (amplitude at the bound on all of them: one full rotation of the active-window patterns
    # and the corner line itself) inside the envelope, and ABOVE_LINE one unit of |saturation| outside it; pass 1: HIT_LINE again
    lines = [(0, idx, True) for idx in range(S.HIT_LINE - 14, S.HIT_LINE + 1)] + [(0, S.ABOVE_LINE, False), (1, S.HIT_LINE, True)]
    for k in range(len(case["fields"])):
        for step, idx, inside in lines:
            r = want[k][step]
            tr = r["trace"]
            pos, w0, w1 = int(tr[idx, 1]), int(tr[idx, 2]), int(tr[idx, 3])
            if step == 0:
                assert (max(abs(w0), abs(w1)) <= S.T0_WAVE_MAX) == inside, (cid, k, step, idx, w0, w1)
            inside = max(abs(w0), abs(w1)) <= S.T0_WAVE_MAX         # (pass 1 starts from pass 0's ccf: on either side)
            s = r["inp"][pos:pos + av_len].astype(np.int64)
            four = np.array([w0, w1, -w0, -w1], dtype=np.int64)
            i = np.arange(av_len)
            inputs = [s + bright, s + bright, (s * four[i & 3]) >> 9, (s * four[(i + 3) & 3]) >> 9]
            for c in range(4):
                q = f.cas[c]
                u = [int(v) for v in inputs[c]]
                if inside:
                    assert max(abs(v) for v in u) <= q.in_max, (cid, k, idx, c)
                # (_run_cascade itself asserts that every biased value stays in the binade)
                got, lo, hi = _run_cascade(q, len(u), u)
                assert got == _reference(q.c, u), (cid, k, idx, c)
                if inside:
                    assert q.lo <= lo and hi <= q.hi and max(abs(v) for v in got) <= q.state_max, (cid, k, idx, c)

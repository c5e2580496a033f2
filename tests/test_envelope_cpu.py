"""What tests/envelope_cases.py claims, proven without a GPU: the restated bound B against crthip_knobs_prepare; the oracle against
the real reference on every case; on the oracle's trace the amplitudes inside one |saturation| of the bound they name, the census of
line classes, the bytes inside the decoded windows; one row of the committed tuples re-derived by search()."""
import numpy as np
import pytest

import crtref as R
import envelope_cases as V

needs_ref = pytest.mark.skipif(not R.have_ref("ntsc"), reason="oracle/_ref not built (no reference sources on this machine)")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


@pytest.mark.parametrize("name", V.SYSTEMS)
def test_restated_bound_equals_knobs_prepare(lib, name):
    """literal == restatement == env.loskip_wave_max, for every listed noise; B's floor and the noise at which it is reached"""
    p = lib.make_params(name, w=64, h=48, outw=V.OUTW, outh=V.OUTH)
    assert len(V.BOUNDS[name]) == 6 and {0, 24, 60, V.NEGATIVE_NOISE, V.FLOOR_NOISE[name] - 1, V.FLOOR_NOISE[name]} == set(V.BOUNDS[name])
    for noise, want in V.BOUNDS[name].items():
        _, env = lib.knobs_prepare(p, np.array([(noise, 0, 10)]))
        assert env.loskip_wave_max == V.bound(name, noise) == want, (name, noise)
    assert V.floor_noise(name) == V.FLOOR_NOISE[name]
    assert V.BOUNDS[name][V.FLOOR_NOISE[name]] == V.B_FLOOR < V.BOUNDS[name][V.FLOOR_NOISE[name] - 1]
    for noise in (V.FLOOR_NOISE[name] + 1, 255, 256, 1 << 20, -(1 << 20)):                 # ... and never below it: not 65 532
        _, env = lib.knobs_prepare(p, np.array([(noise, 0, 10)]))
        assert env.loskip_wave_max == V.bound(name, noise) == V.B_FLOOR, (name, noise)
    _, env = lib.knobs_prepare(p, np.array([((1 << 20) + 1, 0, 10)]))
    assert env.loskip_wave_max == V.bound(name, (1 << 20) + 1) == 65786                     # the full range -128 .. 127
    # a batch takes the narrowest of its fields' bounds
    _, env = lib.knobs_prepare(p, np.array([(0, 0, 10), (60, 5, 12), (24, 0, -3)]))
    assert env.loskip_wave_max == V.BOUNDS[name][60]


def test_the_encoder_hue_does_not_move_the_range():
    for name in V.SYSTEMS:
        assert {V.signal_range(name, 24, enc_hue=h) for h in range(0, 360, 7)} == {V.signal_range(name, 24)}


@needs_ref
@pytest.mark.parametrize("cid", sorted(V.CASES))
def test_oracle_equals_the_reference(cid):
    name = V.CASES[cid]["name"]
    if not R.have_ref(name):
        pytest.skip("no reference build of " + name)
    want, got = V.expected(cid), V.run_case(R.RefLib(name), cid)
    for k in range(V.CASES[cid]["n"]):
        for step in range(V.STEPS):
            o, r = want[k][step], got[k][step]
            what = "%s field %d pass %d " % (cid, k, step)
            assert not o["undefined"], what + "no case excludes anything (start-state cases: recorded count 0)"
            for f in ("analog", "ccf_mod", "inp", "ccf", "out"):
                np.testing.assert_array_equal(r[f], o[f], err_msg=what + f)
            assert (r["rn"], r["hsync"], r["vsync"]) == (o["rn"], o["hsync"], o["vsync"]), what + "rn, hsync, vsync"


LOCK_CASES = sorted(c for c in V.CASES if c not in V.START_CASES)


@pytest.mark.parametrize("cid", LOCK_CASES)
def test_cases_land_where_they_say(cid):
    c = V.CASES[cid]
    b, q = V.case_bound(cid), abs(c["sat"])
    want = V.expected(cid)
    assert 2 <= c["n"] <= 4 and {V.E.field_of(k, s) for k in range(c["n"]) for s in range(V.STEPS)} == {0, 1}
    assert not any(r["undefined"] for per in want for r in per), "exclusions through reads_past_inp: 0 for every case from lock"
    amp = max(int(V.amplitudes(r["trace"]).max()) for per in want for r in per)
    assert amp == c["amp"] and V.DISTANCE[(c["name"], c["noise"], c["bound"], c["side"])] == abs(amp - b) < q + (c["side"] == "above")
    if c["side"] == "below":
        assert b - q < amp <= b, (amp, b)
    else:
        assert b < amp <= b + q, (amp, b)
    rec = V.RECORDED[cid]
    census = V.census(cid)
    assert census == rec["census"] and sum(census) == sum(int((r["trace"][:, 0] == 1).sum()) for per in want for r in per)
    t0, t1, keeplo, not64 = census
    # the classes the case names are not empty: the bound's two sides
    sides = {"lo": (t0, t1 + keeplo), "B": (t1, keeplo), "t0": (t1 + keeplo, not64)}[c["bound"]]
    assert sides[0] > 0 and (sides[1] > 0 or c["side"] == "below"), census
    if c["side"] == "below" and c["bound"] != "B":
        assert sides[1] == 0, census
    lo, hi = V.window_bytes(cid)
    rlo, rhi = V.signal_range(c["name"], c["noise"], c["enc_hue"])
    assert (lo, hi) == rec["window"] and (lo - rlo, rhi - hi) == rec["slack"] and rlo <= lo and hi <= rhi
    if c["noise"] == 0 and c["name"] != "nes" and c["family"] != "random":
        # the hostile images hold both clamp ends, 0 and 110, inside ONE decoded window, counted on the active samples alone
        # (pos .. pos + AV_LEN: the blanking in front of them is 0 as well and does not count): the phase rows in every field-pass
        both = [n for n, _ in V.spanning_windows(cid, 0, 110, margin=0)]
        assert sum(both) > 0 and (c["family"] != "phase" or min(both) > 0), both


@pytest.mark.parametrize("cid", sorted(V.START_CASES))
def test_start_state_cases(cid):
    """(a): single decoded windows hold the sync tip, -40, beside white video, 110 -- on tier-1 lines in the first case; the census and
    the exclusions through reads_past_inp are the recorded ones (0, and never half of a case's fields)"""
    c, rec, want = V.CASES[cid], V.RECORDED[cid], V.expected(cid)
    assert c["starts"] and any(st != (0, 0) for st in c["starts"]) and c["noise"] == 0
    dropped = [k for k, per in enumerate(want) if any(r["undefined"] for r in per)]
    assert sum(r["undefined"] for per in want for r in per) == rec["excluded"] == 0 and 2 * len(dropped) < c["n"]
    assert V.census(cid) == rec["census"] and V.window_bytes(cid) == rec["window"]
    span = V.spanning_windows(cid, -40, 110)
    assert span == rec["spanning"] and sum(n for n, _ in span) > 0
    assert "tier1" in {k for _, cl in V.RECORDED["ntsc-noise0-B-above-phase-start140"]["spanning"] for k in cl}
    # the start state is what does it: from lock no window of the same tuple and images reaches a sync tip
    base = V.START_CASES[cid][0]
    assert sum(n for n, _ in V.spanning_windows(base, -40, 110)) == 0


def test_tail_lines_inside_the_envelope_are_reached_from_lock():
    """the reads_tail clause of line_tier_flags: the field's last line reads the mirrored tail while 65 532 < amplitude <= B"""
    cid = "ntsc-noise0-B-below-phase"
    sd = V.oracle("ntsc").sys
    n = 0
    for per in V.expected(cid):
        for r in per:
            tr = r["trace"][r["trace"][:, 0] == 1]
            tail = tr[:, 1].astype(np.int64) + sd.av_len + 8 > sd.input_size
            a = V.amplitudes(r["trace"])[tail]
            assert tail.sum() == 1 and V.LOSKIP_WAVE_MAX < int(a[0]) <= V.case_bound(cid)
            assert V.line_class(tr[tail][0, 2], tr[tail][0, 3], V.case_bound(cid), True) == "keeplo"
            assert V.line_class(tr[tail][0, 2], tr[tail][0, 3], V.case_bound(cid), False) == "tier1"
            n += 1
    assert n == 4 == V.RECORDED[cid]["census"][2]


def test_one_row_is_rederived_by_the_search():
    """the literals come from the rule: search() restricted to the row's encoder hue finds the committed tuple"""
    key = ("ntsc", 24, "lo", "above")
    enc, mon, sat, amp = V.TUPLES[key]
    got = V.search("ntsc", 24, [V.LOSKIP_WAVE_MAX], n=V.N_FIELDS, enc_hues=[enc])[V.LOSKIP_WAVE_MAX]
    assert got[("above", 1 if sat > 0 else -1)] == (amp - V.LOSKIP_WAVE_MAX, enc, mon, sat, amp)
    assert V.mon_hue_terms("ntsc")[V.S.hue_terms(V.oracle("ntsc"), mon)] == mon

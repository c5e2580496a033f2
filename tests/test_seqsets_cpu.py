"""CPU checks of the cases of the many-sets sequence mode (tests/seqsets_cases.py; the GPU side is tests/test_gpu_seqsets.py): the
expected values are the reference's, no chosen case runs into the reference's undefined over-read, every case can tell a set
boundary from no boundary, and the blend case with duplicated rows exercises the fold's cross-row dependency."""
import numpy as np
import pytest

import crtref as R
import seqsets_cases as SC


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    R.build_oracle()


@pytest.fixture(scope="module")
def want_cache():
    return {}


def _want(cache, cid):
    if cid not in cache:
        cache[cid] = SC.expected(SC.case(cid), check_reads=True)      # also: no field of the case reads past inp[] + 16
    return cache[cid]


@pytest.mark.parametrize("cid", SC.CASE_IDS)
def test_no_case_reads_past_the_field(want_cache, cid):
    """R.reads_past_inp must not hold for any field of any case (asserted inside the per-set loop): nothing is masked later"""
    case = SC.case(cid)
    want = _want(want_cache, cid)
    assert len(want) == SC.n_fields(case)
    sf = case["set_first"]
    assert sf[0] == 0 and all(b > a for a, b in zip(sf, sf[1:]))


@pytest.mark.parametrize("cid", SC.CASE_IDS)
def test_oracle_equals_reference_per_set(want_cache, cid):
    case = SC.case(cid)
    if not R.have_ref(case["name"]):
        pytest.skip("no compiled reference for %s" % case["name"])
    want = _want(want_cache, cid)
    ref = SC.expected(case, lib=R.RefLib(case["name"]))
    for k, (a, b) in enumerate(zip(want, ref)):
        np.testing.assert_array_equal(a[0], b[0], err_msg="%s: oracle vs reference, field %d" % (cid, k))
        assert a[1:] == b[1:], "%s: oracle vs reference state, field %d" % (cid, k)


@pytest.mark.parametrize("cid", SC.CASE_IDS)
def test_case_can_tell_a_set_boundary(want_cache, cid):
    """the fields as ONE long set differ from the per-set expectation in a picture of every set after the first, and in a state"""
    case = SC.case(cid)
    want = _want(want_cache, cid)
    one = SC.expected_one_long_set(case)
    for s, (lo, hi) in enumerate(SC.sets_of(case)):
        same = all(np.array_equal(want[k][0], one[k][0]) for k in range(lo, hi))
        if s == 0:
            assert same and all(want[k][1:] == one[k][1:] for k in range(lo, hi)), "set 0 is the start of the long set"
        else:
            assert not same, "%s: set %d has the pictures of one long set -- the case cannot see its boundary" % (cid, s)
    assert any(a[1:] != b[1:] for a, b in zip(want, one)), "%s: no state differs from one long set" % cid


def _fold_model(case, s, want, wrong):
    """numpy model of the fold over set s: v_k[row] = blend(new_k[row], f(v_{k-1})[src]) on the rows field k writes,
    f(v_{k-1})[row] elsewhere; src = the first row of the line that wrote `row` (wrong: `row` itself).  new_k and the lines come
    from the oracle decoding field k WITHOUT blend from the state the set is in before it."""
    lo, hi = SC.sets_of(case)[s]
    fr, par, dco = SC.frames(case), SC.parities(case), SC.dot_crawl(case)
    inc = SC.incoming(case)[s]
    orc = R.Oracle(case["name"])
    bpp = R.bpp4fmt(case["ofmt"])
    assert bpp == 3, "the model blends every byte (RGB / BGR)"
    outh, pitch = case["outh"], case["outw"] * bpp
    v = SC.init_of_set(case, SC.init_pictures(case), s).reshape(outh, pitch).copy()
    pics = []
    for k in range(lo, hi):
        c = orc.new_crt(case["outw"], case["outh"], case["ofmt"])
        for a, val in case["knobs"].items():
            c.set(a, val)
        c.set("blend", 0)
        before = inc if k == lo else want[k - 1][1:]
        pad, kw, d = SC.field_settings(case, fr[k], par[k], dco[k])
        c.settings(pad, **kw)
        c.modulate()
        c.set("hsync", before[0])
        c.set("vsync", before[1])
        c.set("rn", before[2])
        c.demodulate(case["noise"], trace=True)
        new = c.out.reshape(outh, pitch)
        old = v if case["mode"] == "keep" else SC.display_step_np(v, case["ofmt"], case["mode"])
        v = old.copy()
        for valid, _pos, _w0, _w1, beg, end, _hs, _dx, _sc in c.trace:
            if valid != 1:
                continue
            for row in [beg] + list(range(beg + 1, end - case["knobs"].get("scanlines", 0))):
                if row < outh:
                    v[row] = (new[row] >> 1) + (old[row if wrong else beg] >> 1)
        pics.append(v.reshape(-1).copy())
    return pics


def test_blend_case_has_the_cross_row_dependency(want_cache):
    """scanlines 0 at 832x624: a line writes several rows and the old value is taken at the line's first row.  The model with that
    rule reproduces the oracle; the model that takes the old value at `row` does not -- the case would catch a fold by rows."""
    case = SC.case(SC.DUPROWS)
    want = _want(want_cache, SC.DUPROWS)
    s = 3
    lo, hi = SC.sets_of(case)[s]
    right = _fold_model(case, s, want, wrong=False)
    for k in range(lo, hi):
        np.testing.assert_array_equal(right[k - lo], want[k][0], err_msg="fold model, field %d" % k)
    wrong = _fold_model(case, s, want, wrong=True)
    assert any(not np.array_equal(wrong[k - lo], want[k][0]) for k in range(lo, hi)), "a fold by rows gives the same pictures"


def test_noisy_case_needs_different_numbers_of_passes(want_cache):
    """noise 120: the sets' sync chains need different numbers of fixed-point passes (the joint fixed point runs the maximum)"""
    case = SC.case(SC.NOISY)
    want = _want(want_cache, SC.NOISY)
    passes = [SC.sync_passes_of_set(case, s, want) for s in range(len(SC.sets_of(case)))]
    print("passes per set:", passes)
    assert len(set(passes)) > 1, passes
    assert max(passes) <= max(hi - lo for lo, hi in SC.sets_of(case)) + 1

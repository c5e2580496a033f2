"""CPU checks around CRTHIP_F_VHS_SET_STREAMS (one rand() stream per set in crthip_sequence_sets on the stock VHS build; the GPU side
is tests/test_gpu_vhs_sets.py): the flag's value and what crthip_params_finalize says to it, and the cases of tests/vhs_sets_cases.py
-- their expected values are the reference's, every case can tell per-set streams from one stream, and no case runs into the
reference's undefined over-read on a line of the contract."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crtref as R
import vhs_sets_cases as VC

ALL_IDS = VC.CASE_IDS + VC.KNOB_CASE_IDS


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    R.build_oracle()


@pytest.fixture(scope="module")
def want_cache():
    return {}


def _want(cache, cid):
    """per-set loops of the oracle with check_reads: without aberration no field of any case may read past inp[] + 16; with
    do_aberration the last lines lose their sync pulse, and exactly the lines that start inside the last VC.ABERRATION_ROWS = 12
    output rows are exempt (those rows are not compared on the GPU either) -- nothing else"""
    if cid not in cache:
        cache[cid] = VC.expected(VC.case(cid), check_reads=True)
    return cache[cid]


@pytest.fixture(scope="module")
def crtlib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def test_flag_value_and_finalize(crtlib):
    """0x20000 in the header and in crtlib, ABI version still 6; crthip_params_finalize refuses the flag on NTSC and together with
    CRTHIP_F_VHS_LCG_NOISE (as it refuses CRTHIP_F_VHS_LP on another system) and accepts it on the stock VHS build"""
    hdr = open(os.path.join(R.ROOT, "include", "crt_hip.h")).read()
    assert int(re.search(r"#define\s+CRTHIP_F_VHS_SET_STREAMS\s+(\S+)", hdr).group(1), 0) == 0x20000 == crtlib.F_VHS_SET_STREAMS
    assert int(re.search(r"#define\s+CRTHIP_ABI_VERSION\s+(\d+)", hdr).group(1)) == 6
    assert crtlib.load_library().crthip_abi_version() == 6
    others = [getattr(crtlib, a) for a in dir(crtlib) if a.startswith("F_") and a != "F_VHS_SET_STREAMS"]
    assert not any(crtlib.F_VHS_SET_STREAMS & v for v in others) and not crtlib.F_VHS_SET_STREAMS & (7 << 8)
    geo = dict(w=VC.W, h=VC.H, outw=VC.OUTW, outh=VC.OUTH)
    with pytest.raises(ValueError):
        crtlib.make_params("ntsc", flags=crtlib.F_VHS_SET_STREAMS, **geo)
    with pytest.raises(ValueError):
        crtlib.make_params("vhslcg", flags=crtlib.F_VHS_SET_STREAMS, **geo)
    with pytest.raises(ValueError):
        crtlib.make_params("vhs", flags=crtlib.F_VHS_SET_STREAMS | crtlib.F_VHS_LCG_NOISE, **geo)
    with pytest.raises(ValueError):
        crtlib.make_params("ntsc", flags=crtlib.F_VHS_LP, **geo)                     # the model
    for extra in (0, crtlib.F_VHS_DRAW_ABERRATION, crtlib.F_VHS_LP, crtlib.F_PHOSPHOR_FADE):
        p = crtlib.make_params("vhs", flags=crtlib.F_VHS_SET_STREAMS | extra, **geo)
        assert p.flags & crtlib.F_VHS_SET_STREAMS
    # the flag changes nothing else of the blob
    a, b = crtlib.make_params("vhs", **geo), crtlib.make_params("vhs", flags=crtlib.F_VHS_SET_STREAMS, **geo)
    b.flags &= ~crtlib.F_VHS_SET_STREAMS
    assert bytes(a) == bytes(b)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_no_case_reads_past_the_field(want_cache, cid):
    """crtref.reads_past_inp is asserted inside the per-set loops (see _want for the one cap, the 12 rows of do_aberration); the
    tables hold what the issue asks for: a set of one field, a one-field set directly behind a longer one, unequal lengths, at
    most 12 fields, seeds and incoming pairs that differ from set to set"""
    case = VC.case(cid)
    want, nxt = _want(want_cache, cid)
    assert len(want) == VC.n_fields(case) <= 12 and len(nxt) == len(VC.sets_of(case))
    lens = [hi - lo for lo, hi in VC.sets_of(case)]
    assert lens[0] == 1 and any(a > 1 and b == 1 for a, b in zip(lens, lens[1:])) and len(set(lens)) > 2
    assert len(set(VC.seeds(case))) == len(lens) and len(set(VC.incoming(case))) == len(lens)
    assert len(set(v for _h, v in VC.incoming(case))) == len(lens)      # (crt_modulate of the VHS build resets hsync: vsync is what arrives)
    if case["aberration"]:
        assert all(6 <= w[4] <= 17 for w in want), "aberration heights are (rand() % 12) - 8 + 14"
        assert len(set(w[4] for w in want)) > 2


@pytest.mark.parametrize("cid", ALL_IDS)
def test_oracle_equals_reference_per_set(want_cache, cid):
    """the compiled reference under its own srand on the same per-set loops: pictures (all rows but the cap's), states, and where
    the stream stands after every set"""
    if not R.have_ref("vhs"):
        pytest.skip("no compiled reference for vhs")
    case = VC.case(cid)
    want, nxt = _want(want_cache, cid)
    ref, ref_nxt = VC.expected(case, lib=R.RefLib("vhs"))
    keep = VC.kept_rows(case) * VC.OUTW * 4
    for k, (a, b) in enumerate(zip(want, ref)):
        np.testing.assert_array_equal(a[0][:keep], b[0][:keep], err_msg="%s: oracle vs reference, field %d" % (cid, k))
        assert a[1:4] == b[1:4], "%s: oracle vs reference state, field %d" % (cid, k)
    assert nxt == ref_nxt


@pytest.mark.parametrize("cid", ALL_IDS)
def test_case_can_tell_per_set_streams(want_cache, cid):
    """the same fields as one long set under ONE stream from set 0's seed differ from the per-set loops in at least one rn and one
    picture (rows of the contract) of every set after the first; set 0 is the start of that stream"""
    case = VC.case(cid)
    want, _ = _want(want_cache, cid)
    one = VC.expected_one_stream(case)
    keep = VC.kept_rows(case) * VC.OUTW * 4
    for s, (lo, hi) in enumerate(VC.sets_of(case)):
        same_pic = all(np.array_equal(want[k][0][:keep], one[k][0][:keep]) for k in range(lo, hi))
        same_rn = all(want[k][3] == one[k][3] for k in range(lo, hi))
        if s == 0:
            assert same_pic and all(want[k][1:] == one[k][1:] for k in range(lo, hi)), "set 0 is the start of the one stream"
        else:
            assert not same_pic, "%s: set %d has the pictures of one stream -- the case cannot see its own" % (cid, s)
            assert not same_rn, "%s: set %d has the rn of one stream" % (cid, s)


def test_generator_model_matches_libc():
    """what the GPU test compares the history array with: after srand(seed) and k calls, the next rand() is ((y[k] + y[k+28]) mod
    2^32) >> 1 of the 31-word history crthip_vhs_history_from_seed gives, advanced by y[n] = y[n-31] + y[n-3]"""
    import __graft_entry__ as g
    g.build()
    import crtlib
    L = crtlib.load_library()
    libc = C.CDLL(None)
    for seed in VC.SEEDS:
        buf = (C.c_uint * 31)()
        assert L.crthip_vhs_history_from_seed(C.c_uint(seed), buf) == 0
        y = [int(v) for v in buf]
        libc.srand(C.c_uint(seed))
        for k in range(100):
            nxt = (y[k] + y[k + 28]) & 0xffffffff
            assert nxt >> 1 == libc.rand(), (seed, k)
            y.append(nxt)

"""CPU checks of sequence mode with per-field knobs (crthip_sequence_knobs / crthip_sequence_sets_knobs / crthip_seq_bind_knobs,
include/crt_hip.h; the GPU side is tests/test_gpu_seqknobs.py): the ABI additions, and the yardstick of the GPU tests -- the oracle
driven field by field on one CRT (tests/seqknobs_cases.py) -- against the same loop on the compiled reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crtref as R
import seqknobs_cases as SK


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    R.build_oracle()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


NEW_SYMBOLS = {"crthip_sequence_knobs": 12, "crthip_sequence_sets_knobs": 14, "crthip_seq_bind_knobs": 3}


def test_new_symbols_and_their_argument_counts(lib):
    """exported by the library, declared in the header with the argument counts of the issue, bound by crtlib with as many"""
    L = lib.load_library()
    with open(os.path.join(R.ROOT, "include", "crt_hip.h")) as f:
        header = f.read()
    for sym, nargs in NEW_SYMBOLS.items():
        assert hasattr(L, sym), sym
        m = re.search(r"int\s+%s\(([^;]*)\);" % sym, header)
        assert m, sym + " is not declared in crt_hip.h"
        decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(decl.split(",")) == nargs, (sym, decl)
        assert len(getattr(L, sym).argtypes) == nargs, sym
    for meth in ("sequence_knobs", "sequence_sets_knobs", "seq_bind_knobs"):
        assert callable(getattr(lib.CRT, meth))


def test_abi_version_is_still_6(lib):
    """purely additive: a host finds the new entry points by their presence (tests/test_knobs_cpu.py, test_abi_additions)"""
    assert lib.load_library().crthip_abi_version() == 6
    with open(os.path.join(R.ROOT, "include", "crt_hip.h")) as f:
        assert re.search(r"#define\s+CRTHIP_ABI_VERSION\s+6\b", f.read())


@pytest.mark.parametrize("cid", SK.CASE_IDS)
def test_no_field_of_any_gpu_case_is_inside_the_reference_over_read(cid):
    """the GPU tests exclude NO field: every field of every case must stay clear of the reference's undefined over-read"""
    for k, w in enumerate(SK.expected(SK.case(cid))):
        assert w["undefined"] is False, "%s field %d falls under the reference-UB exclusion: choose other knobs" % (cid, k)


def test_case_tables_say_what_the_gpu_tests_rely_on():
    six = SK.case("six")
    noise = [t[0] for t in six["triples"]]
    assert len(six["triples"]) == 6 and 0 in noise[1:-1] and len(set(six["triples"])) == 6
    sats = sorted(abs(t[2]) for t in six["triples"])
    assert sats[0] <= 13 and sats[-1] >= 900                         # both sides of tier 0's chroma bound, the exact tier
    assert [b - a for a, b in SK.sets_of(SK.case("sets"))] == [1, 4, 2]
    seventy = SK.case("seventy")
    assert SK.n_fields(seventy) == 70 and len(set(seventy["triples"])) == 70
    for cid in ("six-blend", "six-blend-fade", "six-blend-clear", "sets-blend-fade"):
        c = SK.case(cid)
        orc = R.Oracle(c["name"])
        assert c["geo"]["outh"] == orc.sys.vres, "the smallest outh the blend rule accepts (outh + v_fac >= CRT_LINES)"


def test_the_six_field_case_needs_more_than_two_sync_passes():
    """from the oracle alone: the joint fixed point over the six fields with their knobs stops after more than two passes, so the
    kernels re-read the records on a pass behind the first two (the GPU test asserts the library's own count)"""
    c = SK.case("six")
    assert SK.sync_passes(c, SK.expected(c)) > 2


@pytest.mark.parametrize("cid", SK.CASE_IDS)
def test_oracle_loop_against_the_compiled_reference(cid):
    """the yardstick itself: the oracle's loop and the same loop on the reference agree in every picture and state"""
    case = SK.case(cid)
    if not R.have_ref(case["name"]):
        pytest.skip("oracle/_ref not built")
    ref = SK.expected(case, R.RefLib(case["name"]))
    orc = SK.expected(case)
    assert len(ref) == len(orc) == SK.n_fields(case)
    for k, (a, b) in enumerate(zip(ref, orc)):
        tag = "%s field %d" % (cid, k)
        assert (a["hsync"], a["vsync"], a["rn"]) == (b["hsync"], b["vsync"], b["rn"]), tag
        np.testing.assert_array_equal(a["ccf"], b["ccf"], err_msg=tag + " ccf")
        np.testing.assert_array_equal(a["out"], b["out"], err_msg=tag + " out")


def test_structs_reused_from_the_field_pass_knobs(lib):
    assert (C.sizeof(lib.Knobs), C.sizeof(lib.KnobRec), C.sizeof(lib.KnobsEnv)) == (16, 32, 32)

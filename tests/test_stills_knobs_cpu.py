"""CPU checks of stills with one look per still (crthip_stills_knobs, include/crt_hip.h; the GPU side is
tests/test_gpu_stills_knobs.py): the expected values of tests/stills_knobs_cases.py against the compiled reference, no chosen case
inside the reference's undefined over-read, what the case tables promise, and the ABI addition."""
import os
import re
import subprocess

import numpy as np
import pytest

import crtref as R
import levels_cases as LV
import stills_cases as SC
import stills_knobs_cases as SKC


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    R.build_oracle()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def _header():
    with open(os.path.join(R.ROOT, "include", "crt_hip.h")) as f:
        return f.read()


def test_library_exports_the_entry_point(lib):
    L = lib.load_library()
    assert hasattr(L, "crthip_stills_knobs")
    assert len(L.crthip_stills_knobs.argtypes) == 12
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(R.PKG_LIB, "libcrthip.so")], capture_output=True, text=True, check=True).stdout
    assert "crthip_stills_knobs" in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_declares_it_and_the_abi_version_is_still_6(lib):
    header = _header()
    m = re.search(r"int\s+crthip_stills_knobs\(([^;]*)\);", header)
    assert m, "crthip_stills_knobs is not declared in crt_hip.h"
    decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert len(decl.split(",")) == 12, decl
    assert re.search(r"#define\s+CRTHIP_ABI_VERSION\s+6\b", header)
    assert lib.load_library().crthip_abi_version() == 6
    assert "knobs in crthip_stills" not in header                  # the HUE KNOB paragraph's out-of-scope list lost it


def test_binding_has_the_method(lib):
    import inspect
    assert callable(lib.CRT.stills_knobs)
    assert list(inspect.signature(lib.CRT.stills_knobs).parameters) == ["self", "s", "knobs", "interlaced", "first_field", "frames",
                                                                         "schedule", "params"]


def test_a_c89_program_sees_the_prototype(tmp_path):
    src, exe = str(tmp_path / "stills_knobs_proto.c"), str(tmp_path / "stills_knobs_proto")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "crt_hip.h"\n'
                'typedef int (*fn_t)(crthip_ctx *, const crthip_params *, int, const void *, size_t, void *, size_t, crthip_state *, int,\n'
                '                    const crthip_pass *, const crthip_knob_rec *, const crthip_knobs_env *);\n'
                'int main(void) { fn_t f = crthip_stills_knobs; printf("%d %d\\n", f != 0, CRTHIP_ABI_VERSION); return 0; }\n')
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(R.ROOT, "include"), "-o", exe, src,
                    "-L" + R.PKG_LIB, "-lcrthip", "-Wl,-rpath," + R.PKG_LIB, "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["1", "6"]


@pytest.mark.parametrize("cid", SKC.CASE_IDS)
def test_no_case_reads_past_the_field(cid):
    """R.reads_past_inp must not hold for any pass of any still of any case (asserted inside the loop): nothing is excluded on the
    GPU.  The traced run gives the values every other test uses."""
    case = SKC.case(cid)
    traced = SKC.expected(case, check_reads=True)
    want = SKC.expected(case)
    assert len(traced) == len(want) == case["n"]
    for a, b in zip(traced, want):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1:4] == b[1:4]
    assert 1 <= len(case["sched"]) <= 64
    if SKC.noise_max(case) == 0 and case["n"] > 1:
        assert len(SC.distinct_entries(case)) < len(case["sched"]), "%s: a noise-0 case should share at least one encoding" % cid


@pytest.mark.parametrize("cid", SKC.CASE_IDS)
def test_oracle_equals_reference(cid):
    """the same loop driving the compiled reference library: every case"""
    case = SKC.case(cid)
    if not R.have_ref(case["name"]):
        pytest.skip("no compiled reference for %s" % case["name"])
    want = SKC.expected(case)
    ref = SKC.expected(case, lib=R.RefLib(case["name"]))
    for k, (a, b) in enumerate(zip(want, ref)):
        np.testing.assert_array_equal(a[0], b[0], err_msg="%s: oracle vs reference, still %d" % (cid, k))
        assert a[1:4] == b[1:4], "%s: oracle vs reference state, still %d" % (cid, k)
        np.testing.assert_array_equal(a[4], b[4], err_msg="%s: oracle vs reference ccf, still %d" % (cid, k))


def test_case_tables_say_what_the_gpu_tests_rely_on(lib):
    cases = SKC.CASES
    assert {c["n"] for c in cases} == {1, 5, 6}
    assert {SKC.width(c) for c in cases} == {3, 5, 7, 8}
    scheds = [c["sched"] for c in cases]
    for s in (SKC.INTERLACED0, SKC.INTERLACED1, SKC.PROGRESSIVE, SKC.CUSTOM5):
        assert s in scheds
    assert {c["name"] for c in cases} >= {"ntsc", "ntscbloom", "ntscfir7", "snes", "temp", "nes", "vhslcg", "vhs"}
    assert all(SKC.width(c) == 5 for c in cases if c["name"] == "nes")
    # the noise mixes: all clean, one noisy still among clean ones, all above 0
    mixes = [sorted(r[0] for r in c["rows"]) for c in cases]
    assert any(m[-1] == 0 for m in mixes) and any(m[0] > 0 for m in mixes)
    assert any(m[-1] > 0 and m[-2] == 0 and len(m) > 2 for m in mixes)
    # saturation on both sides of tier 0's chroma bound, one still in the 24-bit tier beside tier 0 neighbours
    sats = sorted(abs(r[2]) for r in SKC.SAT_ROWS)
    assert sats[0] <= 13 and sats[-1] >= 900
    p = lib.make_params("ntsc", w=64, h=48, outw=160, outh=120, format=lib.FMT_BGRA, out_format=lib.FMT_BGRA)
    recs, env = lib.knobs_prepare(p, np.array(SKC.PIC_ROWS))
    floors = [int(r[7]) for r in recs]
    assert sorted(floors) == [0, 0, 0, 0, 2], floors
    assert p.desth % 64 != 0 and p.desth > 64, "a wavefront of 64 rows holds rows of two stills"
    # (white, ire_base) on the last fast values and on the first outside, of both signs
    lv = {which: [LV.levels_of("ntsc", r) for r in SKC.bound_rows(which)] for which in ("inside", "white+", "white-", "ire+", "ire-")}
    assert {8191, -8191} <= {w for w, _ in lv["inside"]} and {8191, -8191} <= {b for _, b in lv["inside"]}
    assert max(abs(w) for w, _ in lv["inside"]) == 8191 and max(abs(b) for _, b in lv["inside"]) == 8191
    assert [w for w, _ in lv["white+"] if abs(w) > 8191] == [8192] and [w for w, _ in lv["white-"] if abs(w) > 8191] == [-8192]
    assert [b for _, b in lv["ire+"] if abs(b) > 8191] == [8192] and [b for _, b in lv["ire-"] if abs(b) > 8191] == [-8192]
    for which in lv:
        assert any([r[1:] for r in c["rows"]] == [r[1:] for r in SKC.bound_rows(which)] for c in cases), which
    hues = {r[7] for c in cases if SKC.width(c) == 8 for r in c["rows"]}
    assert {0, -123, 405, 359} <= hues
    # blend 1 and 0, a phosphor mode, duplicated rows, the aberration band, one seed per still
    assert {c["knobs"].get("blend") for c in cases} == {0, 1} and any(c["mode"] == "fade" for c in cases)
    assert any(c["outh"] > 240 and c["knobs"].get("scanlines") == 0 for c in cases) and any(c["outh"] < 240 for c in cases)
    assert any(c["name"] == "vhslcg" and any(e[2] for e in c["sched"]) for c in cases)
    vhs = SKC.case("vhs-rand-levels")
    assert len(set(vhs["seeds"][:vhs["n"]])) == vhs["n"]
    assert any(len(c["configs"]) >= 6 and {cfg[2] for cfg in c["configs"]} == {0, 1} and {cfg[1] for cfg in c["configs"]} == {0, 1} for c in cases)

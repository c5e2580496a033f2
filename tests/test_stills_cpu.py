"""CPU checks of the stills mode (crthip_stills, include/crt_hip.h; the GPU side is tests/test_gpu_stills.py): the schedule helper
against a literal transcription of crt_main.c:241-255, the expected values of tests/stills_cases.py against the compiled reference
and the reference's own `ntsc` program, no chosen case inside the reference's undefined over-read, and the ABI additions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import crtref as R
import stills_cases as SC


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    R.build_oracle()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


@pytest.mark.parametrize("interlaced", [0, 1])
@pytest.mark.parametrize("first_field", [0, 1])
@pytest.mark.parametrize("n_frames", [1, 2, 3, 4])
def test_schedule_is_the_loop_of_crt_main(lib, interlaced, first_field, n_frames):
    want = SC.cli_schedule(interlaced, first_field, n_frames)
    assert len(want) == (2 * n_frames if interlaced else n_frames)
    assert lib.stills_schedule(bool(interlaced), first_field, n_frames) == want
    buf = (lib.Pass * 64)()
    L = lib.load_library()
    assert L.crthip_stills_schedule(interlaced, first_field, n_frames, buf, 64) == len(want)
    assert [(buf[r].field, buf[r].frame, buf[r].aux, buf[r].reserved) for r in range(len(want))] == [e + (0,) for e in want]


def test_schedule_of_the_cli_by_value(lib):
    """what the header documents: four distinct entries, each used twice; progressive: one entry four times"""
    assert lib.stills_schedule() == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 0)]
    assert lib.stills_schedule(interlaced=False) == [(0, 0, 0)] * 4
    assert lib.stills_schedule(interlaced=False, first_field=1) == [(1, 0, 0)] * 4
    assert lib.stills_schedule(first_field=3) == lib.stills_schedule(first_field=1)


def test_schedule_capacity_and_argument_errors(lib):
    L = lib.load_library()
    buf = (lib.Pass * 64)()
    assert L.crthip_stills_schedule(1, 0, 4, buf, 8) == 8
    assert L.crthip_stills_schedule(1, 0, 4, buf, 7) == -1          # does not fit
    assert L.crthip_stills_schedule(0, 0, 4, buf, 3) == -1
    assert L.crthip_stills_schedule(0, 0, 4, buf, 4) == 4
    assert L.crthip_stills_schedule(1, 0, 4, None, 8) == -1
    assert L.crthip_stills_schedule(1, 0, 0, buf, 64) == -1
    assert L.crthip_stills_schedule(1, 0, -2, buf, 64) == -1
    assert L.crthip_stills_schedule(1, 0, 32, buf, 64) == 64         # CRTHIP_STILLS_MAX_PASSES
    assert L.crthip_stills_schedule(1, 0, 33, buf, 1000) == -1
    assert L.crthip_stills_schedule(0, 0, 65, buf, 1000) == -1
    with pytest.raises(ValueError):
        lib.stills_schedule(frames=0)


def test_abi_additions(lib, tmp_path):
    """sizeof(crthip_pass) == 16 on both sides, the symbols are exported, the ABI version did not move"""
    assert C.sizeof(lib.Pass) == 16
    L = lib.load_library()
    for sym in ("crthip_stills_schedule", "crthip_stills_reserve", "crthip_stills"):
        assert hasattr(L, sym), sym
    assert L.crthip_abi_version() == 6
    src, exe = str(tmp_path / "stills_sizeof.c"), str(tmp_path / "stills_sizeof")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "crt_hip.h"\nint main(void) { printf("%d %d\\n", (int) sizeof(crthip_pass), '
                'CRTHIP_STILLS_MAX_PASSES); return 0; }\n')
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(R.ROOT, "include"), "-o", exe, src], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["16", "64"]


@pytest.mark.parametrize("cid", SC.CASE_IDS)
def test_no_case_reads_past_the_field(cid):
    """R.reads_past_inp must not hold for any pass of any still of any case (asserted inside the loop): nothing is excluded on the
    GPU.  The traced run gives the values every other test uses."""
    case = SC.case(cid)
    traced = SC.expected(case, check_reads=True)
    want = SC.expected(case)
    assert len(traced) == len(want) == case["n"]
    for a, b in zip(traced, want):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1:4] == b[1:4]
    assert 1 <= len(case["sched"]) <= 64
    if case["noise"] == 0:
        assert len(SC.distinct_entries(case)) < len(case["sched"]), "%s: a noise-0 case should share at least one encoding" % cid


@pytest.mark.parametrize("cid", [c["id"] for c in SC.CASES if SC.sysid(c) in (R.SYS_NTSC, R.SYS_VHS)])
def test_oracle_equals_reference(cid):
    """the transcribed loop driving the compiled reference library, every NTSC / VHS case"""
    case = SC.case(cid)
    if not R.have_ref(case["name"]):
        pytest.skip("no compiled reference for %s" % case["name"])
    want = SC.expected(case)
    ref = SC.expected(case, lib=R.RefLib(case["name"]))
    for k, (a, b) in enumerate(zip(want, ref)):
        np.testing.assert_array_equal(a[0], b[0], err_msg="%s: oracle vs reference, still %d" % (cid, k))
        assert a[1:4] == b[1:4], "%s: oracle vs reference state, still %d" % (cid, k)
        np.testing.assert_array_equal(a[4], b[4], err_msg="%s: oracle vs reference ccf, still %d" % (cid, k))


@pytest.mark.parametrize("flags,interlaced", [("-op", False), ("-o", True)])
def test_oracle_equals_the_reference_program(tmp_path, flags, interlaced):
    """the reference's own `ntsc` driver on one generated PPM against the oracle's still of the same image"""
    exe = os.path.join(R.REF_DIR, "ntsc_cli")
    if not os.path.exists(exe):
        pytest.skip("no compiled reference driver")
    w, h, outw, outh = 80, 60, 160, 120
    bgra = R.synth_image(w, h, 4, 4711)
    bgra[:, :, 3] = 0                                              # ppm_read24: 0x00RRGGBB
    src, dst = str(tmp_path / "in.ppm"), str(tmp_path / "out.ppm")
    SC.write_ppm(src, bgra[:, :, 2::-1])
    subprocess.run([exe, flags, str(outw), str(outh), "0", "0", src, dst], check=True, capture_output=True)
    want = SC.cli_still(R.Oracle("ntsc"), bgra, outw, outh, 0, interlaced=interlaced)
    with open(dst, "rb") as f:
        got = f.read()
    head = b"P6\n%d %d\n255\n" % (outw, outh)
    assert got[:len(head)] == head
    np.testing.assert_array_equal(np.frombuffer(got[len(head):], dtype=np.uint8), want.reshape(-1))

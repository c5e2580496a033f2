"""Mixed image sizes with one look per field, host side (no GPU): the declarations and exports of crthip_fieldpass_sizes_knobs /
crthip_stills_sizes_knobs, the pin of tests/sizes_knobs_cases.py's checker loop to the REAL reference (oracle/_ref) on every case at
tolerance 0 with no field left out, the Python argument checks and the --looks file of tools/stills_dir.py."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import crtref as R
import sizes_cases as SC
import sizes_knobs_cases as ZK


@pytest.fixture(scope="module")
def crtlib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(g.PKG, "lib", "libcrthip.so")):
        g.build()
    import crtlib
    crtlib.load_library()
    return crtlib


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("stills_dir", os.path.join(R.ROOT, "tools", "stills_dir.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CLI = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]


def test_abi_additions(crtlib, tmp_path):
    """the header declares both functions with the issue's signatures (a C89 program takes their addresses through typed pointers),
    the library exports them, and the ABI version stays 6"""
    L = crtlib.load_library()
    src, exe = str(tmp_path / "sk_decl.c"), str(tmp_path / "sk_decl")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "crt_hip.h"\n'
                'typedef int (*fp_t)(crthip_ctx *, const crthip_params *, int, const void *, void *, size_t, crthip_state *,\n'
                '                    const crthip_size_rec *, const crthip_sizes_env *, const crthip_knob_rec *, const crthip_knobs_env *);\n'
                'typedef int (*st_t)(crthip_ctx *, const crthip_params *, int, const void *, void *, size_t, crthip_state *, int,\n'
                '                    const crthip_pass *, const crthip_size_rec *, const crthip_sizes_env *, const crthip_knob_rec *,\n'
                '                    const crthip_knobs_env *);\n'
                'int main(void) { fp_t a = crthip_fieldpass_sizes_knobs; st_t b = crthip_stills_sizes_knobs;\n'
                '    printf("%d %d\\n", CRTHIP_ABI_VERSION, a != 0 && b != 0); return 0; }\n')
    lib = os.path.join(R.ROOT, "ntsc-crt_amd", "lib")
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(R.ROOT, "include"), "-o", exe, src,
                    "-L" + lib, "-lcrthip", "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["6", "1"]
    assert L.crthip_abi_version() == 6
    for sym in ("crthip_fieldpass_sizes_knobs", "crthip_stills_sizes_knobs"):
        assert hasattr(L, sym), sym
    assert hasattr(crtlib.CRT, "fieldpass_sizes_knobs") and hasattr(crtlib.CRT, "stills_sizes_knobs")


def test_case_tables_cover_what_they_claim():
    """the coverage list of the case module, asserted: row widths, path-switch widths, the level bound, hues, clean and mixed noise"""
    widths = {len(c["rows"][0]) for c in ZK.CASES.values()}
    assert widths == {3, 5, 7, 8}
    for case, c in ZK.CASES.items():
        assert len(c["rows"]) == len(ZK.base(case)["sizes"]), case
        assert len({len(r) for r in c["rows"]}) == 1, case
    ws = {w for case in ("narrow8", "tiles8", "wide_mixed8") for w, _ in ZK.base(case)["sizes"]}
    assert {1, 3, 4, 7, 8, 15, 16, 17, 1279, 1280} <= ws
    import levels_cases as LV
    for case, col, val in (("bound_white", 0, 8192), ("bound_ire", 1, -8192)):
        lv = [LV.levels_of("ntsc", r) for r in ZK.rows8(case)]
        assert sum(1 for x in lv if abs(x[0]) >= 8192 or abs(x[1]) >= 8192) == 1 and val in [x[col] for x in lv], case
    hs = {r[7] for r in ZK.rows8("hues")} | {r[7] for r in ZK.rows8("tiles8")}
    assert {360, -360} <= hs and any(h < 0 for h in hs)
    assert ZK.noise_max("clean8") == 0 and ZK.noise_max("clean3") == 0 and ZK.noise_max("stills_clean") == 0
    assert sorted(r[0] for r in ZK.CASES["one_noisy"]["rows"])[-2:] == [0, 24]
    assert all(r[5:7] == (0, 100) for r in ZK.rows8("hue_only"))
    buf, sizes = ZK.layout("one_image")
    assert (sizes[:, 2] == 0).all() and len(set(map(tuple, sizes))) == 1 and len(set(ZK.CASES["one_image"]["rows"])) == len(sizes)
    assert {ZK.base(c)["name"] for c in ZK.CASES} >= {"vhs", "vhslcg", "snes", "temp", "nesrgb", "ntscp0", "ntscbloom", "ntscfir7"}
    assert len(ZK.CASES["many"]["rows"]) == 520


@pytest.mark.skipif(not R.have_ref("ntsc"), reason="oracle/_ref not built (no reference sources on this machine)")
@pytest.mark.parametrize("case", sorted(ZK.CASES))
def test_checker_loop_equals_the_reference(case):
    """the loop the GPU tests compare with IS the reference's: every case, every field, every pass, tolerance 0; no field falls into
    the reference's undefined over-read (crtref.reads_past_inp) -- the count of left-out fields is asserted to be 0"""
    name = ZK.base(case)["name"]
    assert R.have_ref(name), "no reference build of " + name
    sched = CLI if case.startswith("stills") else None
    got = ZK.checker_fields(R.Oracle(name), case, schedule=sched)
    want = ZK.checker_fields(R.RefLib(name), case, schedule=sched)
    undefined = 0
    for k, (g, w) in enumerate(zip(got, want)):
        for step, (a, b) in enumerate(zip(g, w)):
            tag = "%s field %d pass %d" % (case, k, step)
            undefined += bool(a["undefined"])
            for key in ("inp", "out", "ccf"):
                np.testing.assert_array_equal(a[key], b[key], err_msg=tag + " " + key)
            assert (a["hsync"], a["vsync"], a["rn"]) == (b["hsync"], b["vsync"], b["rn"]), tag
    assert undefined == 0, "%s: %d field-passes inside the reference's undefined over-read -- choose other inputs, exclude nothing" % (case, undefined)


class _NoGpuCRT:
    """CRT's argument checks run before anything reaches the library: an object with the attributes they read, and none of the rest"""

    def __init__(self, crtlib, n):
        self.n, self.L = n, crtlib.load_library()
        self.size_recs = self.knob_recs = None
        self.touched = []

    def upload_sizes(self, images, p):
        self.touched.append("sizes")

    def upload_knobs(self, knobs, p):
        self.touched.append("knobs")


def test_python_argument_checks(crtlib):
    """a length mismatch between images and looks, or between either and the batch, raises ValueError before any upload; None for
    either without an earlier upload raises too"""
    check = crtlib.CRT._sizes_knobs_upload
    sizes = np.array([(8, 8, 0), (4, 4, 256), (5, 5, 512)])
    for n, images, knobs in ((3, (None, sizes), np.zeros((2, 8), dtype=np.int32)),
                             (3, [0, 1], np.zeros((3, 3), dtype=np.int32)),
                             (4, (None, sizes), np.zeros((3, 5), dtype=np.int32)),
                             (4, None, np.zeros((3, 7), dtype=np.int32)),
                             (4, [0, 1, 2], None)):
        fake = _NoGpuCRT(crtlib, n)
        with pytest.raises(ValueError):
            check(fake, images, knobs, None, "fieldpass_sizes_knobs")
        assert fake.touched == [], "nothing reaches the library before the counts agree"
    fake = _NoGpuCRT(crtlib, 3)
    with pytest.raises(ValueError, match="no sizes uploaded"):
        check(fake, None, np.zeros((3, 8), dtype=np.int32), None, "fieldpass_sizes_knobs")
    fake = _NoGpuCRT(crtlib, 3)
    with pytest.raises(ValueError, match="no knobs uploaded"):
        fake.size_recs = object()
        check(fake, (None, sizes), None, None, "stills_sizes_knobs")
    fake = _NoGpuCRT(crtlib, 3)
    fake.size_recs = fake.knob_recs = object()
    check(fake, (None, sizes), np.zeros((3, 8), dtype=np.int32), None, "stills_sizes_knobs")
    assert fake.touched == ["sizes", "knobs"]


def test_looks_file_parser(tool, tmp_path):
    names = ["a.ppm", "b.ppm", "c.ppm"]
    path = tmp_path / "looks.txt"
    path.write_text("# name noise mon_hue saturation brightness contrast black_point white_point hue\n"
                    "c.ppm 0 10 12 -3 200 4 90 -450\n\n"
                    "a.ppm -5 0 10 0 180 0 100 33\n"
                    "b.ppm 24 -20 900 7 120 -6 115 360\n")
    looks = tool.parse_looks(str(path), names)
    assert looks.dtype == np.int32 and looks.shape == (3, 8)
    # in the order of the names; noise below 0 becomes 0 and the hue is C's % 360, as for the command line's NOISE and HUE
    assert looks.tolist() == [[0, 0, 10, 0, 180, 0, 100, 33], [24, -20, 900, 7, 120, -6, 115, 0], [0, 10, 12, -3, 200, 4, 90, -90]]
    for text in ("a.ppm 1 2 3 4 5 6 7\nb.ppm 0 0 10 0 180 0 100 0\nc.ppm 0 0 10 0 180 0 100 0\n",          # seven integers
                 "a.ppm 0 0 10 0 180 0 100 x\nb.ppm 0 0 10 0 180 0 100 0\nc.ppm 0 0 10 0 180 0 100 0\n",   # not an integer
                 "a.ppm 0 0 10 0 180 0 100 0\nb.ppm 0 0 10 0 180 0 100 0\n",                               # no look for c.ppm
                 "a.ppm 0 0 10 0 180 0 100 0\nb.ppm 0 0 10 0 180 0 100 0\nc.ppm 0 0 10 0 180 0 100 0\nd.ppm 0 0 10 0 180 0 100 0\n",
                 "a.ppm 0 0 10 0 180 0 100 0\na.ppm 0 0 10 0 180 0 100 0\nb.ppm 0 0 10 0 180 0 100 0\nc.ppm 0 0 10 0 180 0 100 0\n"):
        path.write_text(text)
        with pytest.raises(SystemExit):
            tool.parse_looks(str(path), names)
    with pytest.raises(SystemExit):
        tool.main(["stills_dir.py", "--looks", str(path), "64", "48", "0", "0", str(tmp_path), str(tmp_path / "out")])     # without --one-call


@pytest.mark.parametrize("noise,hue", [(0, 0), (12, 5), (24, -123)])
def test_uniform_looks_give_the_uniform_records(crtlib, tool, tmp_path, noise, hue):
    """a looks file that gives every picture the command line's NOISE / HUE and the parameter defaults: the per-still records the
    one call then reads hold exactly what the uniform path's blob holds -- noise, white and ire_base, the three carrier tables"""
    names = ["p%d.ppm" % k for k in range(4)]
    path = tmp_path / "uniform.txt"
    path.write_text("".join("%s %s\n" % (nm, " ".join(str(v) for v in tool.default_look(noise, hue))) for nm in names))
    looks = tool.parse_looks(str(path), names)
    assert (looks == np.array(tool.default_look(noise, hue))).all()
    # the blob of the uniform --one-call path (convert_mixed: CRT defaults, Settings(hue=HUE)) and the one of the --looks path (hue 0)
    kw = dict(w=1, h=1, format=R.FMT_RGB, as_color=1, outw=64, outh=48, out_format=R.FMT_RGB, scanlines=1, blend=1)
    uni = crtlib.make_params("ntsc", noise=noise, hue=hue, **kw)
    lk = crtlib.make_params("ntsc", noise=0, hue=0, **kw)
    recs, levs, hues, env, lenv, henv = crtlib.knobs_prepare8(lk, looks)
    one = crtlib.knobs_prepare8(uni, np.array([tool.default_look(noise, hue)], dtype=np.int32))
    for k in range(len(names)):
        assert recs[k].tolist() == one[0][0].tolist() and recs[k, 0] == noise
        assert (levs[k, 0], levs[k, 1]) == (uni.white, uni.ire_base)
        tables = np.concatenate([np.array(t, dtype=np.int32).reshape(-1) for t in (uni.burst, uni.modI, uni.modQ)])
        np.testing.assert_array_equal(hues[k][:tables.size], tables)
    assert env.noise_max == noise

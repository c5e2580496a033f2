"""Mixed image sizes, host side (no GPU): the structs of include/crt_hip.h, crthip_sizes_prepare against crthip_params_finalize, the
column identity the kernels rely on, the "geometry does not move" premise, every refusal -- and the pin of tests/sizes_cases.py's
oracle loop to the REAL reference (oracle/_ref) on every case, tolerance 0, no case and no field left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import crtref as R
import sizes_cases as SC


@pytest.fixture(scope="module")
def crtlib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(g.PKG, "lib", "libcrthip.so")):
        g.build()
    import crtlib
    assert hasattr(crtlib.load_library(), "crthip_fieldpass_sizes")
    return crtlib


def _flags(crtlib, case):
    c = SC.CASES[case]
    return (crtlib.F_IMAGE_SPARE_ROW if c["spare"] else 0) | (R.EQ_KERNEL.get(c["name"], 0) << 8)


def _params(crtlib, case, **kw):
    c = SC.CASES[case]
    name = c["name"][:4] if c["name"].startswith("ntscfir") else c["name"]
    args = dict(w=1, h=1, format=c["fmt"], as_color=1, outw=SC.OUTW, outh=SC.OUTH, out_format=R.FMT_BGRA, noise=c["noise"],
                flags=_flags(crtlib, case))
    args.update(kw)
    return crtlib.make_params(name, **args)


def test_abi_additions(crtlib, tmp_path):
    """struct sizes on both sides; the additions are purely additive, the ABI version stays where the existing tests pin it"""
    L = crtlib.load_library()
    assert (C.sizeof(crtlib.Size), C.sizeof(crtlib.SizeRec), C.sizeof(crtlib.SizesEnv)) == (16, 32, 32)
    src, exe = str(tmp_path / "sizes_sizeof.c"), str(tmp_path / "sizes_sizeof")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "crt_hip.h"\nint main(void) { printf("%d %d %d %d\\n", (int) sizeof(crthip_size), '
                '(int) sizeof(crthip_size_rec), (int) sizeof(crthip_sizes_env), CRTHIP_ABI_VERSION); return 0; }\n')
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(R.ROOT, "include"), "-o", exe, src], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["16", "32", "32", str(L.crthip_abi_version())]
    for sym in ("crthip_sizes_prepare", "crthip_fieldpass_sizes", "crthip_stills_sizes"):
        assert hasattr(L, sym)


@pytest.mark.parametrize("case", sorted(SC.CASES))
def test_prepare_equals_finalize_per_field(crtlib, case):
    """record k = what crthip_params_finalize derives for a copy of p with field k's w and h; the env = the bounds; the extent = the
    end of the furthest image, which is exactly where the case's buffer ends (no slack)"""
    p = _params(crtlib, case)
    buf, sizes = SC.layout(case)
    recs, env = crtlib.sizes_prepare(p, sizes)
    for k, (w, h, off) in enumerate(sizes):
        q = _params(crtlib, case, w=int(w), h=int(h))
        assert (q.destw, q.desth, q.xo, q.yo) == (p.destw, p.desth, p.xo, p.yo)
        assert tuple(recs[k]) == (w, h, q.col_step_lo, q.col_step_hi, off & 0xffffffff, off >> 32, 0, 0)
    assert (env.n, env.w_min, env.w_max, env.h_min, env.h_max) == (len(sizes), sizes[:, 0].min(), sizes[:, 0].max(),
                                                                   sizes[:, 1].min(), sizes[:, 1].max())
    assert env.extent == buf.size


def test_standard_geometry(crtlib):
    p = _params(crtlib, "scale")
    assert (p.destw, p.desth) == (SC.DESTW, SC.DESTH)


def test_column_identity_for_every_width(crtlib):
    """(x * col_step) >> 32 == x * w / destw for every x < destw and every width of the tables: the scalar column walk of k_active"""
    done = set()
    for case in sorted(SC.CASES):
        p = _params(crtlib, case)
        recs, _ = crtlib.sizes_prepare(p, SC.layout(case)[1])
        x = np.arange(p.destw, dtype=object)
        for r in recs:
            w = int(r[0])
            if (p.destw, w) in done:
                continue
            done.add((p.destw, w))
            step = (int(r[3]) << 32) | int(r[2])
            assert all((xx * step) >> 32 == xx * w // p.destw for xx in x), (case, w)


@pytest.mark.parametrize("case", sorted(SC.CASES))
def test_layout_verdict_does_not_move_with_the_size(crtlib, case):
    L = crtlib.load_library()
    p = _params(crtlib, case)
    n = len(SC.CASES[case]["sizes"])

    def verdict(q, shape):
        lay, fs = (C.c_int * 4)(), C.c_size_t()
        return L.crthip_signal_layout_query(C.byref(q), n, shape, lay, C.byref(fs)), tuple(lay), fs.value
    for w, h in set(SC.CASES[case]["sizes"]):
        q = _params(crtlib, case, w=w, h=h)
        for shape in (0, 1, 2):
            assert verdict(q, shape) == verdict(p, shape)


def test_prepare_refusals(crtlib):
    L = crtlib.load_library()
    p = _params(crtlib, "scale")
    ok = np.array([[8, 8, 0], [4, 2, 256]])

    def refused(params, sizes):
        with pytest.raises(ValueError):
            crtlib.sizes_prepare(params, np.asarray(sizes))
    crtlib.sizes_prepare(p, ok)
    refused(p, [[0, 8, 0]])
    refused(p, [[8, 0, 0]])
    refused(p, [[8, -3, 0]])
    refused(p, [[8, 8, 2]])                                        # 4-byte pixels at an offset that is no multiple of 4
    crtlib.sizes_prepare(_params(crtlib, "rgb_odd"), np.array([[8, 8, 3]]))
    refused(_params(crtlib, "scale", raw=1), ok)
    refused(_params(crtlib, "scale", format=17), ok)               # crt_modulate refuses the format: no image would be read
    refused(crtlib.make_params("nes", w=256, h=240, outw=SC.OUTW, outh=SC.OUTH), [[256, 240, 0]])
    unfinal = crtlib.Params()
    C.memmove(C.byref(unfinal), C.byref(p), C.sizeof(p))
    unfinal.finalized = 0
    refused(unfinal, ok)
    sin, rec, env = (crtlib.Size * 1)(), (crtlib.SizeRec * 1)(), crtlib.SizesEnv()
    sin[0].w = sin[0].h = 8
    assert L.crthip_sizes_prepare(C.byref(p), 1, sin, rec, C.byref(env)) == 0
    assert L.crthip_sizes_prepare(C.byref(p), 0, sin, rec, C.byref(env)) < 0
    assert L.crthip_sizes_prepare(None, 1, sin, rec, C.byref(env)) < 0
    assert L.crthip_sizes_prepare(C.byref(p), 1, None, rec, C.byref(env)) < 0
    assert L.crthip_sizes_prepare(C.byref(p), 1, sin, None, C.byref(env)) < 0
    assert L.crthip_sizes_prepare(C.byref(p), 1, sin, rec, None) < 0


GUARD_PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "crt_size_guard.h"
typedef unsigned long long u64;
static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 10) std::printf("line %d: %s\n", __LINE__, #c); } } while (0)
int main()
{
    const int vals[] = { -2147483647 - 1, -5, -1, 0, 1, 3, 4, 5, 16, 753, 1 << 20, (1 << 29) - 1, 1 << 29, 2147483647 };
    const u64 offs[] = { 0, 1, 2, 4, 60, 64, 4096, 1ull << 31, 1ull << 32, (1ull << 63) + 4, ~0ull - 3, ~0ull };
    const u64 extents[] = { 32, 64, 4096, 1ull << 20, 1ull << 33, ~0ull };
    const u64 steps[] = { 0, 1, 0x55555555ull, 1ull << 32, (1ull << 32) * 3 / 753, 2800000ull << 32, 0x7fffffffull << 32,
                          0x80000000ull << 32, 0xdeadbeefcafef00dull, ~0ull };
    const int nv = sizeof(vals) / sizeof(*vals), no = sizeof(offs) / sizeof(*offs), ne = sizeof(extents) / sizeof(*extents);
    long n_ok = 0, n_fallback = 0;
    for (int bpp = 3; bpp <= 4; bpp++) for (int spare = 0; spare < 2; spare++) for (int tiles = 0; tiles <= (bpp == 4); tiles++)
    for (int e = 0; e < ne; e++) for (int a = 0; a < nv; a++) for (int b = 0; b < nv; b++) for (int o = 0; o < no; o++)
    for (unsigned s = 0; s < sizeof(steps) / sizeof(*steps); s++) {
        crthip_size_rec r = { vals[a], vals[b], (unsigned) steps[s], (unsigned) (steps[s] >> 32), (unsigned) offs[o], (unsigned) (offs[o] >> 32), { 0, 0 } };
        const size_view v = size_rec_checked(r, bpp, spare != 0, tiles != 0, extents[e]);
        /* what the kernel may rely on: a walkable size, and the image (with its spare row) inside the extent -- in 128-bit arithmetic */
        CHECK(v.w >= (tiles ? 4 : 1) && v.h >= 1);
        CHECK(!tiles || ((v.off & 3) == 0 && v.w < (1 << 29)));
        const unsigned __int128 end = (unsigned __int128) v.off + (unsigned __int128) ((u64) v.h + spare) * (u64) v.w * bpp;
        CHECK(end <= extents[e]);
        const bool kept = v.w == r.w && v.h == r.h && v.off == offs[o];
        if (kept) { n_ok++; CHECK(v.cstep == steps[s]); } else { n_fallback++; CHECK(v.w == (tiles ? 4 : 1) && v.h == 1 && v.off == 0); }
        /* the column walk of the sample loop (the tile path also computes the three samples behind the line end) */
        u64 cpos = 0;
        for (int x = 0; x < 753 + 3; x++) {
            const int col = size_col_clamped((int) (cpos >> 32), v.w);
            CHECK(col >= 0 && col < v.w);
            cpos += v.cstep;
        }
    }
    /* a record of crthip_sizes_prepare passes through unchanged, and its columns are not touched */
    for (int w = 1; w < 2000; w += 7) {
        const u64 step = (((u64) w << 32) + 752) / 753;
        crthip_size_rec r = { w, 9, (unsigned) step, (unsigned) (step >> 32), 64, 0, { 0, 0 } };
        const size_view v = size_rec_checked(r, 4, true, w >= 4, 64 + (u64) w * 10 * 4);
        CHECK(v.w == w && v.h == 9 && v.off == 64 && v.cstep == step);
        for (int x = 0; x < 753; x++) CHECK(size_col_clamped((int) ((x * step) >> 32), w) == x * w / 753);
        const size_view t = size_rec_checked(r, 4, true, w >= 4, 64 + (u64) w * 10 * 4 - 1);      /* one byte short: refused */
        CHECK(t.off == 0 && t.h == 1);
    }
    std::printf("%ld %ld %d\n", n_ok, n_fallback, bad);
    return bad != 0;
}
"""


def test_address_guard_on_hostile_records(crtlib, tmp_path):
    """csrc/crt_size_guard.h -- the very functions k_active's SZ instantiations call -- compiled for the host and run over hostile
    records: sizes, offsets and extents at every edge (negative, zero, 2^29, 2^31 - 1, offsets near 2^64) and col_step values that
    make the column negative at once (col_step_hi >= 0x80000000) or after accumulation.  Whatever the record, the view the kernel
    walks lies inside the extent and every column inside [0, w); records of crthip_sizes_prepare pass unchanged.  A guard that failed
    on the device would be a fault there; this is where it is shown instead."""
    src, exe = str(tmp_path / "guard_probe.cpp"), str(tmp_path / "guard_probe")
    with open(src, "w") as f:
        f.write(GUARD_PROBE)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(R.ROOT, "include"),
                    "-I" + os.path.join(R.ROOT, "ntsc-crt_amd", "csrc"), "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    n_ok, n_fallback, bad = (int(t) for t in r.stdout.split()[-3:])
    assert r.returncode == 0 and bad == 0, r.stdout
    assert n_ok > 1000 and n_fallback > 1000, "both outcomes are exercised"


def test_layouts_are_what_they_claim(crtlib):
    """packed with no slack, descending order, a shared image, 3-byte formats at odd offsets, 4-byte ones at offsets = 4 mod 8"""
    for case, c in SC.CASES.items():
        buf, sizes = SC.layout(case)
        b, spare = SC.bpp(case), 1 if c["spare"] else 0
        ends = sizes[:, 2] + (sizes[:, 1] + spare) * sizes[:, 0] * b
        assert ends.max() == buf.size
        for k, (w, h, off) in enumerate(sizes):
            np.testing.assert_array_equal(buf[off:off + (h + spare) * w * b], SC.field_image(case, k)[:h + spare].reshape(-1))
        if c["pack"] == "packed":
            assert sizes[0, 2] == 0 and (np.sort(sizes[:, 2])[1:] == np.sort(ends)[:-1]).all()
        if c["pack"] == "descending":
            assert (np.diff(sizes[:, 2]) < 0).all()
        if c["pack"] == "shared":
            assert sizes[-1, 2] == sizes[0, 2]
        if c["pack"] == "odd":
            assert b == 3 and (sizes[:, 2] % 2 == 1).any()
        if c["pack"] == "mod8":
            assert b == 4 and (sizes[:, 2] % 8 == 4).any() and (sizes[:, 2] % 4 == 0).all()


@pytest.mark.skipif(not R.have_ref("ntsc"), reason="oracle/_ref not built (no reference sources on this machine)")
@pytest.mark.parametrize("case", sorted(SC.CASES))
def test_oracle_loop_equals_the_reference(crtlib, case):
    """the loop the GPU tests compare with IS the reference's: every case, every field, every pass, tolerance 0; the inputs are chosen
    so that no field falls into the reference's undefined over-read (crtref.reads_past_inp) -- the cap on left-out fields is 0"""
    name = SC.CASES[case]["name"]
    assert R.have_ref(name), "no reference build of " + name
    sched = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)] if case.startswith("stills") else None
    got = SC.checker_fields(R.Oracle(name), case, schedule=sched)
    want = SC.checker_fields(R.RefLib(name), case, schedule=sched)
    for k, (g, w) in enumerate(zip(got, want)):
        for step, (a, b) in enumerate(zip(g, w)):
            tag = "%s field %d pass %d" % (case, k, step)
            assert not a["undefined"], tag + ": inside the reference's undefined over-read -- choose other inputs, exclude nothing"
            for key in ("inp", "out", "ccf"):
                np.testing.assert_array_equal(a[key], b[key], err_msg=tag + " " + key)
            assert (a["hsync"], a["vsync"], a["rn"]) == (b["hsync"], b["vsync"], b["rn"]), tag

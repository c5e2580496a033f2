"""CPU checks of the phosphor display modes (CRTHIP_F_PHOSPHOR_FADE / _CLEAR, include/crt_hip.h): the numpy restatement of
crt_main.c's fade_phosphors / memset (crt_main.c:438-463) that the GPU tests take their expected pictures from, pinned against the
reference's word formula; the host table crthip_phosphor_table; the flags' validation in crthip_params_finalize."""
import ctypes as C

import numpy as np
import pytest

import crtref as R

# the byte of a pixel the decoder writes 0xff into (crt_core.c:620-652); RGB / BGR have none
ALPHA_BYTE = {R.FMT_RGBA: 3, R.FMT_BGRA: 3, R.FMT_ARGB: 0, R.FMT_ABGR: 0, R.FMT_RGB: None, R.FMT_BGR: None}
DEPTH = 38


def fade_bytes(a):
    """fade of every byte: (c>>1) + (c>>2) + (c>>3) + (c>>4)"""
    a = np.asarray(a, dtype=np.uint8)
    return ((a >> 1) + (a >> 2) + (a >> 3) + (a >> 4)).astype(np.uint8)


def fade_np(buf, fmt, times=1):
    """one (or `times`) phosphor fade of an output buffer of format `fmt` (any shape whose bytes are whole pixels): every colour
    byte faded, the alpha byte of the 4-byte formats 0"""
    out = np.array(buf, dtype=np.uint8, copy=True)
    flat = out.reshape(-1)
    for _ in range(times):
        flat[:] = fade_bytes(flat)
    ab = ALPHA_BYTE[fmt]
    if ab is not None:
        flat.reshape(-1, 4)[:, ab] = 0
    return out


def clear_np(buf):
    """crt_main.c:462: every byte 0"""
    return np.zeros_like(np.asarray(buf, dtype=np.uint8))


def display_step_np(buf, fmt, mode):
    return fade_np(buf, fmt) if mode == "fade" else clear_np(buf)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def test_restatement_is_the_word_formula_of_crt_main():
    """crt_main.c:446-450 on the little-endian int of a BGRA (or RGBA) pixel, 200 000 random words"""
    words = R.lcg_bytes(4 * 200000, 77).view("<u4")
    c = words & np.uint32(0xffffff)
    want = (((c >> 1) & np.uint32(0x7f7f7f)) + ((c >> 2) & np.uint32(0x3f3f3f)) +
            ((c >> 3) & np.uint32(0x1f1f1f)) + ((c >> 4) & np.uint32(0x0f0f0f))).astype("<u4")
    for fmt in (R.FMT_BGRA, R.FMT_RGBA):
        got = fade_np(words.view(np.uint8), fmt).view("<u4")
        np.testing.assert_array_equal(got, want)


def test_fade_depth_is_38():
    """fade is monotone, fade(c) < c for c > 0, fade^38 = 0 for every byte and fade^37(255) != 0: CLEAR = fade 38 or more times"""
    c = np.arange(256, dtype=np.uint8)
    f = fade_bytes(c)
    assert np.all(np.diff(f.astype(int)) >= 0)
    assert np.all(f[1:] < c[1:]) and f[0] == 0
    v = c.copy()
    for _ in range(DEPTH - 1):
        v = fade_bytes(v)
    assert v[255] != 0
    assert np.all(fade_bytes(v) == 0)
    assert list(fade_bytes(np.array([255, 236, 220], dtype=np.uint8))) == [236, 220, 205]


def test_phosphor_table_is_fade_to_the_power_of_age(lib):
    c = np.arange(256, dtype=np.uint8)
    v = c.copy()
    for age in range(65):
        got = np.frombuffer(lib.phosphor_table(age), dtype=np.uint8)
        np.testing.assert_array_equal(got, v, err_msg="age %d" % age)
        if age >= DEPTH:
            assert not got.any()
        v = fade_bytes(v)
    L = lib.load_library()
    lut = (C.c_ubyte * 256)()
    assert L.crthip_phosphor_table(-1, lut) == -1                     # CRTHIP_E_ARG


def test_finalize_refuses_fade_and_clear_together(lib):
    for flags in (lib.F_PHOSPHOR_FADE, lib.F_PHOSPHOR_CLEAR):
        p = lib.make_params("ntsc", w=640, h=480, outw=640, outh=480, flags=flags)
        assert p.flags & (lib.F_PHOSPHOR_FADE | lib.F_PHOSPHOR_CLEAR) == flags
    with pytest.raises(ValueError):
        lib.make_params("ntsc", w=640, h=480, outw=640, outh=480, flags=lib.F_PHOSPHOR_FADE | lib.F_PHOSPHOR_CLEAR)
    # and through the C call itself
    L = lib.load_library()
    p = lib.Params()
    assert L.crthip_params_default(C.byref(p), 0, 1) == 0
    p.w, p.h, p.outw, p.outh = 320, 240, 320, 240
    p.flags = lib.F_PHOSPHOR_FADE | lib.F_PHOSPHOR_CLEAR
    assert L.crthip_params_finalize(C.byref(p)) == -1
    p.flags = lib.F_PHOSPHOR_CLEAR
    assert L.crthip_params_finalize(C.byref(p)) == 0


def test_make_params_round_trips_the_flags(lib):
    assert (lib.F_PHOSPHOR_FADE, lib.F_PHOSPHOR_CLEAR) == (0x8000, 0x10000)
    for name in ("ntsc", "nes", "ntscbloom", "vhs"):
        for f in (lib.F_PHOSPHOR_FADE, lib.F_PHOSPHOR_CLEAR):
            p = lib.make_params(name, w=256, h=240, outw=640, outh=480, flags=f)
            assert p.flags & f == f
            assert p.flags & (lib.F_PHOSPHOR_FADE | lib.F_PHOSPHOR_CLEAR) == f
    assert lib.PHOSPHOR_FLAGS == {"keep": 0, "fade": lib.F_PHOSPHOR_FADE, "clear": lib.F_PHOSPHOR_CLEAR}

"""CPU checks of the per-field knobs (crthip_knobs_prepare / crthip_fieldpass_knobs, include/crt_hip.h; the GPU side is
tests/test_gpu_knobs.py): the host-side records and bounds against crthip_params_finalize field by field, the refusals, the ABI
additions, and the knob triples of tests/knobs_cases.py through the oracle against the compiled reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import crtref as R
import knobs_cases as KC


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    R.build_oracle()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


# hues of both signs and beyond +-360, saturation 0 and negative, noise 0 inside a noisy batch
TRIPLES = [(24, 0, 10), (0, 17, 14), (110, -33, 0), (5, 725, -70), (60, -1000, 900), (12, 360, 13), (0, -360, 1), (200, 359, 40)]


def _base(lib, system="ntsc", **kw):
    d = dict(w=64, h=48, outw=160, outh=120)
    d.update(kw)
    return lib.make_params(system, **d)


@pytest.mark.parametrize("system", ["ntsc", "ntscbloom", "vhs", "vhslcg", "nes", "snes", "temp", "nesrgb", "pv1k"])
def test_prepare_field_by_field_against_finalize(lib, system):
    p = _base(lib, system, noise=77, mon_hue=5, saturation=3)       # its own three knobs are ignored
    recs, env = lib.knobs_prepare(p, np.array(TRIPLES, dtype=np.int64))
    assert recs.shape == (len(TRIPLES), 8) and recs.dtype == np.int32
    bounds = []
    for k, (noise, hue, sat) in enumerate(TRIPLES):
        q = _base(lib, system, noise=noise, mon_hue=hue, saturation=sat)
        r = recs[k].view(np.int32)
        assert (r[0], r[1], r[2], r[3], r[4]) == (noise, q.huesn, q.huecs, sat, q.bloom_max_e), (system, k)
        assert not r[5:].any()
        # the library's own envelope for a uniform batch with this field's noise (crt_host.hip, sync_blob)
        lo, hi = C.c_int(), C.c_int()
        L = lib.load_library()
        L.crt_setup_signal_range(C.byref(q), C.byref(lo), C.byref(hi))
        bounds.append(L.crt_setup_loskip_bound(lo.value, hi.value))
    assert env.magic == 0x43524B31 and env.n == len(TRIPLES)
    assert env.noise_max == max(abs(t[0]) for t in TRIPLES) == 200
    assert env.sat_abs_max == max(abs(t[2]) for t in TRIPLES) == 900
    assert env.loskip_wave_max == min(bounds)                        # valid for every field: the narrowest of the per-field bounds
    assert 65532 <= env.loskip_wave_max <= 120000
    assert not any(env.reserved)


def test_prepare_envelope_with_noise_of_both_signs(lib):
    """the signal range grows with |noise| on either side of zero: the bound is the smaller of the two extremes'"""
    L = lib.load_library()
    trip = [(-90, 0, 10), (3, 0, 10), (60, 0, 10)]
    _, env = lib.knobs_prepare(_base(lib), np.array(trip))
    per = []
    for noise, _, _ in trip:
        q = _base(lib, noise=noise)
        lo, hi = C.c_int(), C.c_int()
        L.crt_setup_signal_range(C.byref(q), C.byref(lo), C.byref(hi))
        per.append(L.crt_setup_loskip_bound(lo.value, hi.value))
    assert env.loskip_wave_max == min(per) and env.noise_max == 90
    _, env0 = lib.knobs_prepare(_base(lib), np.array([(0, 5, 10)] * 3))
    assert env0.noise_max == 0 and env0.sat_abs_max == 10


def test_prepare_accepts_tensors_and_checks_the_shape(lib):
    import torch
    p = _base(lib)
    a, ea = lib.knobs_prepare(p, np.array(TRIPLES, dtype=np.int32))
    b, eb = lib.knobs_prepare(p, torch.tensor(TRIPLES, dtype=torch.int64))
    assert np.array_equal(a, b) and bytes(ea) == bytes(eb)
    for bad in (np.zeros((4, 2), dtype=np.int32), np.zeros((0, 3), dtype=np.int32), np.zeros((3,), dtype=np.int32), np.zeros((2, 3), dtype=np.float32)):
        with pytest.raises(ValueError):
            lib.knobs_prepare(p, bad)


def test_prepare_refusals(lib):
    L = lib.load_library()
    p = _base(lib)
    kin = (lib.Knobs * 2)(lib.Knobs(24, 0, 10, 0), lib.Knobs(0, 5, 10, 0))
    recs, env = (lib.KnobRec * 2)(), lib.KnobsEnv()
    assert L.crthip_knobs_prepare(C.byref(p), 2, kin, recs, C.byref(env)) == 0
    assert L.crthip_knobs_prepare(C.byref(p), 0, kin, recs, C.byref(env)) == -1
    assert L.crthip_knobs_prepare(C.byref(p), -3, kin, recs, C.byref(env)) == -1
    assert L.crthip_knobs_prepare(None, 2, kin, recs, C.byref(env)) == -1
    assert L.crthip_knobs_prepare(C.byref(p), 2, None, recs, C.byref(env)) == -1
    assert L.crthip_knobs_prepare(C.byref(p), 2, kin, None, C.byref(env)) == -1
    assert L.crthip_knobs_prepare(C.byref(p), 2, kin, recs, None) == -1
    raw = lib.Params()
    L.crthip_params_default(C.byref(raw), 0, 1)
    raw.w = raw.h = raw.outw = raw.outh = 64                          # never finalized
    assert L.crthip_knobs_prepare(C.byref(raw), 2, kin, recs, C.byref(env)) == -1
    # what crthip_params_finalize refuses with the field's knobs in place: bloom builds with noise < 0 or max_e <= 0
    pb = _base(lib, "ntscbloom")
    for noise in (-1, -300, -256):
        with pytest.raises(ValueError):
            _base(lib, "ntscbloom", noise=noise)
        bad = (lib.Knobs * 2)(lib.Knobs(24, 0, 10, 0), lib.Knobs(noise, 0, 10, 0))
        assert L.crthip_knobs_prepare(C.byref(pb), 2, bad, recs, C.byref(env)) == -1
        assert L.crthip_knobs_prepare(C.byref(p), 2, bad, recs, C.byref(env)) == 0      # no bloom: negative noise is legal
    with pytest.raises(ValueError):
        lib.knobs_prepare(pb, np.array([(24, 0, 10), (-1, 0, 10)]))


def test_abi_additions(lib, tmp_path):
    """struct sizes on both sides, the symbols are exported, and the library reports the header's ABI version.  The additions are
    purely additive (new symbols, nothing existing changes meaning), and the existing ABI tests pin crthip_abi_version() to 6, so the
    version stays where they hold it: a host finds out about the knob entry points by their presence."""
    assert (C.sizeof(lib.Knobs), C.sizeof(lib.KnobRec), C.sizeof(lib.KnobsEnv)) == (16, 32, 32)
    L = lib.load_library()
    for sym in ("crthip_knobs_prepare", "crthip_fieldpass_knobs"):
        assert hasattr(L, sym), sym
    src, exe = str(tmp_path / "knobs_sizeof.c"), str(tmp_path / "knobs_sizeof")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "crt_hip.h"\nint main(void) { printf("%d %d %d %d\\n", (int) sizeof(crthip_knobs), '
                '(int) sizeof(crthip_knob_rec), (int) sizeof(crthip_knobs_env), CRTHIP_ABI_VERSION); return 0; }\n')
    subprocess.run(["gcc", "-std=c89", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(R.ROOT, "include"), "-o", exe, src], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["16", "32", "32", str(L.crthip_abi_version())]


def test_python_wrappers_exist(lib):
    assert callable(lib.knobs_prepare) and callable(lib.CRT.fieldpass_knobs) and callable(lib.CRT.upload_knobs)


def _tier_of(wave_abs):
    return 0 if wave_abs <= 65532 else 1 if wave_abs <= 120000 else 2 if wave_abs <= 524288 else 3


def test_tier_mixing_triples_mix_tiers_and_stay_out_of_the_reference_ub():
    """The six triples of the small GPU case: run through the oracle field by field (the expected values of the GPU test), none may
    fall under the exclusion rule of the parity tests (crtref.reads_past_inp), and their carrier amplitudes must put the lines of
    one wavefront into different decoder tiers (|wave| against 65 532 / 120 000 / 2^19, crt_dev.h)."""
    tiers = set()
    for k, res in enumerate(KC.oracle_fields("ntsc", KC.SMALL, KC.SMALL_TRIPLES, steps=2)):
        for step in res:
            assert not step["undefined"], "triple %d falls under the reference-UB exclusion: choose another" % k
            tr = step["trace"]
            valid = tr[:, 0] == 1
            tiers.add(_tier_of(int(np.abs(tr[valid][:, 2:4]).max())))
    assert tiers >= {0, 1, 3} or tiers >= {0, 2, 3}, tiers


@pytest.mark.skipif(not R.have_ref("ntsc"), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", ["ntsc", "vhslcg"])
def test_knob_triples_oracle_against_the_compiled_reference(name):
    """the expected values of the GPU cases are the oracle's: pinned here against the reference itself, per triple"""
    geo = KC.SMALL
    for k, (noise, hue, sat) in enumerate(KC.SMALL_TRIPLES):
        ref, orc = R.RefLib(name), R.Oracle(name)
        pair = [(ref, ref.new_crt(geo["outw"], geo["outh"], R.FMT_BGRA)), (orc, orc.new_crt(geo["outw"], geo["outh"], R.FMT_BGRA))]
        img = KC.image(geo, k)
        pad = np.concatenate([img, img[-1:]], axis=0)
        for _, c in pair:
            c.settings(pad, format=R.FMT_BGRA, w=geo["w"], h=geo["h"], as_color=1, field=k & 1, frame=(k >> 1) & 1)
            c.set("hue", hue)
            c.set("saturation", sat)
            c.set("scanlines", 1)
        for step in range(2):
            for _, c in pair:
                c.modulate()
                c.demodulate(noise)
            R.compare_state(pair[0][1], pair[1][1], "%s triple %d step %d" % (name, k, step))

"""The float form of the decoder's filter stages without a GPU, through the host function crthip_float_stages_query:
the rounding identity behind it, the constants it hands the kernel, the bias schedule reproduced by an exact-integer model of a
cascade against the reference's recurrence, and the verdicts that must be "no"."""
import random
import struct
import zlib

import numpy as np
import pytest

# every system and build switch the library can set coefficients for (crtlib.SYSTEMS, crtlib.VARIANTS, the bloom builds)
NAMES = ["ntsc", "ntscp0", "nes", "nesp0", "snes", "pv1k", "temp", "nesrgb", "vhs", "vhslp", "vhsep", "vhslcg", "ntschipass",
         "nesborder", "ntscbloom", "vhsbloom", "snesbloom", "pv1kbloom"]
B23, B24, BITS0 = 1 << 23, 1 << 24, 0x4B000000
CASCADES = ("luma low", "luma high", "I high", "Q high")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def _params(lib, name, **kw):
    return lib.make_params(name, w=64, h=48, outw=64, outh=48, **kw)


def _value(bits):
    """the integer a float bit pattern of the binade [2^23, 2^24) holds"""
    assert BITS0 <= bits < BITS0 + B23, hex(bits)
    return bits - BITS0 + B23


def _fma_down(d, ce, addend):
    """v_fma_f32 in round-toward-minus-infinity on exact integers: floor(d * ce / 65536 + addend), which must land in the binade
    (ulp 1 there: the rounding is the floor and nothing else)"""
    r = (d * ce) // 65536 + addend          # Python's // floors; addend is an integer
    assert B23 <= r < B24, r
    return r


def _coefficients(p):
    return [p.eq_lf[0], p.eq_hf[0], p.eq_hf[1], p.eq_hf[2]]


@pytest.mark.parametrize("name", NAMES)
def test_rounding_identity_and_constants(lib, name):
    p = _params(lib, name)
    ok, f = lib.float_stages(p)
    # the verdict: the arithmetic holds for every system; the decoder runs it for the systems of 4 samples per chroma cycle
    assert f.ranges_ok == 1 and ok == f.ok == (0 if name.startswith("pv1k") else 1), name
    for k, c in enumerate(_coefficients(p)):
        q = f.cas[k]
        assert q.c == c and q.form == (1 if k < 2 else 0)
        ce = c - 65536 if q.form else c
        assert q.ce == ce and ce != 0
        # c * a / 65536 = n + 1/2, exactly; a is a power of two with the sign of ce
        assert 2 * ce * q.a == 65536 * (2 * q.n + 1), (name, k)
        assert abs(q.a) & (abs(q.a) - 1) == 0 and (q.a > 0) == (ce > 0) and q.n >= 0
        # the identity, for every difference the envelope can produce and beyond
        d = np.arange(-(1 << 17), (1 << 17) + 1, dtype=np.int64)
        assert np.array_equal((ce * d + 32768) >> 16, np.floor_divide(ce * (d + q.a), 65536) - q.n), (name, k)
        # the multiplier is ce / 65536 as a float, exactly
        assert struct.unpack("<f", struct.pack("<i", q.mul_bits))[0] * 65536.0 == float(ce)
        assert q.drift == (q.n + q.a if q.form else q.n) and q.dstage == (q.n if q.form else q.n - q.a)
        assert _value(q.in0_bits) - _value(q.x0_bits) == q.a
        assert _value(q.out0_bits) == _value(q.x0_bits) + 3 * q.dstage + q.drift


def _run_cascade(q, steps, inputs):
    """The kernel's schedule (eq_stepf_yiq) on exact integers: four stages, the input biased by in0 + t * drift, stage 3 un-biased by
    out0 + t * drift.  Returns the un-biased outputs and the range every biased value took."""
    x = [_value(q.x0_bits) + j * q.dstage for j in range(4)]
    kin, kout = _value(q.in0_bits), _value(q.out0_bits)
    lo, hi, out = min(x), max(x), []
    for t in range(steps):
        u = inputs[t] + kin
        assert B23 <= u < B24
        lo, hi = min(lo, u), max(hi, u)
        prev = u
        for j in range(4):
            d = prev - x[j]                                   # v_sub_f32: exact
            x[j] = _fma_down(d, q.ce, prev if q.form else x[j])
            lo, hi = min(lo, x[j]), max(hi, x[j])
            prev = x[j]
        out.append(x[3] - kout)
        kin += q.drift
        kout += q.drift
    return out, lo, hi


def _reference(c, inputs):
    """crt_core.c:206-233, one cascade"""
    x, out = [0, 0, 0, 0], []
    for u in inputs:
        prev = u
        for j in range(4):
            x[j] += (c * (prev - x[j]) + 32768) >> 16
            prev = x[j]
        out.append(x[3])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_bias_schedule_stays_in_the_binade_and_equals_the_recurrence(lib, name):
    p = _params(lib, name)
    ok, f = lib.float_stages(p)
    assert f.ranges_ok == 1
    rng = random.Random(zlib.crc32(name.encode()))
    for k, c in enumerate(_coefficients(p)):
        q = f.cas[k]
        assert B23 <= q.lo and q.hi < B24, (name, CASCADES[k])
        m = q.in_max
        # one line per cascade: random samples at the envelope's amplitude, with runs at either extreme
        inputs = []
        while len(inputs) < f.steps:
            mode = rng.randrange(4)
            run = rng.randrange(1, 40)
            inputs += [m if mode == 0 else -m if mode == 1 else rng.randint(-m, m) for _ in range(run)]
        inputs = inputs[:f.steps]
        got, lo, hi = _run_cascade(q, f.steps, inputs)
        assert got == _reference(c, inputs), (name, CASCADES[k])
        assert q.lo <= lo and hi <= q.hi, (name, CASCADES[k], lo, hi, q.lo, q.hi)
        assert max(abs(v) for v in got) <= q.state_max


def test_brightness_is_part_of_the_luma_envelope(lib):
    for b in (-2600, -300, 0, 300, 2600):
        p = _params(lib, "ntsc", brightness=b)
        ok, f = lib.float_stages(p)
        assert ok == 1
        assert f.cas[0].in_max == 128 + abs(p.bright) and f.cas[1].in_max == 128 + abs(p.bright)
        q = f.cas[1]
        m = q.in_max
        inputs = [m if (t // 37) % 2 else -m for t in range(f.steps)]
        got, lo, hi = _run_cascade(q, f.steps, inputs)
        assert got == _reference(q.c, inputs) and q.lo <= lo and hi <= q.hi


def test_verdict_no(lib):
    import ctypes as C
    L = lib.load_library()
    base = _params(lib, "ntsc")
    assert lib.float_stages(base)[0] == 1

    def verdict(steps=0, **coef):
        p = lib.Params()
        C.memmove(C.byref(p), C.byref(base), C.sizeof(p))
        for k, v in coef.items():
            name, i = k.rsplit("_", 1)
            getattr(p, name)[int(i)] = v
        out = lib.FStages()
        return L.crthip_float_stages_query(C.byref(p), steps, C.byref(out)), out

    # made-up coefficients: an odd one (a = 2^15, n up to 2^14: the biases run out of the binade within a line), alpha = 1
    # exactly (no odd part), a chroma coefficient at 2^15 and a luma one below it (outside the forms' ranges)
    assert verdict(eq_hf_1=32637)[0] == 0
    assert verdict(eq_lf_0=42157)[0] == 0
    assert verdict(eq_hf_0=65536)[0] == 0
    assert verdict(eq_hf_2=32768)[0] == 0
    assert verdict(eq_lf_0=32000)[0] == 0
    # an over-long line: the drift (5270 per sample for NTSC's luma low cascade) leaves the binade
    rc, out = verdict(steps=1700)
    assert rc == 0 and out.steps == 1700
    assert verdict(steps=1000)[0] == 1
    # arguments
    assert L.crthip_float_stages_query(None, 0, C.byref(lib.FStages())) < 0
    raw = lib.Params()
    assert L.crthip_float_stages_query(C.byref(raw), 0, C.byref(lib.FStages())) < 0       # not finalized

"""The oracle is the real reference on the inputs tests/test_gpu_parity.py runs: every (table, system-name variant, case) of
tests/parity_cases.py through oracle/crt_oracle.c and through the reference compiled unmodified (oracle/_ref), with the inputs, knobs,
noise, passes and field walk of the GPU test, compared after every call at tolerance 0 -- analog and ccf after crt_modulate, inp, ccf,
hsync, vsync, rn and out after crt_demodulate.  A reading error that the oracle shares with a kernel passes every GPU test; it does not
pass here.  Fields that crtref.reads_past_inp takes out (the reference reads behind inp[] + 16 there: undefined)
are counted, and the count is a stated condition: parity_cases.EXCLUDED, asserted exactly.  CPU only."""
import numpy as np
import pytest

import crtref as R
import parity_cases as P

pytestmark = pytest.mark.skipif(not R.have_ref("ntsc"), reason="oracle/_ref not built (no reference sources on this machine)")

_LIBS = {}


def _checkers(name):
    if not R.have_ref(name):
        pytest.skip("no reference build of " + name)
    if name not in _LIBS:
        _LIBS[name] = (R.Oracle(name), R.RefLib(name))
    return _LIBS[name]


def _same(a, b, what):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=what)


def _modulated(o, r, what):
    _same(o.analog, r.analog, what + " analog")
    _same(o.ccf, r.ccf, what + " ccf after modulate")


def _demodulate(orc, o, r, noise, what):
    """crt_demodulate on both; inp and rn compared (they do not depend on what the sync search reads) -> does the reference read past
    inp[] + 16 in this pass?"""
    hs_before = o.get("hsync")
    o.demodulate(noise, trace=True)
    r.demodulate(noise)
    _same(o.inp, r.inp, what + " inp")
    assert o.get("rn") == r.get("rn"), what + " rn"
    return R.reads_past_inp(orc, o.trace, o.get("vsync"), hs_before)


def _demodulated(o, r, what):
    _same(o.ccf, r.ccf, what + " ccf")
    for f in ("hsync", "vsync"):
        assert o.get(f) == r.get(f), "%s %s: oracle %d reference %d" % (what, f, o.get(f), r.get(f))
    _same(o.out, r.out, what + " out")


def _stated(table, cid, lost, passes):
    assert lost == P.excluded(table, cid), "%s %s: reads_past_inp excludes %d of %d field-passes, parity_cases.EXCLUDED says %d" % (
        table, cid, lost, passes, P.excluded(table, cid))
    assert 2 * lost <= passes, "%s %s: more than half of the field-passes are out of the comparison" % (table, cid)


def _ids(kind):
    return [(t, cid) for t, tab in P.TABLES.items() if tab["kind"] == kind for cid in tab["cases"]]


def _name(p):
    return "%s-%s" % p


@pytest.mark.parametrize("tc", _ids("run"), ids=_name)
def test_oracle_equals_the_reference_on_the_run_case_tables(tc):
    table, cid = tc
    tab = P.TABLES[table]
    case, ks = tab["cases"][cid], range(tab["n"])
    if table == "SHAPE_PICK":
        case, k0, k1 = case
        ks = range(k0, k1)
    orc, ref = _checkers(case[0])
    noise, lost = case[7], 0
    for k in ks:
        img = P.image(case, k)
        o, r = P.checker_crt(orc, case, k, img), P.checker_crt(ref, case, k, img)
        for step in range(tab["steps"]):
            what = "%s %s field %d pass %d" % (table, cid, k, step)
            P.checker_walk(orc, o, k, step)
            P.checker_walk(ref, r, k, step)
            o.modulate()
            r.modulate()
            _modulated(o, r, what)
            if _demodulate(orc, o, r, noise, what):
                lost += tab["steps"] - step              # out of the comparison from here on, as in _run_case
                break
            _demodulated(o, r, what)
    _stated(table, cid, lost, len(ks) * tab["steps"])


@pytest.mark.parametrize("tc", _ids("nes"), ids=_name)
def test_oracle_equals_the_reference_on_the_nes_table(tc):
    table, cid = tc
    tab = P.TABLES[table]
    case, fused = tab["cases"][cid]
    orc, ref = _checkers(case[0])
    lost = 0
    for k in range(tab["n"]):
        o, r = P.nes_checker_crt(orc, case), P.nes_checker_crt(ref, case)
        for step in range(tab["steps"]):
            what = "%s %s field %d pass %d" % (table, cid, k, step)
            P.nes_checker_pass(o, step, k, fused)
            P.nes_checker_pass(r, step, k, fused)
            _modulated(o, r, what)
            if _demodulate(orc, o, r, case[3], what):
                lost += tab["steps"] - step
                break
            _demodulated(o, r, what)
    _stated(table, cid, lost, tab["n"] * tab["steps"])


@pytest.mark.parametrize("tc", _ids("vhs"), ids=_name)
def test_oracle_equals_the_reference_on_the_rand_noise_vhs_builds(tc):
    """one checker runs a field's whole sequence under srand(seed), then the other under the same seed: they share libc's stream"""
    table, cid = tc
    sysname, fused, noise, size = P.TABLES[table]["cases"][cid]
    orc, ref = _checkers(sysname)
    imgs = P.vhs_images(size)
    names = ("inp", "out", "hsync", "vsync", "rn", "ccf", "analog", "ccf after modulate")
    for k in range(P.VHS_N):
        a = P.vhs_sequence(orc, sysname, fused, noise, size, k, imgs[k], stages=True)
        b = P.vhs_sequence(ref, sysname, fused, noise, size, k, imgs[k], stages=True)
        for step in range(P.VHS_STEPS):
            for f, x, y in zip(names, a[step], b[step]):
                _same(x, y, "%s %s field %d pass %d %s" % (table, cid, k, step, f))


@pytest.mark.parametrize("tc", _ids("seeds"), ids=_name)
def test_oracle_equals_the_reference_on_the_many_seeds(tc):
    table, cid = tc
    noise = P.TABLES[table]["cases"][cid]
    orc, ref = _checkers("vhs")
    analog = P.many_seeds_analog(orc)
    _same(analog, P.many_seeds_analog(ref), "the encoded field")
    for k in range(P.MANY_SEEDS_N):
        a = P.many_seeds_sequence(orc, analog, noise, k)
        b = P.many_seeds_sequence(ref, analog, noise, k)
        for step in range(2):
            for f, x, y in zip(("inp", "out", "hsync", "vsync", "rn"), a[step], b[step]):
                _same(x, y, "seed %d noise %d call %d %s" % (P.MANY_SEEDS[k], noise, step, f))


_WILD = {}


def _wild_inputs(name, n):
    if (name, n) not in _WILD:
        _WILD.clear()                                     # one set of images at a time
        _WILD[(name, n)] = P.wild_inputs(name, n)
    return _WILD[(name, n)]


@pytest.mark.parametrize("tc", _ids("wild"), ids=_name)
def test_oracle_equals_the_reference_on_the_wild_sync_states(tc):
    """the start states and pictures of test_wild_sync_states_against_the_oracle, with that test's own exclusion: a field is left at
    the first pass in which the reference reads past inp[] + 16"""
    table, cid = tc
    name, n, noise, ks = P.TABLES[table]["cases"][cid]
    orc, ref = _checkers(name)
    inp = _wild_inputs(name, n)
    lost = 0
    for k in ks:
        o, r = P.wild_checker_crt(orc, name, inp, k), P.wild_checker_crt(ref, name, inp, k)
        for step in range(P.WILD_STEPS):
            what = "%s %s field %d (hsync0 %d vsync0 %d) pass %d" % (table, cid, k, inp["hs"][k], inp["vs"][k], step)
            P.wild_checker_modulate(o, inp["nes"])
            P.wild_checker_modulate(r, inp["nes"])
            _modulated(o, r, what)
            if _demodulate(orc, o, r, noise, what):
                lost += P.WILD_STEPS - step
                break
            _demodulated(o, r, what)
    assert lost == P.excluded(table, cid), "%s %s: %d field-passes excluded, parity_cases.EXCLUDED says %d" % (table, cid, lost, P.excluded(table, cid))


def test_wild_sync_states_keep_enough_fields():
    """that test's own rule -- at least two of three passes over the fields it looks at are compared -- on the recorded counts"""
    for name, n, noise in sorted({p[:3] for p in P.WILD_PARAMS}):
        parts = [cid for cid in P.TABLES["WILD_SYNC"]["cases"] if cid.startswith("%s-n%d-noise%d-part" % (name, n, noise))]
        assert sorted(k for cid in parts for k in P.TABLES["WILD_SYNC"]["cases"][cid][3]) == P.wild_check(n)
        lost = sum(P.excluded("WILD_SYNC", cid) for cid in parts)
        assert P.WILD_STEPS * len(P.wild_check(n)) - lost >= 2 * len(P.wild_check(n)), (name, n, noise, lost)


def test_exclusion_records_name_real_cases():
    for table, per in P.EXCLUDED.items():
        assert set(per) <= set(P.TABLES[table]["cases"]), table
        assert all(v > 0 for v in per.values()), table
    # the tables the issue measured at zero, and the ones whose GPU tests compare every field unconditionally
    for table in ("CASES", "WIDE_CASES", "RANDOM", "NES_CASES"):
        assert P.excludes_nothing(table), table
    assert all(cid.endswith("nesrgb") for cid in P.EXCLUDED.get("RANDOM_WIDE", {}))

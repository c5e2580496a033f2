"""The chains of tests/async_cases.py without a GPU: the oracle that gives their expected values is pinned to the real reference on
every class after every call, every chain can tell a stale table from a fresh one, and the tables are well-formed."""
import os

import numpy as np
import pytest

import async_cases as AC
import crtref as R

needs_ref = pytest.mark.skipif(not R.have_ref("ntsc"), reason="oracle/_ref not built (no reference sources on this machine)")


@needs_ref
@pytest.mark.parametrize("cid", AC.CHAIN_IDS)
def test_oracle_is_the_reference_on_every_class_after_every_call(cid):
    """tolerance 0, picture and (hsync, vsync, rn) and inp[]; no field may leave the comparison under the reference-UB rule
    (crtref.reads_past_inp): the chains' inputs are chosen so that none does"""
    ch = AC.get(cid)
    assert R.have_ref(ch["name"]), "no reference build of " + ch["name"]
    exp, _nxt = AC.expected(cid)
    got_all = AC.simulate(R.RefLib(ch["name"]), ch)
    compared = 0
    for u, (cls, part, fields) in enumerate(AC.units(ch)):
        for i, (w, g) in enumerate(zip(exp[u], got_all[u])):
            assert (w is None) == (g is None) == (not part[i])
            if w is None:
                continue
            what = "%s unit %d (class %d, fields %d..) call %d" % (cid, u, cls, fields[0], i)
            assert w["ub"] is False, what + ": the reference reads past inp[] here, the inputs must be chosen so that it does not"
            assert (w["hsync"], w["vsync"], w["rn"]) == (g["hsync"], g["vsync"], g["rn"]), what + ": state"
            np.testing.assert_array_equal(w["inp"], g["inp"], err_msg=what + ": inp")
            np.testing.assert_array_equal(w["out"], g["out"], err_msg=what + ": picture")
            compared += 1
    assert compared == sum(sum(part) for _cls, part, _f in AC.units(ch))


@pytest.mark.parametrize("cid", AC.CHAIN_IDS)
def test_no_expected_field_falls_under_the_ub_rule(cid):
    """(also where the reference is not built: the rule is the oracle's own trace)"""
    exp, _ = AC.expected(cid)
    bad = [(u, i) for u, per in enumerate(exp) for i, w in enumerate(per) if w is not None and w["ub"]]
    assert not bad, "%s: (unit, call) under the UB rule: %s" % (cid, bad)


@pytest.mark.parametrize("cid", AC.CHAIN_IDS)
def test_every_call_changes_the_picture_of_every_class(cid):
    """a chain whose call i leaves the picture of call i - 1 proves nothing about call i: a dropped launch would pass"""
    ch = AC.get(cid)
    exp, _ = AC.expected(cid)
    for u, per in enumerate(exp):
        for i in range(1, len(per)):
            if per[i] is None:
                continue
            mine = [j for j in range(i) if per[j] is not None and ch["steps"][j]["ctx"] == ch["steps"][i]["ctx"]]
            if ch["contexts"] > 1:
                assert not np.array_equal(per[i]["out"], per[i - 1]["out"]), "%s unit %d call %d: the other context's picture" % (cid, u, i)
            before = per[mine[-1]]["out"] if mine else np.zeros_like(per[i]["out"])
            assert not np.array_equal(per[i]["out"], before), "%s unit %d: call %d leaves the picture as it was" % (cid, u, i)


@pytest.mark.parametrize("cid", [c["id"] for c in AC.CHAINS if c["stale"]])
def test_a_stale_table_shows(cid):
    """the table, record and layout chains: call i with call i - 1's parameters (what a table, a record buffer or a layout that was
    not rewritten in time amounts to) gives another picture on every class"""
    ch = AC.get(cid)
    exp, _ = AC.expected(cid)
    orc = R.Oracle(ch["name"])
    assert len(AC.units(ch)) == AC.NCLS
    for i in range(1, len(ch["steps"])):
        for u, (cls, part, _fields) in enumerate(AC.units(ch)):
            stale = AC.run_class(orc, ch, cls, part, upto=i, stale_at=i)[i]
            assert not np.array_equal(stale["out"], exp[u][i]["out"]), "%s class %d call %d: stale parameters give the same picture" % (cid, cls, i)


def test_the_vhs_chain_has_four_generator_streams():
    ch = AC.get("vhs-side-noise")
    _exp, nxt = AC.expected("vhs-side-noise")
    assert len(set(AC.VHS_SEEDS)) == AC.NCLS // 2
    for i in range(len(ch["steps"])):
        per_image = {}
        for cls in range(AC.NCLS):
            per_image.setdefault(AC.class_image(cls), set()).add(nxt[(cls, i)])
        # the two parities of an image draw equally often from the same seed; the four images are at four places
        assert all(len(v) == 1 for v in per_image.values()), per_image
        assert len({min(v) for v in per_image.values()}) == AC.NCLS // 2
    for cls in range(AC.NCLS):
        assert len({nxt[(cls, i)] for i in range(len(ch["steps"]))}) == len(ch["steps"]), "the generator moves with every call"


def test_tables_are_well_formed():
    assert len(set(AC.CHAIN_IDS)) == len(AC.CHAIN_IDS)
    assert len(set(AC.GPU_IDS)) == len(AC.GPU_IDS)
    assert AC.N == 512 and AC.N % AC.NCLS == 0
    counts = np.bincount([AC.class_of(k) for k in range(AC.N)], minlength=AC.NCLS)
    assert (counts == AC.N // AC.NCLS).all()
    assert sorted({(AC.class_image(c), AC.class_parity(c)[0]) for c in range(AC.NCLS)}) == [(i, p) for i in range(4) for p in range(2)]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for ch in AC.CHAINS:
        assert ch["contexts"] == 1 + max(st["ctx"] for st in ch["steps"])
        assert any(st["call"] == "replay" for st in ch["steps"]) == (ch["capture"] is not None)
        us = AC.units(ch)
        # every field is in exactly one unit, of its class; behind the head every unit set holds every class
        assert sorted(k for _c, _p, fields in us for k in fields) == list(range(AC.N))
        assert all(AC.class_of(k) == cls for cls, _p, fields in us for k in fields)
        head = AC.HEAD if AC.has_seq(ch) else 0
        assert [fields for _c, _p, fields in us[:head]] == [[k] for k in range(head)] and head % AC.NCLS == 0
        assert (len(us) - head) % AC.NCLS == 0 and AC.SEQ_FIELDS <= AC.HEAD
        for st in ch["steps"]:
            assert st["call"] in ("fieldpass", "knobs", "replay", "stages", "stills", "sizes", "sequence", "sequence_sets")
            assert (st["call"] == "knobs") == (st["rows"] is not None)
            if st["rows"] is not None:
                assert len(st["rows"]) == AC.NCLS and len({len(r) for r in st["rows"]}) == 1 and len(st["rows"][0]) in (3, 8)
                assert len(set(st["rows"])) == AC.NCLS
            # the calls that wait on the host: a call over more fields than the context holds grows the workspace (the fused entry
            # points: crthip_reserve; the stage-level bloom decoder: its sort scratch), and sequence mode's sync loop
            first_big = AC.fields_of(st) > ch["reserve"] and all(AC.fields_of(q) <= ch["reserve"] for q in ch["steps"][:ch["steps"].index(st)])
            want = None
            if st["call"] in ("sequence", "sequence_sets"):
                want = AC.WAIT_SEQ
            elif first_big:
                want = AC.WAIT_BLOOM if st["call"] == "stages" else AC.WAIT_RESERVE
            assert st["waits"] == want, "%s: %s declares %s" % (ch["id"], st["call"], st["waits"])
            if st["waits"] is not None:
                path, func, line = st["waits"]
                src = open(os.path.join(root, path)).read()
                body = src[src.index("int %s(" % func):]
                body = body[:body.index("\n}\n")]
                assert line in body, "%s: %s no longer holds the declared host wait `%s`" % (path, func, line)


def test_margin_side_and_overlap_thresholds_are_the_batch_size():
    """N is the smallest batch at which both are on: read from the sources the chains are about"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dev = open(os.path.join(root, "ntsc-crt_amd", "csrc", "crt_dev.h")).read()
    host = open(os.path.join(root, "ntsc-crt_amd", "csrc", "crt_host.hip")).read()
    assert "#define MARGIN_SIDE_MIN_FIELDS %d " % AC.N in dev
    assert "n >= 256 * want_chunks" in host and 256 * max(AC.get("skeleton-churn")["overlaps"]) == AC.N


def test_layout_pingpong_takes_the_layouts_it_names():
    """crthip_signal_layout_query (host only) on the blobs of the chain: padded 100, padded 84, flat, padded 100"""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    import crtlib
    L = crtlib.load_library()
    ch = AC.get("layout-pingpong")
    got = []
    for st in ch["steps"]:
        sk, kn, noise = AC.step_params(ch, st)
        p = crtlib.make_params("ntsc", w=AC.IW, h=AC.IH, outw=AC.OUTW, outh=AC.OUTH, out_format=R.FMT_BGRA, format=R.FMT_BGRA, as_color=1,
                               hue=sk.get("hue", 0), xoffset=sk.get("xoffset", 0), yoffset=sk.get("yoffset", 0), noise=noise,
                               mon_hue=kn["hue"], **{k: kn[k] for k in ("brightness", "contrast", "saturation", "black_point", "white_point",
                                                                         "scanlines", "blend", "v_fac")})
        lay, stride = (C.c_int * 4)(), C.c_size_t(0)
        rc = L.crthip_signal_layout_query(C.byref(p), AC.N, ch["shape"], lay, C.byref(stride))
        assert rc in (0, 1)
        got.append((rc == 1, lay[1]))
    assert got == [(True, 100), (True, 84), (False, 0), (True, 100)], got
    assert [g[0] for g in got] == [st["signal"] for st in ch["steps"]]

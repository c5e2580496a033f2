"""The call programs of tests/reuse_cases.py without a GPU: every fused field-pass of every program takes the signal layout the program
says (crthip_signal_layout_query: the layout rule without a context), the programs really do change the layout from call to call (a
refactor of the rule cannot silently turn the GPU test into eight identical passes), and the oracle-only side of the exclusion caps:
how many (field, call) pairs of a program the reference-UB rule (crtref.reads_past_inp) takes out of the comparison."""
import ctypes as C

import pytest

import crtref as R
import reuse_cases as RC


@pytest.fixture(scope="module")
def crtlib():
    import __graft_entry__ as g
    g.build()
    import crtlib
    return crtlib


def _query(crtlib, prog, si):
    st = prog["steps"][si]
    p = crtlib.make_params(prog["name"], **RC.query_kwargs(prog, st))
    lay = (C.c_int * 4)()
    stride = C.c_size_t(0)
    rc = crtlib.load_library().crthip_signal_layout_query(C.byref(p), RC.fields_of(prog, st), RC.shape_at(prog, si), lay, C.byref(stride))
    assert rc in (0, 1), "%s call %d: crthip_signal_layout_query failed (%d)" % (prog["id"], si, rc)
    return rc == 1, list(lay), stride.value


@pytest.mark.parametrize("pid", RC.PROGRAM_IDS)
def test_fused_calls_take_the_layout_the_program_says(crtlib, pid):
    prog = RC.program(pid)
    hres = crtlib.load_library().crthip_hres(*R.SYSTEMS[prog["name"]][:2])
    flat_stride = crtlib.load_library().crthip_field_stride(*R.SYSTEMS[prog["name"]][:2])
    asked = 0
    for si, st in enumerate(prog["steps"]):
        if st["call"] not in RC.FUSED:
            continue                                   # sequence mode and the stage-level calls never consult the rule
        asked += 1
        padded, lay, stride = _query(crtlib, prog, si)
        what = "%s call %d (%s, %d fields, shape %d)" % (pid, si, st["call"], RC.fields_of(prog, st), RC.shape_at(prog, si))
        assert (padded, lay[1]) == st["rule"], "%s: the rule says padded=%s shift=%d" % (what, padded, lay[1])
        if padded:
            assert lay[0] > hres and lay[0] % 128 == 0 and stride > flat_stride and 80 <= lay[2] <= 96 and 0 <= lay[3] <= 16, what
        else:
            assert lay == [hres, 0, 0, 0] and stride == flat_stride, what
        # what the pass takes: the rule, unless crthip_set_signal_layout(ctx, 0) is in force
        sig_pad = 1
        for prev in prog["steps"][:si + 1]:
            sig_pad = prev["sw"].get("signal_layout", sig_pad)
        assert st["expect"] == (st["rule"] if sig_pad else RC.FLAT), what
    assert asked >= 1, pid


@pytest.mark.parametrize("pid", RC.PROGRAM_IDS)
def test_programs_change_the_layout(pid):
    prog = RC.program(pid)
    assert RC.layout_changes(prog) >= prog["min_changes"], "%s: %s" % (pid, RC.executed_layouts(prog))
    if pid.startswith("A-"):
        lays = RC.executed_layouts(prog)
        assert lays[0] == lays[1], "a pass in its predecessor's layout belongs to the program"
        assert len({l for l in lays if l[0]}) >= 3 and RC.FLAT in lays, "three shifts and the flat layout"
    if pid.startswith(("A-", "B-", "F-")):
        assert prog["min_changes"] >= 4


def test_the_ping_pong_programs_differ_only_in_noise_and_start_state():
    a = [RC.program(pid) for pid in RC.PROGRAM_IDS if pid.startswith("A-")]
    assert [(p["noise"], p["start"]) for p in a] == [(24, "ordinary"), (60, "ordinary"), (60, "wild"), (150, "wild")]
    assert all(p["steps"] == a[0]["steps"] and p["n"] == 24 and len(p["steps"]) == 8 for p in a)


@pytest.mark.parametrize("pid", RC.PROGRAM_IDS)
def test_exclusion_caps_on_the_oracle(pid):
    """conditions, not measurements: a program with an ordinary start state loses nothing to the reference-UB rule, the wild start
    states at noise 60 keep at least 90 % of their (field, call) pairs, at noise 150 two thirds (the wild-state test's rule)"""
    prog = RC.program(pid)
    run = RC.OracleRun(prog)
    for si in range(len(prog["steps"])):
        run.run(si)
    print("%s: %d of %d (field, call) pairs kept, %d of %d fields lost" % (pid, run.kept, run.total, sum(run.ub.values()), len(run.ub)))
    assert run.total > 0
    if pid.startswith("A-"):
        assert run.total == 192
    if prog["keep"] == 1.0:
        assert run.kept == run.total, "%s: %d of %d pairs fall under the UB rule, none may" % (pid, run.total - run.kept, run.total)
    else:
        assert run.kept >= prog["keep"] * run.total, "%s: only %d of %d pairs kept" % (pid, run.kept, run.total)

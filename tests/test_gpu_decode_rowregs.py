"""k_decode keeps its row tables in registers: every lane fetches the source pointer, destination pointer and row count of the rows it
fills and drains from the lanes that own them (crt_decode_lane.h).  A wrong fetched row shows where the row bookkeeping is least
regular, so the cases sit there: batches whose last wavefront is partial and whose wavefronts straddle field boundaries (240 lines
per field, 64 per wavefront), widths with a partial last pixel tile and a partial last 16-byte piece, a height with duplicated rows
and one with several rank passes and lines that write nothing, the 4-byte drain (in-register and permuted byte order) and the 3-byte
drain, with and without blend, the float and the integer stages, the bloom and the picture-knob instantiations (other translation
units) and tier group 1.

Every case runs ONCE on fenced buffers (tests/fence.py, through the Run of tests/test_gpu_fence.py): the payloads equal the oracle
bit for bit and no byte outside them has changed -- a wrong pointer is a fence hit here, not a fault."""
import pytest

import crtref as R
import fence_cases as FC
from test_gpu_fence import Run, crtlib  # noqa: F401  (crtlib: the module's fixture)

pytestmark = pytest.mark.gpu
SEED = FC.FILL_SEEDS[0]


def _case(tag, n, outw, outh, ofmt, blend, dec_float=True, **kw):
    fmt = {R.FMT_BGRA: "bgra", R.FMT_ARGB: "argb", R.FMT_RGB: "rgb"}[ofmt]
    cid = "rowregs-%s-n%d-%dx%d-%s-b%d-%s" % (tag, n, outw, outh, fmt, blend, "f" if dec_float else "i")
    four = ofmt in FC.F4
    knobs = dict(kw.pop("knobs", {}), blend=blend)
    c = FC.C(cid, n=n, outw=outw, outh=outh, ofmt=ofmt, knobs=knobs, img=FC.IMG4[n % 4], out=(FC.OUT4 if four else FC.OUT3)[(n + blend) % 4], **kw)
    return c, dec_float


def _cases():
    cs = []
    # fields x widths; heights, formats, blend and the stages' arithmetic take turns.  have = pixels of the last 16-byte piece:
    # 641 -> 1, 642 -> 2, 99 -> 3 (100 and 16: whole pieces, a partial / a single tile)
    fmts = (R.FMT_BGRA, R.FMT_ARGB, R.FMT_RGB)
    i = 0
    for n in (1, 2, 3, 5):
        for outw in (100, 641, 16):
            outh = (241, 720, 100)[(i + n) % 3]
            cs.append(_case("grid", n, outw, outh, fmts[i % 3], i & 1, dec_float=(i % 4) != 3))
            i += 1
    for outw, ofmt in ((642, R.FMT_ARGB), (99, R.FMT_BGRA), (99, R.FMT_RGB)):
        cs.append(_case("have", 3, outw, 77, ofmt, 1))
    # row duplicates (nr > 1) and rank passes with lines of no rows, each with every drain
    for ofmt in fmts:
        cs.append(_case("dup", 2, 100, 720, ofmt, ofmt == R.FMT_ARGB))
        cs.append(_case("rank", 5, 100, 100, ofmt, ofmt != R.FMT_ARGB, dec_float=ofmt != R.FMT_BGRA))
    # the instantiations of the other translation units: a bloom library, a picture-knob call (integer stages, per-lane knobs;
    # all fields at the context's own brightness and contrast, which is what the oracle of fence_cases.py is given)
    cs.append(_case("bloom", 3, 100, 241, R.FMT_BGRA, 1, name="ntscbloom"))
    cs.append(_case("bloom", 2, 16, 100, R.FMT_RGB, 0, name="ntscbloom"))
    pic = [(24, 0, 10, 9, 170), (0, 17, 14, 9, 170), (12, -20, 6, 9, 170)]
    cs.append(_case("picknobs", 3, 100, 241, R.FMT_BGRA, 0, triples=pic, knobs=dict(brightness=9, contrast=170)))
    cs.append(_case("picknobs", 3, 641, 100, R.FMT_RGB, 1, triples=pic, knobs=dict(brightness=9, contrast=170)))
    # tier group 1: the 24-bit tier forced (crthip_set_exact 2)
    cs.append(_case("tier2", 3, 100, 241, R.FMT_ARGB, 1, exact=2))
    cs.append(_case("tier2", 5, 641, 100, R.FMT_RGB, 0, exact=2))
    return cs


CASES = _cases()
assert len({c["id"] for c, _ in CASES}) == len(CASES)


@pytest.mark.parametrize("c,dec_float", CASES, ids=[c["id"] for c, _ in CASES])
def test_row_tables_in_registers(crtlib, monkeypatch, c, dec_float):  # noqa: F811
    monkeypatch.setenv("CRTHIP_DEC_FLOAT", "1" if dec_float else "0")       # read when the context is created
    r = Run(crtlib, c, SEED)
    try:
        r.call()
        r.check()
        if c["kind"] == "fieldpass" and not c["triples"] and c["name"] == "ntsc" and not c["exact"]:
            assert r.fstage == int(dec_float), "%s: float stages %d" % (c["id"], r.fstage)
    finally:
        r.close()

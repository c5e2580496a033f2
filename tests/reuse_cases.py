"""Call programs for ONE long-lived context (tests/test_gpu_context_reuse.py runs them on the GPU, tests/test_context_reuse_cpu.py
checks their layouts and their exclusion caps without one); no tests in here.

A program is an ordered list of calls on one crthip context.  What a context carries from call to call: the signal workspace d_inp,
shared by the reference's flat lines and the padded lines of the fused path (crt_dev.h, sig_layout) and zeroed once, when it is
reserved; the encoder's cached tables; the layout of the last pass (crthip_fieldpass_signal); the bloom decoder's sort scratch.  Every
entry names the entry point, the fields of the call, the settings, the monitor knobs, the switches to set first and -- for a fused
field-pass -- the signal layout the pass must take: (padded, shift).  Expected pictures and states never come from the library: the
oracle runs every field with the batch semantics of the existing GPU tests (analog[] clean before every crt_modulate, sync state and
output buffer carried over).

The expected layouts follow from the geometry (crt_setup.c / crt_host.hip, layout_rule): the active row of standard NTSC starts at
xo = (156 + xoffset) & ~3 and is 753 samples long, a line has 910, `shift` = (128 - xo % 128) % 128 puts the row on a 128-byte
boundary, and a row that overhangs its line by more than 16 samples (xoffset 24: 23) does not fit the padded lines.  The SNES's row
starts at 196 (shift 60), the bloom build's narrower one at 212 (shift 44)."""
import numpy as np

import crtref as R
import seqsets_cases as SC

# the start states of tests/test_gpu_parity.py:test_wild_sync_states_against_the_oracle
HS0 = [0, 3, 30, 60, 140, 300, 500, 700, 880, 892, 905, 909]
VS0 = [0, 4, 9, 100, 180, 250, 255, 258, 261]
DEFAULT_KNOBS = dict(hue=0, brightness=0, contrast=180, saturation=10, black_point=0, white_point=100, scanlines=0, blend=0, v_fac=0)
FLAT = (False, 0)
FUSED = ("fieldpass", "capture", "replay")            # the calls whose layout comes from the rule (crt_fused_layout)
INIT_SEED = 5                                         # the output buffer's content before a sequence call's first field


def P(shift):
    return (True, shift)


def fp(call="fieldpass", m=None, sk=None, knobs=None, sw=None, expect=FLAT, rule=None, img=0, noise=None, reset=False, set_first=None, par=None):
    """one call.  m: fields of the call (None: the whole batch);  sk: NTSC_SETTINGS members;  knobs: struct CRT members (absolute: what
    is not named is at its crt_init value);  sw: crthip_set_<name>(value) to call first (they stay);  expect: the layout the pass takes;
    rule: what the layout rule alone says where a switch overrides it;  img: which set of images;  reset: the test resets ITS
    television sets (state, output buffer) first -- the context stays as old as it is;  par: the call whose field parities this one
    shows (a replayed graph: the captured call's)"""
    return dict(call=call, m=m, sk=sk or {}, knobs=knobs or {}, sw=sw or {}, expect=expect, rule=rule if rule is not None else expect,
                img=img, noise=noise, reset=reset, set_first=set_first, par=par)


def _xy(x, y, **kw):
    return dict(xoffset=x, yoffset=y, **kw)


def _prog(id, name, n, outw, outh, iw, ih, steps, shape=1, noise=24, start="ordinary", keep=1.0, min_changes=0, same_images=False,
          stream=False, seed=4000, scanlines=1):
    """keep: the share of (field, call) pairs that must stay in the comparison (1.0: none may fall under the reference-UB rule);
    min_changes: how often at least the layout of a fused pass differs from the previous call's"""
    return dict(id=id, name=name, n=n, outw=outw, outh=outh, ofmt=R.FMT_BGRA, iw=iw, ih=ih, steps=steps, shape=shape, noise=noise,
                start=start, keep=keep, min_changes=min_changes, same_images=same_images, stream=stream, seed=seed, scanlines=scanlines)


def _pingpong():
    """A: padded, padded again, padded with another shift, the flat fallback, back, another shift through the other encoder, flat by
    the switch, padded"""
    return [fp(sk=_xy(0, 0), expect=P(100)),
            fp(sk=_xy(0, 0), expect=P(100)),
            fp(sk=_xy(16, 1), expect=P(84)),
            fp(sk=_xy(24, 1), expect=FLAT),
            fp(sk=_xy(0, 0), sw=dict(signal_tile=32), expect=P(100)),
            fp(sk=_xy(4, 0), sw=dict(shape=2), expect=P(96)),
            fp(sk=_xy(0, 0), sw=dict(shape=1, signal_layout=0), expect=FLAT, rule=P(100)),
            fp(sk=_xy(16, 1), sw=dict(signal_layout=1, signal_tile=0), expect=P(84))]


def _entry_points(shift):
    return [fp(expect=P(shift)),
            fp("sequence", img=1, set_first=[0, 9]),
            fp(expect=P(shift), img=2, reset=True),
            fp("sequence_sets", img=3, set_first=[0, 3, 9]),
            fp(expect=P(shift), img=4, reset=True),
            fp("stages", img=5),
            fp(expect=P(shift), img=6)]


_NES_BASE = dict(hue=20, border_color=0x21)
_NES_CHURN = [fp(sk=dict(_NES_BASE)),
              fp(sk=dict(_NES_BASE, border_color=0x16), img=1),
              fp(sk=dict(_NES_BASE), img=2),
              fp(sk=dict(_NES_BASE), knobs=dict(black_point=6, white_point=90), img=3),
              fp(sk=dict(_NES_BASE), img=4),
              fp(sk=dict(_NES_BASE, yoffset=3), img=5),
              fp(sk=dict(_NES_BASE), img=6),
              fp(sk=dict(_NES_BASE, hue=0), img=7),
              fp(sk=dict(_NES_BASE), img=8)]

PROGRAMS = [
    # A. layout ping-pong; the counts of the caps: 24 fields x 8 calls on the oracle (tests/test_context_reuse_cpu.py recounts them)
    _prog("A-ordinary-noise24", "ntsc", 24, 640, 480, 640, 480, _pingpong(), noise=24, min_changes=6, same_images=True),
    _prog("A-ordinary-noise60", "ntsc", 24, 640, 480, 640, 480, _pingpong(), noise=60, min_changes=6, same_images=True),
    _prog("A-wild-noise60", "ntsc", 24, 640, 480, 640, 480, _pingpong(), noise=60, start="wild", keep=0.9, min_changes=6, same_images=True),
    _prog("A-wild-noise150", "ntsc", 24, 640, 480, 640, 480, _pingpong(), noise=150, start="wild", keep=2.0 / 3, min_changes=6, same_images=True),
    # B. the library's own choice of shape: the batch size crosses ROWS_SHAPE_MAX_FIELDS_ENC = 256 on a context reserved for 300
    _prog("B-batch-size", "ntsc", 300, 96, 240, 64, 48,
          [fp(m=300, expect=P(100)), fp(m=40, img=1), fp(m=300, expect=P(100), img=2), fp(m=257, expect=P(100), img=3), fp(m=256, img=4),
           fp(m=300, expect=P(100), img=5)], shape=0, min_changes=4),
    # C. the entry points interleaved: sequence mode and the stage-level calls between fused passes
    _prog("C-entry-points-ntsc", "ntsc", 9, 640, 480, 640, 480, _entry_points(100), min_changes=0),
    _prog("C-entry-points-snes", "snes", 9, 640, 480, 640, 480, _entry_points(60), min_changes=0),
    # D. the cached tables and the decoder tiers: every key changed and changed back
    _prog("D-tables-ntsc", "ntsc", 6, 640, 480, 640, 480,
          [fp(sk=dict(hue=0), expect=P(100)), fp(sk=dict(hue=77), expect=P(100), img=1), fp(sk=dict(hue=0), expect=P(100), img=2),
           fp(sk=dict(hue=-57), expect=P(100), img=3), fp(sk=dict(hue=-57, as_color=0), expect=P(100), img=4),
           fp(sk=dict(hue=0, as_color=1), knobs=dict(saturation=40), expect=P(100), img=5),
           fp(sk=dict(hue=0), knobs=dict(saturation=900), expect=P(100), img=6), fp(sk=dict(hue=0), expect=P(100), img=7)]),
    _prog("D-tables-nes", "nes", 4, 640, 480, 256, 240, _NES_CHURN, noise=12),
    _prog("D-tables-nesborder", "nesborder", 4, 640, 480, 256, 240, _NES_CHURN, noise=12),
    _prog("D-bloom-scratch", "ntscbloom", 12, 640, 480, 320, 240,
          [fp(m=12, expect=P(44)), fp(m=5, knobs=dict(brightness=40), expect=P(44), img=1), fp(m=12, knobs=dict(saturation=19), expect=P(44), img=2),
           fp(m=7, expect=P(44), img=3), fp(m=12, knobs=dict(saturation=40), expect=P(44), img=4)]),
    # E. a refused call in the middle: by check_encoder (nothing enqueued), and by the decoder's checks (encoder and sync chain enqueued)
    _prog("E-refused", "ntsc", 4, 640, 480, 640, 480,
          [fp(expect=P(100)), fp("refused_encoder", sk=_xy(-400, 0), img=1), fp(expect=P(100), img=2),
           fp("refused_decoder", sk=_xy(16, 1), img=3), fp(expect=P(100), img=4)]),
    # F. a kept graph of a padded pass, replayed between eager passes that leave the workspace in other layouts
    _prog("F-kept-graph", "ntsc", 4, 640, 480, 640, 480,
          [fp("capture", expect=P(100)), fp(sk=_xy(24, 1), img=1), fp("replay", expect=P(100), par=0), fp(sk=_xy(24, 1), img=2),
           fp("replay", expect=P(100), par=0), fp(sk=_xy(16, 1), expect=P(84), img=3), fp("replay", expect=P(100), par=0),
           fp(sw=dict(signal_layout=0), rule=P(100), img=4)], min_changes=6, stream=True),
]
PROGRAM_IDS = [p["id"] for p in PROGRAMS]


def program(id):
    return PROGRAMS[PROGRAM_IDS.index(id)]


def is_nes(prog):
    return R.SYSTEMS[prog["name"]][0] == R.SYS_NES


def fields_of(prog, st):
    return prog["n"] if st["m"] is None else st["m"]


def checked_fields(prog):
    """fields are independent, so a subset is exact: every 7th, the last, and the last of every partial call"""
    n = prog["n"]
    if n <= 64:
        return list(range(n))
    ks = set(range(0, n, 7)) | {n - 1}
    for st in prog["steps"]:
        ks.add(fields_of(prog, st) - 1)
        ks.add(min(fields_of(prog, st), n - 1))        # ... and the first field a partial call must leave alone
    return sorted(ks)


def noise_of(prog, st):
    return prog["noise"] if st["noise"] is None else st["noise"]


def knobs_of(prog, st):
    return dict(DEFAULT_KNOBS, scanlines=prog["scanlines"], **st["knobs"])


def images(prog, st):
    """[n, ih, iw, 4] bytes (the NES: [n, 240, 256] PPU pixels) of image set st["img"]; program A shows the pictures of the wild-state
    test in every call (its caps were counted with them)"""
    n, iw, ih = prog["n"], prog["iw"], prog["ih"]
    if prog["same_images"]:
        base = np.stack([R.synth_image(iw, ih, 4, 8100 + k, "bars" if k % 3 == 1 else "random") for k in range(n)])
        base[2::3] //= 16
        return base
    seed = prog["seed"] + 1000 * st["img"]
    if is_nes(prog):
        return np.stack([R.synth_ppu(iw, ih, seed + k) for k in range(n)])
    return np.stack([R.synth_image(iw, ih, 4, seed + k, "bars" if (k + st["img"]) % 4 == 1 else "random") for k in range(n)])


def parity(prog, si, k):
    """(field, frame, dot_crawl_offset) of field k in fused / stage-level call si"""
    par = prog["steps"][si]["par"]
    si = si if par is None else par
    if prog["same_images"]:
        return (k + si) & 1, 0, 0
    return (k + si) & 1, (k >> 1) & 1, (k + si) % 3


def start_state(prog, k):
    """(hsync, vsync) of field k before the first call"""
    return (HS0[k % len(HS0)], VS0[k % len(VS0)]) if prog["start"] == "wild" else (0, 0)


def query_kwargs(prog, st):
    """crtlib.make_params keywords of a fused call (crthip_signal_layout_query takes the finalized blob)"""
    sk = st["sk"]
    kw = dict(w=prog["iw"], h=prog["ih"], outw=prog["outw"], outh=prog["outh"], out_format=prog["ofmt"], hue=sk.get("hue", 0),
              xoffset=sk.get("xoffset", 0), yoffset=sk.get("yoffset", 0), noise=noise_of(prog, st))
    if not is_nes(prog):
        kw.update(format=R.FMT_BGRA, as_color=sk.get("as_color", 1))
    kn = knobs_of(prog, st)
    kw.update(mon_hue=kn["hue"], **{k: kn[k] for k in ("brightness", "contrast", "saturation", "black_point", "white_point", "scanlines", "blend", "v_fac")})
    return kw


def shape_at(prog, si):
    """crthip_set_shape's value when call si runs"""
    shape = prog["shape"]
    for st in prog["steps"][:si + 1]:
        shape = st["sw"].get("shape", shape)
    return shape


def executed_layouts(prog):
    """the layouts the workspace takes, call by call (a capture runs nothing; sequence mode and the stage-level calls of the tests
    keep the reference's flat lines)"""
    return [st["expect"] if st["call"] in FUSED else FLAT for st in prog["steps"] if st["call"] not in ("capture", "refused_encoder", "refused_decoder")]


def layout_changes(prog):
    lays = executed_layouts(prog)
    return sum(1 for a, b in zip(lays, lays[1:]) if a != b)


def seq_case(prog, st):
    """the seqsets_cases case of a sequence / sequence_sets call"""
    return dict(id="%s call" % prog["id"], name=prog["name"], outw=prog["outw"], outh=prog["outh"], ofmt=prog["ofmt"],
                knobs={k: v for k, v in knobs_of(prog, st).items() if v != DEFAULT_KNOBS[k] or k == "scanlines"}, mode="keep",
                noise=noise_of(prog, st), set_first=st["set_first"], progressive=False, init="shared")


def seq_init(prog):
    size = prog["outh"] * prog["outw"] * R.bpp4fmt(prog["ofmt"])
    return R.lcg_bytes(size, INIT_SEED).reshape(prog["outh"], prog["outw"], -1)


class OracleRun:
    """the television sets of a program on the oracle: one struct CRT per checked field, the reference-UB rule (crtref.reads_past_inp:
    a field that once read past inp[] + 16 leaves the comparison from that call on)"""

    def __init__(self, prog):
        self.prog = prog
        self.orc = R.Oracle(prog["name"])
        self.fields = checked_fields(prog)
        self.ub = {k: False for k in self.fields}
        self.kept = self.total = 0
        self.reset()
        for k, c in self.crts.items():
            hs, vs = start_state(prog, k)
            c.set("hsync", hs)
            c.set("vsync", vs)

    def reset(self):
        p = self.prog
        self.crts = {k: self.orc.new_crt(p["outw"], p["outh"], p["ofmt"]) for k in self.fields}

    def _settings(self, c, si, k, img):
        p, st = self.prog, self.prog["steps"][si]
        sk = st["sk"]
        field, frame, dco = parity(p, si, k)
        pad = np.concatenate([img, img[-1:]], axis=0)
        geo = dict(hue=sk.get("hue", 0), xoffset=sk.get("xoffset", 0), yoffset=sk.get("yoffset", 0))
        if is_nes(p):
            c.settings(pad, w=p["iw"], h=p["ih"], dot_crawl_offset=dco, border_color=sk.get("border_color", 0), **geo)
        else:
            c.settings(pad, format=R.FMT_BGRA, w=p["iw"], h=p["ih"], as_color=sk.get("as_color", 1), field=field, frame=frame, **geo)
            if self.orc.system in R.DOT_CRAWL_SYSTEMS:
                c.sset("dot_crawl_offset", dco)

    def fieldpass(self, si):
        """one fused (or stage-level) call -> {field: None under the UB rule, else dict(out, hsync, vsync, rn, ccf, inp)}"""
        p, st = self.prog, self.prog["steps"][si]
        if st["reset"]:
            self.reset()
        imgs = images(p, st)
        res = {}
        for k in self.fields:
            if k >= fields_of(p, st):
                continue
            c = self.crts[k]
            for name, v in knobs_of(p, st).items():
                c.set(name, v)
            self._settings(c, si, k, imgs[k])
            c.analog[:] = 0                            # batch semantics: every field-pass starts from a clean analog[]
            if self.orc.system in R.PROGRESSIVE_SYSTEMS:   # the NES's timing: the field is set up again
                c.sset("field_initialized", 0)
            c.modulate()
            hs_before = c.get("hsync")
            c.demodulate(noise_of(p, st), trace=True)
            self.ub[k] = self.ub[k] or R.reads_past_inp(self.orc, c.trace, c.get("vsync"), hs_before)
            self.total += 1
            self.kept += 0 if self.ub[k] else 1
            res[k] = None if self.ub[k] else dict(out=c.out.copy(), hsync=c.get("hsync"), vsync=c.get("vsync"), rn=c.get("rn"),
                                                  ccf=c.ccf.copy(), inp=np.asarray(c.inp).copy())
        return res

    def sequence(self, si):
        """a sequence / sequence_sets call: the reference's serial loop once per set, from the incoming states of
        seqsets_cases -> {field: dict(out, hsync, vsync, rn)}; the loops assert that no field falls under the UB rule"""
        p, st = self.prog, self.prog["steps"][si]
        case = seq_case(p, st)
        fr, par, dco = images(p, st), SC.parities(case), SC.dot_crawl(case)
        res = {}
        for s, (lo, hi) in enumerate(SC.sets_of(case)):
            want = SC.live_loop(self.orc, case, fr, par, dco, lo, hi, seq_init(p), SC.incoming(case)[s], check_reads=True)
            for k in range(lo, hi):
                o, hs, vs, rn = want[k - lo]
                res[k] = dict(out=o, hsync=hs, vsync=vs, rn=rn)
                self.total += 1
                self.kept += 1
        return res

    def run(self, si):
        call = self.prog["steps"][si]["call"]
        if call in ("fieldpass", "stages", "replay"):
            return self.fieldpass(si)
        if call in ("sequence", "sequence_sets"):
            return self.sequence(si)
        return {}                                      # a capture and a refused call compute nothing

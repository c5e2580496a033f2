"""Call chains that are enqueued WITHOUT host synchronisation (tests/test_gpu_async.py runs them on the GPU, tests/test_async_cpu.py
checks their tables and their expected values without one); no tests in here.

A chain is an ordered list of calls on one crthip context (two for `two-contexts-one-stream`).  Every other GPU test waits on the
host between library calls; these chains are enqueued behind a device-side delay, so every call is issued while the work of all
earlier ones is still pending.  What orders that work is the library's own plumbing ("Asynchronous call
chains": the inventory of every object an earlier call may still be using and the edge that protects it).

A batch has N = 512 fields: the smallest size at which k_margin runs on the internal stream beside k_active (MARGIN_SIDE_MIN_FIELDS,
crt_dev.h) and at which crthip_set_overlap(2) cuts the batch in two (fieldpass_body, crt_host.hip).  It is built from 4 distinct
images x 2 parities, all from the power-on state: field k belongs to class k % 8, so the oracle carries 8 television sets through a
chain serially and every one of the 512 fields is compared with its class.  The VHS chain gives the 4 images 4 distinct srand()
seeds.  Where calls cover fewer fields (growth) or couple fields to each other (sequence mode on fields [0, 9)), the fields that went
through different calls are units of their own (units()).  Expected values never come from the library."""
import ctypes as C
import functools

import numpy as np

import crtref as R

N, NCLS = 512, 8
IW, IH, OUTW, OUTH = 64, 48, 96, 240                  # (the NES chains: 256 x 240 PPU pixels)
NES_IW, NES_IH = 256, 240
VHS_SEEDS = [11, 4242, 90001, 777]                    # one per image: srand(seed) before the first call of the class
IMG_SEED = 7300
DEFAULT_KNOBS = dict(hue=0, brightness=0, contrast=180, saturation=10, black_point=0, white_point=100, scanlines=1, blend=0, v_fac=0)
STREAMS = ("current", "own")                          # torch's current stream; a torch.cuda.Stream of the test's own (use_stream)

# the calls that wait on the host by design, with the line that waits (tests/test_async_cpu.py checks that the line says so)
WAIT_RESERVE = ("ntsc-crt_amd/csrc/crt_host.hip", "crthip_reserve", "HIPCHK(c, hipStreamSynchronize(c->stream));")
WAIT_BLOOM = ("ntsc-crt_amd/csrc/crt_decode3.hip", "crt_reserve_bloom", "HIPCHK(c, hipStreamSynchronize(c->stream));")
WAIT_SEQ = ("ntsc-crt_amd/csrc/crt_host.hip", "seq_converge", "HIPCHK(c, hipStreamSynchronize(c->stream));")   # the sync loop reads its flag
STILLS_SCHED = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]       # the passes of a `stills` call: 4 distinct entries
SIZES = [(64, 48), (40, 48), (64, 30), (33, 17)]                  # (w, h) of image i in a `sizes` call: its top-left corner
HEAD = 16                                                         # a chain with sequence calls: fields [0, HEAD) are sets of their own
SEQ_FIELDS, SETS_FIRST = 9, [0, 3, 9]
SEQ_INIT_SEED = 5


def fp(call="fieldpass", sk=None, knobs=None, rows=None, ctx=0, m=None, signal=None, waits=None, noise=None):
    """one call.  call: fieldpass | stages (crthip_modulate, _noise, _sync, _decode on the test's own analog / inp / line buffers) |
    stills (crthip_stills, STILLS_SCHED, at the call's noise) | sizes (crthip_fieldpass_sizes on records uploaded before the chain:
    image i is its SIZES[i] corner) | sequence / sequence_sets (fields [0, 9) as consecutive fields of one / two television sets
    whose incoming state is what fields 0 / 0 and 3 hold, output buffer preset to seq_init()) | knobs (crthip_fieldpass_knobs on the
    records the test put in place on-stream) | replay (of the chain's captured call);  sk: NTSC_SETTINGS members;  knobs: struct CRT members (absolute);  rows: per CLASS one (noise, mon_hue,
    saturation) or (noise, mon_hue, saturation, brightness, contrast, black_point, white_point, hue) -- (n, 8) records bind levels
    and hues, (n, 3) records unbind them;  ctx: which context;  m: fields of the call (None: all N);  signal: the `padded` flag
    crthip_fieldpass_signal must report, its result copied out on-stream (None: not asked);  waits: None = asynchronous, else
    (file, function, source line) of the host wait the call makes by design"""
    return dict(call=call, sk=dict(sk or {}), knobs=dict(knobs or {}), rows=rows, ctx=ctx, m=m, signal=signal, waits=waits, noise=noise)


def chain(id, name, steps, noise=24, shape=1, capture=None, reserve=N, contexts=1, stale=False, overlaps=(1, 2)):
    """capture: the call that is recorded into a graph before the chain starts (its replays are steps);  reserve: crthip_reserve
    before the chain;  stale: the stale-table control applies (tests/test_async_cpu.py: every call's expected picture differs from
    what the call gives with the PREVIOUS call's parameters)"""
    return dict(id=id, name=name, steps=steps, noise=noise, shape=shape, capture=capture, reserve=reserve, contexts=contexts,
                stale=stale, overlaps=overlaps)


def _xy(x, y, hue=0):
    return dict(xoffset=x, yoffset=y, hue=hue)


_NES = dict(hue=20, border_color=0x21)
_NES_STEPS = [fp(sk=_NES),
              fp(sk=dict(_NES, border_color=0x16), knobs=dict(black_point=6, white_point=90)),
              fp(sk=_NES),
              fp(sk=dict(_NES, border_color=0x16, yoffset=3), knobs=dict(black_point=10, white_point=95)),
              fp(sk=dict(_NES, border_color=0x05), knobs=dict(black_point=6, white_point=90)),
              fp(sk=_NES)]
_NES_GRAPH = dict(capture=fp(sk=_NES),
                  steps=[fp(sk=dict(_NES, hue=0), knobs=dict(black_point=6, white_point=90)), fp("replay"), fp(sk=_NES), fp("replay"), fp("replay")])

# per-class knob rows of `records-rewritten`: (noise, mon_hue, saturation, brightness, contrast, black_point, white_point, hue)
ROWS_A = [(24, 0, 10, 0, 180, 0, 100, 0), (12, 20, 14, 10, 170, 4, 96, 33), (0, -30, 6, -8, 190, 0, 90, -57), (30, 77, 12, 0, 180, 8, 100, 120),
          (24, 5, 18, 5, 160, 2, 98, 200), (6, -77, 10, -4, 185, 0, 100, -123), (18, 45, 8, 0, 175, 6, 94, 15), (24, 0, 16, 12, 180, 0, 92, 300)]
ROWS_B = [(r[0] ^ 6, r[1] + 40, r[2] + 3, -r[3], r[4] - 10, (r[5] + 5) % 11, r[6] - 3, r[7] + 90) for r in ROWS_A]
ROWS_C = [(20, 0, 10), (24, 33, 7), (10, -33, 15), (24, 90, 12), (0, 10, 20), (28, -10, 9), (16, 60, 11), (24, -60, 13)]

CHAINS = [
    # every call rebuilds d_skel (burst by hue, yo by yoffset) while the previous call's k_margin may be on the internal stream
    chain("skeleton-churn", "ntsc", [fp(sk=_xy(0, 0, 0)), fp(sk=_xy(0, 0, 77)), fp(sk=_xy(0, 1, 0)), fp(sk=_xy(0, 1, 77)),
                                     fp(sk=_xy(0, 0, -57)), fp(sk=_xy(0, 1, 0))], stale=True),
    # ... and d_nes_tab (black and white point), with the border colour of the NES_BORDER build in the skeleton's key
    chain("nes-table-churn", "nes", _NES_STEPS, noise=12, stale=True),
    chain("nes-table-churn-border", "nesborder", _NES_STEPS, noise=12, stale=True),
    # padded (shift 100), padded (shift 84), flat, padded: the same bytes of d_inp in three layouts; the signal copied out on-stream
    chain("layout-pingpong", "ntsc", [fp(sk=_xy(0, 0), signal=True), fp(sk=_xy(16, 1), signal=True), fp(sk=_xy(24, 1), signal=False),
                                      fp(sk=_xy(0, 0), signal=True)], stale=True),
    # the caller's record buffers overwritten by a device copy between the calls; levels and hues bound, rebound, unbound
    chain("records-rewritten", "ntsc", [fp("knobs", rows=ROWS_A), fp("knobs", rows=ROWS_B), fp("knobs", rows=ROWS_C)], stale=True),
    # a kept graph replayed between eager calls that rebuild the tables (into the alternate buffer: the graph reads the first)
    chain("graph-between-eager", "ntsc", [fp(sk=dict(hue=77)), fp("replay"), fp(sk=dict(hue=0)), fp("replay"), fp("replay")],
          capture=fp(sk=dict(hue=0))),
    chain("graph-between-eager-nes", "nes", _NES_GRAPH["steps"], noise=12, capture=_NES_GRAPH["capture"]),
    # the sort scratch (hist, cursor, perm) and k_bloom_clear of call i + 1 behind the decoder of call i
    chain("bloom-sort", "ntscbloom", [fp(), fp(knobs=dict(brightness=40)), fp(knobs=dict(saturation=19)), fp(knobs=dict(saturation=40, brightness=-20))]),
    # rand()'s history carried from call to call through d_vhs_next -> d_vhs_hist on the side branch of the noise stage
    chain("vhs-side-noise", "vhs", [fp(), fp(), fp(), fp()], noise=12, shape=0),
    # a context reserved for 64 fields: a 64-field call and at once a 512-field one, whose crthip_reserve waits and frees
    chain("growth", "ntsc", [fp(m=64), fp(sk=dict(hue=77), waits=WAIT_RESERVE)], reserve=64),
    chain("growth-bloom", "ntscbloom", [fp("stages", m=64), fp("stages", sk=dict(hue=77), waits=WAIT_BLOOM)], reserve=64),
    # the entry points that share d_inp, d_lines, d_still_sig and the record buffers, one after the other
    chain("entry-points", "ntsc", [fp(), fp("stages", sk=dict(hue=30)), fp("knobs", rows=ROWS_C), fp("stills", noise=0), fp("sizes", sk=dict(hue=-40)),
                                   fp("knobs", rows=ROWS_A), fp(sk=dict(hue=77))]),
    # sequence mode (which waits on the host in its sync loop) between field-passes that must not be disturbed
    chain("sequence-between", "ntsc", [fp(), fp("sequence", m=SEQ_FIELDS, waits=WAIT_SEQ), fp(sk=dict(hue=77)),
                                       fp("sequence_sets", m=SEQ_FIELDS, waits=WAIT_SEQ), fp(sk=dict(hue=0))]),
    # two contexts with different hue and layout (padded / flat) alternate on one caller stream
    chain("two-contexts-one-stream", "ntsc", [fp(sk=_xy(0, 0, 0), ctx=0), fp(sk=_xy(24, 1, 77), ctx=1), fp(sk=_xy(0, 0, 0), ctx=0),
                                              fp(sk=_xy(24, 1, 77), ctx=1), fp(sk=_xy(0, 0, 0), ctx=0), fp(sk=_xy(24, 1, 77), ctx=1)], contexts=2),
]
CHAIN_IDS = [c["id"] for c in CHAINS]
GPU_IDS = [(c["id"], ov, st) for c in CHAINS for ov in c["overlaps"] for st in STREAMS]


def get(id):
    return CHAINS[CHAIN_IDS.index(id)]


def is_nes(ch):
    return R.SYSTEMS[ch["name"]][0] == R.SYS_NES


def is_vhs(ch):
    return R.SYSTEMS[ch["name"]][0] == R.SYS_VHS


def class_of(k):
    return k % NCLS


def class_image(c):
    return c >> 1


def class_parity(c):
    """(field, frame, dot_crawl_offset) of a class: the columns of the state tensor the test loads ONCE, before the chain"""
    return c & 1, 0, c & 1


def image_size(ch):
    return (NES_IW, NES_IH) if is_nes(ch) else (IW, IH)


@functools.lru_cache(maxsize=None)
def _images(nes):
    if nes:
        return np.stack([R.synth_ppu(NES_IW, NES_IH, IMG_SEED + i) for i in range(NCLS // 2)])
    return np.stack([R.synth_image(IW, IH, 4, IMG_SEED + i, "bars" if i == 1 else "random") for i in range(NCLS // 2)])


def images(ch):
    """the 4 distinct images of a chain: [4, ih, iw, 4] bytes, the NES: [4, 240, 256] PPU pixels"""
    return _images(is_nes(ch))


def fields_of(st):
    return N if st["m"] is None else st["m"]


def step_params(ch, st):
    """what the call's blob is made of: (sk, struct CRT knobs, noise) -- a replay: the captured call's"""
    src = ch["capture"] if st["call"] == "replay" else st
    return src["sk"], dict(DEFAULT_KNOBS, **src["knobs"]), ch["noise"] if src["noise"] is None else src["noise"]


def has_seq(ch):
    return any(st["call"] in ("sequence", "sequence_sets") for st in ch["steps"])


def units(ch):
    """fields with the same image, parity and calls behind them have the same expectation: one UNIT per class and per distinct tuple
    of (takes part in call i) -- [(class, (bool per call), [fields])].  A chain with sequence calls couples its first fields to each
    other: there the fields [0, HEAD) are units of their own (unit k = field k), the classes start behind them."""
    head = HEAD if has_seq(ch) else 0
    out = [(class_of(k), tuple(fields_of(st) > k for st in ch["steps"]), [k]) for k in range(head)]
    cuts = sorted({max(fields_of(st), head) for st in ch["steps"]} | {N})
    lo = head
    for hi in cuts:
        for cls in range(NCLS):
            fields = [k for k in range(lo, hi) if class_of(k) == cls]
            if fields:
                out.append((cls, tuple(fields_of(st) > lo for st in ch["steps"]), fields))
        lo = hi
    return out


def seq_init():
    """the output buffer before the first field of a sequence call"""
    return R.lcg_bytes(OUTH * OUTW * 4, SEQ_INIT_SEED)


def seq_parity(j):
    """(field, frame) of field j of a set (extra/video_convert.c:261-267)"""
    return j & 1, ((j + 1) >> 1) & 1


def seq_sets(st):
    return [(0, SEQ_FIELDS)] if st["call"] == "sequence" else list(zip(SETS_FIRST, SETS_FIRST[1:]))


def _apply(orc, ch, c, cls, st, parity=None):
    """the parameters of call `st` onto television set c of class `cls`; returns the noise of the call"""
    sk, kn, noise = step_params(ch, st)
    hue = sk.get("hue", 0)
    rows = st["rows"]
    if rows is not None:
        row = rows[cls]
        names = ("hue", "saturation") if len(row) == 3 else ("hue", "saturation", "brightness", "contrast", "black_point", "white_point")
        noise = row[0]
        kn = dict(kn, **dict(zip(names, row[1:7])))
        if len(row) == 8:
            hue = row[7]
    for name, v in kn.items():
        c.set(name, v)
    img = images(ch)[class_image(cls)]
    iw, ih = image_size(ch)
    if st["call"] == "sizes":
        iw, ih = SIZES[class_image(cls)]
        img = img[:ih, :iw]
    field, frame, dco = class_parity(cls)
    if parity is not None:
        field, frame = parity
    pad = np.concatenate([img, img[-1:]], axis=0)
    geo = dict(hue=hue, xoffset=sk.get("xoffset", 0), yoffset=sk.get("yoffset", 0))
    if is_nes(ch):
        c.settings(pad, w=iw, h=ih, dot_crawl_offset=dco, border_color=sk.get("border_color", 0), **geo)
        c.sset("field_initialized", 0)                 # (every call of the chain: CRTHIP_F_NES_SETUP)
    else:
        c.settings(pad, format=R.FMT_BGRA, w=iw, h=ih, as_color=1, field=field, frame=frame, **geo)
    return noise


def _pass(lib, c, noise, trace, clean=True):
    if clean:
        c.analog[:] = 0                                # batch semantics: every field-pass starts from a clean analog[]
    c.modulate()
    hs_before = c.get("hsync")
    if trace:
        c.demodulate(noise, trace=True)
        ub = R.reads_past_inp(lib, c.trace, c.get("vsync"), hs_before)
    else:
        c.demodulate(noise)
        ub = None
    return dict(out=np.array(c.out).copy(), hsync=c.get("hsync"), vsync=c.get("vsync"), rn=c.get("rn") & 0xffffffff,
                inp=np.array(c.inp).copy(), ub=ub)


def _step(lib, ch, c, cls, st, trace):
    """one call that treats its fields independently, on television set c"""
    if st["call"] == "stills":                          # the passes of the schedule on the set as it stands
        ub = False
        for field, frame, _aux in STILLS_SCHED:
            res = _pass(lib, c, _apply(lib, ch, c, cls, st, parity=(field, frame)), trace)
            ub = ub or bool(res["ub"])
        return dict(res, ub=ub if trace else None)
    return _pass(lib, c, _apply(lib, ch, c, cls, st), trace)


def run_class(lib, ch, cls, takes_part, upto=None, stale_at=None, trace=False):
    """one television set per context of class `cls` through calls [0, upto] of the chain, on `lib` (R.Oracle or R.RefLib) ->
    [result of call i or None where the unit takes no part].  stale_at = i: call i runs with call i - 1's parameters (the control
    of the CPU tests).  VHS: under srand(the image's seed); one class at a time, never interleaved (libc's one stream)."""
    steps = ch["steps"] if upto is None else ch["steps"][:upto + 1]
    crts = [lib.new_crt(OUTW, OUTH, R.FMT_BGRA) for _ in range(ch["contexts"])]
    if is_vhs(ch):
        lib.srand(VHS_SEEDS[class_image(cls)])
    res = []
    for i, st in enumerate(steps):
        if not takes_part[i]:
            res.append(None)
            continue
        src = ch["steps"][i - 1] if stale_at == i else st
        res.append(_step(lib, ch, crts[st["ctx"]], cls, src, trace))
    return res


def _copy_state(src, dst):
    dst.set("hsync", src.get("hsync"))
    dst.set("vsync", src.get("vsync"))
    rn = src.get("rn") & 0xffffffff
    dst.set("rn", rn - (1 << 32) if rn >> 31 else rn)   # (a 32-bit word: signed or unsigned by the checker's struct)


def _sequence(lib, ch, st, crts, trace):
    """a sequence / sequence_sets call: the reference's serial loop once per set on a television set of its own, which starts from
    seq_init() and from the (hsync, vsync, rn) that the set's first field holds; what it shows and holds after field k goes to
    field k's own set (crts[k]: the call writes pictures and states of all its fields) -> {field: result}"""
    sk, kn, noise = step_params(ch, st)
    out = {}
    for lo, hi in seq_sets(st):
        c = lib.new_crt(OUTW, OUTH, R.FMT_BGRA)
        c.out[:] = seq_init()
        _copy_state(crts[lo], c)
        for k in range(lo, hi):
            _apply(lib, ch, c, class_of(k), st, parity=seq_parity(k - lo))
            out[k] = _pass(lib, c, noise, trace, clean=False)
            crts[k].out[:] = c.out
            _copy_state(c, crts[k])
    return out


def simulate(lib, ch, upto=None, stale_at=None, trace=False):
    """every unit of the chain on `lib` -> [per unit: [result of call i, or None where the unit takes no part]]"""
    us = units(ch)
    if not has_seq(ch):
        return [run_class(lib, ch, cls, part, upto, stale_at, trace) for cls, part, _ in us]
    assert ch["contexts"] == 1 and stale_at is None
    crts = [lib.new_crt(OUTW, OUTH, R.FMT_BGRA) for _ in us]
    res = [[] for _ in us]
    for i, st in enumerate(ch["steps"] if upto is None else ch["steps"][:upto + 1]):
        seq = _sequence(lib, ch, st, crts, trace) if st["call"] in ("sequence", "sequence_sets") else None
        for u, (cls, part, _fields) in enumerate(us):
            if seq is not None:
                res[u].append(seq.get(u))               # (unit k = field k for k < HEAD)
            else:
                res[u].append(_step(lib, ch, crts[u], cls, st, trace) if part[i] else None)
    return res


def next_rand_after(lib, ch, cls, i):
    """VHS: what libc's rand() gives next after calls [0, i] of the class (drawing it moves the stream: a run of its own)"""
    run_class(lib, ch, cls, (True,) * len(ch["steps"]), upto=i)
    return int(C.CDLL(None).rand())


@functools.lru_cache(maxsize=None)
def expected(id):
    """the oracle's results of a chain: [per unit: [per call: dict(out, hsync, vsync, rn, inp, ub) or None]], and for the VHS chain
    {(class, call): next rand()}"""
    ch = get(id)
    orc = R.Oracle(ch["name"])
    exp = simulate(orc, ch, trace=True)
    nxt = {}
    if is_vhs(ch):
        nxt = {(cls, i): next_rand_after(orc, ch, cls, i) for cls in range(NCLS) for i in range(len(ch["steps"]))}
    return exp, nxt


def sizes_layout(ch):
    """the image buffer of a `sizes` call: every field's SIZES corner of its image followed by a readable row, back to back ->
    (bytes, (N, 3) array of (w, h, byte offset))"""
    parts, sizes, off = [], np.zeros((N, 3), dtype=np.int64), 0
    for k in range(N):
        i = class_image(class_of(k))
        w, h = SIZES[i]
        img = images(ch)[i][:h, :w]
        parts.append(np.concatenate([img, img[-1:]], axis=0).reshape(-1))
        sizes[k] = (w, h, off)
        off += parts[-1].size
    return np.concatenate(parts), sizes


def knob_rows(st):
    """the (N, 3) or (N, 8) knob array of a `knobs` call: field k has its class's row"""
    return np.array([st["rows"][class_of(k)] for k in range(N)], dtype=np.int32)

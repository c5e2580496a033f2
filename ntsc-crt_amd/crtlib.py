"""Host-side Python binding of the crthip_* C ABI (include/crt_hip.h).

PyTorch is used for plumbing only: device memory (torch tensors), streams and, in bench.py,
torch.distributed.  All computation happens in the hand-written HIP kernels of
lib/libcrthip.so; there is NO CPU or eager fallback here -- a missing library or a missing
GPU raises immediately.

The surface mirrors the reference's (crt_core.h:100-139): a ``CRT`` object is created with
the output geometry (crt_init), carries the monitor knobs as attributes (struct CRT members,
crt_core.h:77-86), and has ``modulate(settings)`` / ``demodulate(noise)``; the difference is
that it holds a *batch* of independent fields (one struct CRT each in the reference's terms).
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(HERE, "lib")

SYSTEM_NTSC, SYSTEM_NES, SYSTEM_PV1K, SYSTEM_SNES, SYSTEM_TEMP, SYSTEM_VHS, SYSTEM_NESRGB = 0, 1, 2, 3, 4, 5, 6
FMT_RGB, FMT_BGR, FMT_ARGB, FMT_RGBA, FMT_ABGR, FMT_BGRA = range(6)
F_NES_SETUP, F_VHS_DRAW_ABERRATION, F_BLOOM, F_IMAGE_SPARE_ROW = 2, 4, 8, 16
F_NO_HSYNC, F_NO_VSYNC, F_VHS_LCG_NOISE, F_HIPASS, F_VHS_LP, F_VHS_EP, F_NES_BORDER = 0x20, 0x40, 0x80, 0x800, 0x2000, 0x4000, 0x1000
# display modes of crt_main.c's displaycb (crt_main.c:459-463): fade the phosphors / clear the display before every field
F_PHOSPHOR_FADE, F_PHOSPHOR_CLEAR = 0x8000, 0x10000
# sequence_sets on the stock VHS build: one rand() stream per set (vhs_hist[set_first[s]] = set s's generator before its first field)
F_VHS_SET_STREAMS = 0x20000
PHOSPHOR_FLAGS = {"keep": 0, "fade": F_PHOSPHOR_FADE, "clear": F_PHOSPHOR_CLEAR}
K_NAMES = ("template", "active", "noise", "sync", "decode")
MAX_VPER, MAX_CCS, CARRIER_ROWS = 5, 5, 10
STATE_INTS = 36      # sizeof(crthip_state) / 4
LINE_INTS = 8        # sizeof(crthip_line) / 4
# columns of the state tensor
ST_FIELD, ST_FRAME, ST_AUX, ST_HSYNC, ST_VSYNC, ST_RN, ST_CCF, ST_ODD = 0, 1, 2, 3, 4, 5, 6, 31
SHAPE_AUTO, SHAPE_LANE_PER_SCANLINE, SHAPE_SCANLINE_PARALLEL = 0, 1, 2

# name -> (CRT_SYSTEM, CRT_CHROMA_PATTERN); a "bloom" suffix selects the CRT_DO_BLOOM build (crt_core.h:70)
SYSTEMS = {"ntsc": (SYSTEM_NTSC, 1), "vhs": (SYSTEM_VHS, 1), "nes": (SYSTEM_NES, 2), "nesp0": (SYSTEM_NES, 0),
           "ntscp0": (SYSTEM_NTSC, 0), "snes": (SYSTEM_SNES, 1), "pv1k": (SYSTEM_PV1K, 1), "temp": (SYSTEM_TEMP, 1),
           "nesrgb": (SYSTEM_NESRGB, 2)}
DOT_CRAWL_SYSTEMS = (SYSTEM_NES, SYSTEM_NESRGB, SYSTEM_SNES, SYSTEM_PV1K, SYSTEM_TEMP)


# the reference's remaining build-time switches as names: base system + crthip_params.flags
VARIANTS = {"vhslp": ("vhs", F_VHS_LP), "vhsep": ("vhs", F_VHS_EP), "vhslcg": ("vhs", F_VHS_LCG_NOISE),
            "ntscnovsync": ("ntsc", F_NO_VSYNC), "ntscnohsync": ("ntsc", F_NO_HSYNC), "ntschipass": ("ntsc", F_HIPASS),
            "nesborder": ("nes", F_NES_BORDER)}


def split_system(name):
    """'ntscbloom' -> ('ntsc', True); a VARIANTS name -> its base system (variant_flags gives the flags)"""
    if name in VARIANTS:
        return VARIANTS[name][0], False
    if name.endswith("bloom"):
        return name[:-5], True
    return name, False


def variant_flags(name):
    return VARIANTS[name][1] if name in VARIANTS else 0


class Pass(C.Structure):
    """crthip_pass (include/crt_hip.h): the encoder inputs of one pass of a stills schedule."""
    _fields_ = [("field", C.c_int), ("frame", C.c_int), ("aux", C.c_int), ("reserved", C.c_int)]


STILLS_MAX_PASSES = 64


class Knobs(C.Structure):
    """crthip_knobs (include/crt_hip.h): what varies per field in fieldpass_knobs, as the caller thinks of it."""
    _fields_ = [("noise", C.c_int), ("mon_hue", C.c_int), ("saturation", C.c_int), ("reserved", C.c_int)]


class Knobs5(C.Structure):
    """crthip_knobs5 (include/crt_hip.h): the same with the two picture knobs, brightness and contrast."""
    _fields_ = [("noise", C.c_int), ("mon_hue", C.c_int), ("saturation", C.c_int), ("brightness", C.c_int),
                ("contrast", C.c_int), ("reserved", C.c_int * 3)]


class KnobRec(C.Structure):
    """crthip_knob_rec (include/crt_hip.h): what the kernels read per field, 32 bytes.  ``reserved`` = (bright, contrast,
    tier_floor): filled by crthip_knobs_prepare5, zeros from crthip_knobs_prepare."""
    _fields_ = [("noise", C.c_int), ("huesn", C.c_int), ("huecs", C.c_int), ("saturation", C.c_int),
                ("bloom_max_e", C.c_int), ("reserved", C.c_int * 3)]


REC_BRIGHT, REC_CONTRAST, REC_TIER_FLOOR = 5, 6, 7      # columns of the (n, 8) record array


class KnobsEnv(C.Structure):
    """crthip_knobs_env (include/crt_hip.h): the batch-wide bounds of one knobs_prepare call.  ``reserved`` = (pic, tier_floors,
    bright_abs_lo): the picture words of crthip_knobs_prepare5 (zeros from crthip_knobs_prepare), by name below."""
    _fields_ = [("magic", C.c_int), ("n", C.c_int), ("noise_max", C.c_int), ("sat_abs_max", C.c_int),
                ("loskip_wave_max", C.c_int), ("reserved", C.c_int * 3)]

    pic = property(lambda self: self.reserved[0])                        # the records carry picture knobs
    tier_floor_min = property(lambda self: self.reserved[1] & 0xff)      # smallest / largest tier floor of the batch
    tier_floor_max = property(lambda self: (self.reserved[1] >> 8) & 0xff)
    bright_abs_lo = property(lambda self: self.reserved[2])              # largest |bright| among the fields whose floor is below 2


KNOB_REC_INTS = C.sizeof(KnobRec) // 4


class Knobs7(C.Structure):
    """crthip_knobs7 (include/crt_hip.h): the five knobs and the two that reach the encoder, black point and white point."""
    _fields_ = [("noise", C.c_int), ("mon_hue", C.c_int), ("saturation", C.c_int), ("brightness", C.c_int),
                ("contrast", C.c_int), ("black_point", C.c_int), ("white_point", C.c_int), ("reserved", C.c_int)]


class LevelRec(C.Structure):
    """crthip_level_rec (include/crt_hip.h): what the encoder's LV kernels read per field, 16 bytes."""
    _fields_ = [("white", C.c_int), ("ire_base", C.c_int), ("reserved", C.c_int * 2)]


class LevelsEnv(C.Structure):
    """crthip_levels_env (include/crt_hip.h): the batch-wide bounds of the level records of one crthip_knobs_prepare7 call."""
    _fields_ = [("magic", C.c_int), ("n", C.c_int), ("white_abs_max", C.c_int), ("ire_base_abs_max", C.c_int),
                ("reserved", C.c_int * 4)]


class Knobs8(C.Structure):
    """crthip_knobs8 (include/crt_hip.h): crthip_knobs7 with its last word named: the ENCODER hue of the field."""
    _fields_ = [("noise", C.c_int), ("mon_hue", C.c_int), ("saturation", C.c_int), ("brightness", C.c_int),
                ("contrast", C.c_int), ("black_point", C.c_int), ("white_point", C.c_int), ("hue", C.c_int)]


CARRIER_ROWS, MAX_CCS = 10, 5                            # CRTHIP_CARRIER_ROWS, CRTHIP_MAX_CCS


class HueRec(C.Structure):
    """crthip_hue_rec (include/crt_hip.h): the three carrier tables of one field, 640 bytes."""
    _fields_ = [("burst", (C.c_int * MAX_CCS) * CARRIER_ROWS), ("modI", (C.c_int * MAX_CCS) * CARRIER_ROWS),
                ("modQ", (C.c_int * MAX_CCS) * CARRIER_ROWS), ("reserved", C.c_int * 10)]


class HuesEnv(C.Structure):
    """crthip_hues_env (include/crt_hip.h)."""
    _fields_ = [("magic", C.c_int), ("n", C.c_int), ("reserved", C.c_int * 6)]


class Size(C.Structure):
    """crthip_size (include/crt_hip.h): one field's image size and the byte offset of its image from d_images, 16 bytes."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("off_lo", C.c_uint), ("off_hi", C.c_uint)]


class SizeRec(C.Structure):
    """crthip_size_rec (include/crt_hip.h): what the encoder's SZ kernels read per field, 32 bytes."""
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("col_step_lo", C.c_uint), ("col_step_hi", C.c_uint),
                ("off_lo", C.c_uint), ("off_hi", C.c_uint), ("reserved", C.c_int * 2)]


class SizesEnv(C.Structure):
    """crthip_sizes_env (include/crt_hip.h): the bounds of one crthip_sizes_prepare call."""
    _fields_ = [("magic", C.c_int), ("n", C.c_int), ("w_min", C.c_int), ("w_max", C.c_int), ("h_min", C.c_int),
                ("h_max", C.c_int), ("extent_lo", C.c_uint), ("extent_hi", C.c_uint)]

    extent = property(lambda self: (self.extent_hi << 32) | self.extent_lo)     # bytes of the image buffer the call may read


SIZE_REC_INTS = C.sizeof(SizeRec) // 4
SZ_W, SZ_H, SZ_STEP_LO, SZ_STEP_HI, SZ_OFF_LO, SZ_OFF_HI = range(6)            # columns of the (n, 8) size record array
LEVEL_REC_INTS = C.sizeof(LevelRec) // 4
HUE_REC_INTS = C.sizeof(HueRec) // 4
HUE_BURST, HUE_MODI, HUE_MODQ = 0, CARRIER_ROWS * MAX_CCS, 2 * CARRIER_ROWS * MAX_CCS    # first column of each table in the (n, 160) array
LEV_WHITE, LEV_IRE_BASE = 0, 1                           # columns of the (n, 4) level record array


class Params(C.Structure):
    """crthip_params (include/crt_hip.h)."""
    _fields_ = [(n, C.c_int) for n in (
        "system", "chroma_pattern", "w", "h", "format", "raw", "as_color", "hue", "xoffset", "yoffset",
        "outw", "outh", "out_format", "mon_hue", "brightness", "contrast", "saturation",
        "black_point", "white_point", "scanlines", "blend")] + [
        ("v_fac", C.c_uint), ("noise", C.c_int), ("flags", C.c_int),
        ("finalized", C.c_int), ("in_bpp", C.c_int), ("out_bpp", C.c_int),
        ("destw", C.c_int), ("desth", C.c_int), ("xo", C.c_int), ("yo", C.c_int),
        ("burst", (C.c_int * MAX_CCS) * CARRIER_ROWS), ("modI", (C.c_int * MAX_CCS) * CARRIER_ROWS),
        ("modQ", (C.c_int * MAX_CCS) * CARRIER_ROWS),
        ("dem_cs", (C.c_int * MAX_CCS) * 2), ("dem_sn", (C.c_int * MAX_CCS) * 2),
        ("iir_c", C.c_int * 3), ("eq_lf", C.c_int * 3), ("eq_hf", C.c_int * 3),
        ("eq_g", (C.c_int * 3) * 3), ("huesn", C.c_int), ("huecs", C.c_int),
        ("bright", C.c_int), ("white", C.c_int), ("ire_base", C.c_int), ("dx", C.c_int),
        ("ratio", C.c_int), ("eq_kernel", C.c_int), ("bloom", C.c_int), ("bloom_max_e", C.c_int),
        ("col_step_lo", C.c_uint), ("col_step_hi", C.c_uint), ("loskip_wave_max", C.c_int), ("nes_border_color", C.c_int), ("reserved", C.c_int * 2)]


class FStageCascade(C.Structure):
    """crthip_fstage_cascade (include/crt_hip.h)."""
    _fields_ = [(n, C.c_int) for n in ("c", "form", "ce", "a", "n", "drift", "dstage", "mul_bits", "x0_bits", "in0_bits", "out0_bits",
                                       "in_max", "state_max", "lo", "hi")]


class FStages(C.Structure):
    """crthip_fstages (include/crt_hip.h): what crthip_float_stages_query reports."""
    _fields_ = [("ok", C.c_int), ("ranges_ok", C.c_int), ("steps", C.c_int), ("cas", FStageCascade * 4)]


def float_stages(params, steps=0):
    """crthip_float_stages_query (host only): (verdict, FStages) for a finalized Params"""
    out = FStages()
    rc = load_library().crthip_float_stages_query(C.byref(params), int(steps), C.byref(out))
    if rc < 0:
        raise ValueError("crthip_float_stages_query failed (%d)" % rc)
    return rc, out


def bpp4fmt(fmt):
    return 3 if fmt in (0, 1) else (4 if fmt in (2, 3, 4, 5) else 0)


_LIB = None


def load_library():
    """dlopen lib/libcrthip.so (built by ``make -C ntsc-crt_amd`` / __graft_entry__.build())."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # CRTHIP_LIBDIR: another build of the same library (A/B measurements of a kernel change against the previous build)
    path = os.path.join(os.environ.get("CRTHIP_LIBDIR") or LIBDIR, "libcrthip.so")
    if not os.path.exists(path):
        raise RuntimeError("native library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % path)
    L = C.CDLL(path, mode=os.RTLD_GLOBAL)
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    PP = C.POINTER(Params)
    L.crthip_abi_version.restype = ci
    L.crthip_device_count.restype = ci
    L.crthip_params_default.argtypes = [PP, ci, ci]
    L.crthip_params_finalize.argtypes = [PP]
    L.crthip_input_size.argtypes = [ci, ci]
    L.crthip_hres.argtypes = [ci, ci]
    L.crthip_lines.argtypes = [ci]
    L.crthip_field_stride.argtypes = [ci, ci]
    L.crthip_field_stride.restype = sz
    L.crthip_create.argtypes = [C.POINTER(vp), ci, ci, ci]
    L.crthip_destroy.argtypes = [vp]
    L.crthip_destroy.restype = None
    L.crthip_set_stream.argtypes = [vp, vp]
    L.crthip_synchronize.argtypes = [vp]
    L.crthip_error_string.argtypes = [vp]
    L.crthip_error_string.restype = C.c_char_p
    L.crthip_reserve.argtypes = [vp, ci]
    L.crthip_fieldpass.argtypes = [vp, PP, ci, vp, sz, vp, sz, vp]
    L.crthip_modulate.argtypes = [vp, PP, ci, vp, sz, vp, vp]
    L.crthip_noise.argtypes = [vp, PP, ci, vp, vp, vp]
    L.crthip_sync.argtypes = [vp, PP, ci, vp, vp, vp]
    L.crthip_decode.argtypes = [vp, PP, ci, vp, vp, vp, sz]
    L.crthip_profile_enable.argtypes = [vp, ci]
    L.crthip_set_exact.argtypes = [vp, ci]
    L.crthip_vhs_history_from_seed.argtypes = [C.c_uint, C.POINTER(C.c_uint)]
    L.crthip_vhs_bind_history.argtypes = [vp, vp]
    L.crthip_set_overlap.argtypes = [vp, ci]
    L.crthip_set_shape.argtypes = [vp, ci]
    L.crthip_set_signal_tile.argtypes = [vp, ci]
    L.crthip_set_wide_lpw.argtypes = [vp, ci]
    L.crthip_set_signal_layout.argtypes = [vp, ci]
    L.crthip_signal_layout_query.argtypes = [PP, ci, ci, C.POINTER(ci), C.POINTER(sz)]
    if hasattr(L, "crthip_float_stages_query"):          # (an older build under CRTHIP_LIBDIR has neither)
        L.crthip_float_stages_query.argtypes = [PP, ci, C.POINTER(FStages)]
        L.crthip_float_stages_used.argtypes = [vp]
    L.crthip_fieldpass_signal.argtypes = [vp, ci, vp, C.POINTER(ci)]
    L.crthip_table_generation.argtypes = [vp]
    L.crthip_table_generation.restype = C.c_uint
    L.crthip_sequence.argtypes = [vp, PP, ci, vp, sz, vp, sz, vp, vp, C.POINTER(ci)]
    L.crthip_sequence_sets.argtypes = [vp, PP, ci, C.POINTER(ci), vp, sz, vp, sz, vp, sz, vp, C.POINTER(ci)]
    L.crthip_stills_schedule.argtypes = [ci, ci, ci, C.POINTER(Pass), ci]
    L.crthip_stills_reserve.argtypes = [vp, ci, ci]
    L.crthip_stills.argtypes = [vp, PP, ci, vp, sz, vp, sz, vp, ci, C.POINTER(Pass)]
    L.crthip_vhs_chain.argtypes = [vp, ci, vp, ci]
    L.crthip_seq_vhs_prechained.argtypes = [vp, ci]
    L.crthip_seq_encode.argtypes = [vp, PP, ci, ci, ci, vp, sz, vp]
    L.crthip_seq_sync.argtypes = [vp, PP, ci, vp, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.crthip_seq_decode.argtypes = [vp, PP, ci, vp, sz, vp]
    L.crthip_seq_weave.argtypes = [vp, PP, ci, vp, sz, vp, ci]
    L.crthip_set_pixel_tile.argtypes = [vp, ci]
    L.crthip_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(ci)]
    L.crthip_phosphor_table.argtypes = [ci, C.POINTER(C.c_ubyte)]
    if hasattr(L, "crthip_fieldpass_knobs"):                      # (an earlier build loaded through CRTHIP_LIBDIR for an A/B run has none)
        L.crthip_knobs_prepare.argtypes = [PP, ci, C.POINTER(Knobs), C.POINTER(KnobRec), C.POINTER(KnobsEnv)]
    if hasattr(L, "crthip_knobs_prepare5"):                       # (likewise)
        L.crthip_knobs_prepare5.argtypes = [PP, ci, C.POINTER(Knobs5), C.POINTER(KnobRec), C.POINTER(KnobsEnv)]
        L.crthip_fieldpass_knobs.argtypes = [vp, PP, ci, vp, sz, vp, sz, vp, vp, C.POINTER(KnobsEnv)]
    if hasattr(L, "crthip_sequence_knobs"):                       # (likewise)
        L.crthip_sequence_knobs.argtypes = [vp, PP, ci, vp, sz, vp, sz, vp, vp, vp, C.POINTER(KnobsEnv), C.POINTER(ci)]
        L.crthip_sequence_sets_knobs.argtypes = [vp, PP, ci, C.POINTER(ci), vp, sz, vp, sz, vp, sz, vp, vp, C.POINTER(KnobsEnv), C.POINTER(ci)]
        L.crthip_seq_bind_knobs.argtypes = [vp, vp, C.POINTER(KnobsEnv)]
    if hasattr(L, "crthip_knobs_prepare7"):                       # (likewise)
        L.crthip_knobs_prepare7.argtypes = [PP, ci, C.POINTER(Knobs7), C.POINTER(KnobRec), C.POINTER(LevelRec),
                                            C.POINTER(KnobsEnv), C.POINTER(LevelsEnv)]
        L.crthip_bind_levels.argtypes = [vp, vp, C.POINTER(LevelsEnv)]
    if hasattr(L, "crthip_knobs_prepare8"):                       # (likewise)
        L.crthip_knobs_prepare8.argtypes = [PP, ci, C.POINTER(Knobs8), C.POINTER(KnobRec), C.POINTER(LevelRec), C.POINTER(HueRec),
                                            C.POINTER(KnobsEnv), C.POINTER(LevelsEnv), C.POINTER(HuesEnv)]
        L.crthip_bind_hues.argtypes = [vp, vp, C.POINTER(HuesEnv)]
    if hasattr(L, "crthip_stills_knobs"):                         # (likewise)
        L.crthip_stills_knobs.argtypes = [vp, PP, ci, vp, sz, vp, sz, vp, ci, C.POINTER(Pass), vp, C.POINTER(KnobsEnv)]
    if hasattr(L, "crthip_fieldpass_sizes"):                      # (likewise)
        L.crthip_sizes_prepare.argtypes = [PP, ci, C.POINTER(Size), C.POINTER(SizeRec), C.POINTER(SizesEnv)]
        L.crthip_fieldpass_sizes.argtypes = [vp, PP, ci, vp, vp, sz, vp, vp, C.POINTER(SizesEnv)]
        L.crthip_stills_sizes.argtypes = [vp, PP, ci, vp, vp, sz, vp, ci, C.POINTER(Pass), vp, C.POINTER(SizesEnv)]
    if hasattr(L, "crthip_fieldpass_sizes_knobs"):                # (likewise)
        L.crthip_fieldpass_sizes_knobs.argtypes = [vp, PP, ci, vp, vp, sz, vp, vp, C.POINTER(SizesEnv), vp, C.POINTER(KnobsEnv)]
        L.crthip_stills_sizes_knobs.argtypes = [vp, PP, ci, vp, vp, sz, vp, ci, C.POINTER(Pass), vp, C.POINTER(SizesEnv),
                                                vp, C.POINTER(KnobsEnv)]
    _LIB = L
    return L


def make_params(system="ntsc", **kw):
    """crthip_params_default + user fields + crthip_params_finalize (host only, no GPU needed)."""
    L = load_library()
    name_in = system
    system, bloom = split_system(system)
    sysid, pattern = SYSTEMS[system]
    if bloom:
        kw["flags"] = kw.get("flags", 0) | F_BLOOM
    kw["flags"] = kw.get("flags", 0) | variant_flags(name_in)
    p = Params()
    rc = L.crthip_params_default(C.byref(p), sysid, pattern)
    if rc:
        raise ValueError("crthip_params_default failed (%d)" % rc)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    rc = L.crthip_params_finalize(C.byref(p))
    if rc:
        raise ValueError("crthip_params_finalize failed (%d)" % rc)
    return p


def phosphor_table(age):
    """crthip_phosphor_table (host only): [fade^age(c) for c in 0..255] as bytes, crt_main.c:446-450 per colour byte."""
    lut = (C.c_ubyte * 256)()
    rc = load_library().crthip_phosphor_table(int(age), lut)
    if rc:
        raise ValueError("crthip_phosphor_table failed (%d)" % rc)
    return bytes(lut)


def knobs_prepare(params, knobs):
    """crthip_knobs_prepare / crthip_knobs_prepare5 (host only): ``knobs`` = (n, 3) integers, one (noise, mon_hue, saturation) per
    field, or (n, 5): (noise, mon_hue, saturation, brightness, contrast) -- the picture knobs as well --, for the finalized
    ``params`` -> (records as an (n, 8) int32 numpy array in the layout of KnobRec, KnobsEnv).  Every knob entry point of CRT takes
    either width.  (n, 7): (..., black_point, white_point) as well -- crthip_knobs_prepare7; the KnobsEnv then carries the encoder's
    level records and their bounds as ``env.levs`` ((n, 4) int32, the layout of LevelRec) and ``env.lenv`` (knobs_prepare7 returns
    all four), which CRT.upload_knobs uploads and binds."""
    import numpy as np
    if hasattr(knobs, "detach"):
        knobs = knobs.detach().cpu().numpy()
    k = np.asarray(knobs)
    if k.ndim == 2 and k.shape[1] == 7 and k.shape[0] >= 1 and np.issubdtype(k.dtype, np.integer):
        recs, levs, env, lenv = knobs_prepare7(params, k)
        env.levs, env.lenv = levs, lenv
        return recs, env
    if k.ndim != 2 or k.shape[1] not in (3, 5) or k.shape[0] < 1 or not np.issubdtype(k.dtype, np.integer):
        raise ValueError("knobs must be an (n, 3) integer array of (noise, mon_hue, saturation), "
                         "an (n, 5) one of (noise, mon_hue, saturation, brightness, contrast) "
                         "or an (n, 7) one of (noise, mon_hue, saturation, brightness, contrast, black_point, white_point)")
    n, five = int(k.shape[0]), k.shape[1] == 5
    kin = np.zeros((n, 8 if five else 4), dtype=np.int32)
    kin[:, :k.shape[1]] = k
    recs = np.zeros((n, KNOB_REC_INTS), dtype=np.int32)
    env = KnobsEnv()
    if five:
        rc = load_library().crthip_knobs_prepare5(C.byref(params), n, kin.ctypes.data_as(C.POINTER(Knobs5)),
                                                  recs.ctypes.data_as(C.POINTER(KnobRec)), C.byref(env))
    else:
        rc = load_library().crthip_knobs_prepare(C.byref(params), n, kin.ctypes.data_as(C.POINTER(Knobs)),
                                                 recs.ctypes.data_as(C.POINTER(KnobRec)), C.byref(env))
    if rc:
        raise ValueError("crthip_knobs_prepare%s failed (%d)" % ("5" if five else "", rc))
    return recs, env


def knobs_prepare7(params, knobs):
    """crthip_knobs_prepare7 (host only): ``knobs`` = (n, 7) integers, one (noise, mon_hue, saturation, brightness, contrast,
    black_point, white_point) per field -> (knob records (n, 8) int32, level records (n, 4) int32, KnobsEnv, LevelsEnv)."""
    import numpy as np
    if hasattr(knobs, "detach"):
        knobs = knobs.detach().cpu().numpy()
    k = np.asarray(knobs)
    if k.ndim != 2 or k.shape[1] != 7 or k.shape[0] < 1 or not np.issubdtype(k.dtype, np.integer):
        raise ValueError("knobs must be an (n, 7) integer array of (noise, mon_hue, saturation, brightness, contrast, "
                         "black_point, white_point)")
    n = int(k.shape[0])
    kin = np.zeros((n, 8), dtype=np.int32)
    kin[:, :7] = k
    recs = np.zeros((n, KNOB_REC_INTS), dtype=np.int32)
    levs = np.zeros((n, LEVEL_REC_INTS), dtype=np.int32)
    env, lenv = KnobsEnv(), LevelsEnv()
    rc = load_library().crthip_knobs_prepare7(C.byref(params), n, kin.ctypes.data_as(C.POINTER(Knobs7)),
                                              recs.ctypes.data_as(C.POINTER(KnobRec)), levs.ctypes.data_as(C.POINTER(LevelRec)),
                                              C.byref(env), C.byref(lenv))
    if rc:
        raise ValueError("crthip_knobs_prepare7 failed (%d)" % rc)
    return recs, levs, env, lenv


def knobs_prepare8(params, knobs):
    """crthip_knobs_prepare8 (host only): ``knobs`` = (n, 8) integers, one (noise, mon_hue, saturation, brightness, contrast,
    black_point, white_point, hue) per field -- hue = the ENCODER hue -> (knob records (n, 8) int32, level records (n, 4) int32,
    hue records (n, 160) int32 in the layout of HueRec, KnobsEnv, LevelsEnv, HuesEnv).  The KnobsEnv carries ``levs`` / ``lenv`` /
    ``hues`` / ``henv`` as well: CRT.upload_knobs -- the door of every knob entry point of CRT -- takes the (n, 8) array itself."""
    import numpy as np
    if hasattr(knobs, "detach"):
        knobs = knobs.detach().cpu().numpy()
    k = np.asarray(knobs)
    if k.ndim != 2 or k.shape[1] != 8 or k.shape[0] < 1 or not np.issubdtype(k.dtype, np.integer):
        raise ValueError("knobs must be an (n, 8) integer array of (noise, mon_hue, saturation, brightness, contrast, "
                         "black_point, white_point, hue)")
    n = int(k.shape[0])
    kin = np.ascontiguousarray(k, dtype=np.int32)
    recs = np.zeros((n, KNOB_REC_INTS), dtype=np.int32)
    levs = np.zeros((n, LEVEL_REC_INTS), dtype=np.int32)
    hues = np.zeros((n, HUE_REC_INTS), dtype=np.int32)
    env, lenv, henv = KnobsEnv(), LevelsEnv(), HuesEnv()
    rc = load_library().crthip_knobs_prepare8(C.byref(params), n, kin.ctypes.data_as(C.POINTER(Knobs8)),
                                              recs.ctypes.data_as(C.POINTER(KnobRec)), levs.ctypes.data_as(C.POINTER(LevelRec)),
                                              hues.ctypes.data_as(C.POINTER(HueRec)), C.byref(env), C.byref(lenv), C.byref(henv))
    if rc:
        raise ValueError("crthip_knobs_prepare8 failed (%d)" % rc)
    env.levs, env.lenv, env.hues, env.henv = levs, lenv, hues, henv
    return recs, levs, hues, env, lenv, henv


def sizes_prepare(params, sizes):
    """crthip_sizes_prepare (host only): ``sizes`` = (n, 3) integers, one (w, h, byte offset of the image from the buffer's start)
    per field, for the finalized ``params`` (whose own w and h are ignored) -> (records as an (n, 8) uint32 numpy array in the
    layout of SizeRec, SizesEnv)."""
    import numpy as np
    if hasattr(sizes, "detach"):
        sizes = sizes.detach().cpu().numpy()
    k = np.asarray(sizes)
    if k.ndim != 2 or k.shape[1] != 3 or k.shape[0] < 1 or not np.issubdtype(k.dtype, np.integer):
        raise ValueError("sizes must be an (n, 3) integer array of (w, h, byte offset)")
    n = int(k.shape[0])
    if (k[:, 2] < 0).any() or (np.abs(k[:, :2].astype(np.int64)) >= 1 << 31).any():
        raise ValueError("sizes: w and h are 32-bit integers, offsets are not negative")
    sin = (Size * n)()
    for i in range(n):
        off = int(k[i, 2])
        sin[i].w, sin[i].h, sin[i].off_lo, sin[i].off_hi = int(k[i, 0]), int(k[i, 1]), off & 0xffffffff, off >> 32
    recs = np.zeros((n, SIZE_REC_INTS), dtype=np.uint32)
    env = SizesEnv()
    rc = load_library().crthip_sizes_prepare(C.byref(params), n, sin, recs.ctypes.data_as(C.POINTER(SizeRec)), C.byref(env))
    if rc:
        raise ValueError("crthip_sizes_prepare failed (%d)" % rc)
    return recs, env


def _is_knobs8(knobs):
    import numpy as np
    k = knobs.detach().cpu().numpy() if hasattr(knobs, "detach") else np.asarray(knobs)
    return k.ndim == 2 and k.shape[1] == 8 and k.shape[0] >= 1 and np.issubdtype(k.dtype, np.integer)


def stills_schedule(interlaced=True, first_field=0, frames=4):
    """crthip_stills_schedule (host only): the passes of the reference's `ntsc` program (crt_main.c:241-255) as a list of
    (field, frame, aux) -- `frames` passes when progressive, 2 * frames when interlaced; frames = 4 is the CLI."""
    buf = (Pass * STILLS_MAX_PASSES)()
    n = load_library().crthip_stills_schedule(int(bool(interlaced)), int(first_field), int(frames), buf, STILLS_MAX_PASSES)
    if n < 0:
        raise ValueError("crthip_stills_schedule failed (%d)" % n)
    return [(buf[r].field, buf[r].frame, buf[r].aux) for r in range(n)]


class Settings:
    """The reference's ``struct NTSC_SETTINGS`` for a batch: ``data`` is a device tensor holding n
    images ([n, h, w, bpp] uint8, or [n, h, w] int16/uint16 PPU pixels for NES); ``field`` /
    ``frame`` (or ``dot_crawl_offset`` for NES) may be ints or per-image sequences."""

    def __init__(self, data, format=FMT_BGRA, raw=0, as_color=1, field=0, frame=0, hue=0,
                 xoffset=0, yoffset=0, dot_crawl_offset=0, aberration=0, spare_row=None, border_color=0):
        self.data = data
        # CRTHIP_F_IMAGE_SPARE_ROW: every image is followed by one more readable row (the reference reads row h,
        # crt_ntsc.c:263).  None = detect from the tensor: stride(0) and the storage behind the last image cover it.
        self.spare_row = spare_row
        self.format, self.raw, self.as_color = format, raw, as_color
        self.field, self.frame, self.hue = field, frame, hue
        self.xoffset, self.yoffset = xoffset, yoffset
        self.dot_crawl_offset = dot_crawl_offset
        self.aberration = aberration
        self.border_color = border_color  # NES, NES_BORDER builds (crt_nes.h:136)
        self.initialized = 0          # iirs_initialized / field_initialized


class CRT:
    """A batch of n independent CRTs on one GPU (one ``struct CRT`` each in the reference)."""

    def __init__(self, n, outw, outh, out_format=FMT_BGRA, system="ntsc", device=0, out=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the HIP path has no CPU fallback")
        self.torch = torch
        self.L = load_library()
        self.system = system
        self.base_system, self.bloom = split_system(system)
        self.sysid, self.pattern = SYSTEMS[self.base_system]
        self.dev = torch.device("cuda", device)
        self.n = n
        ctx = C.c_void_p()
        rc = self.L.crthip_create(C.byref(ctx), device, self.sysid, self.pattern)
        if rc:
            raise RuntimeError("crthip_create failed (%d): needs a gfx950 device" % rc)
        self.ctx = ctx
        self.input_size = self.L.crthip_input_size(self.sysid, self.pattern)
        self.hres = self.L.crthip_hres(self.sysid, self.pattern)
        self.lines = self.L.crthip_lines(self.sysid)
        self.fstride = self.L.crthip_field_stride(self.sysid, self.pattern)
        # crt_init (crt_core.c:263-289)
        self.outw, self.outh, self.out_format = outw, outh, out_format
        self.hue = self.brightness = self.black_point = 0
        self.saturation, self.contrast, self.white_point = 10, 180, 100
        self.scanlines = self.blend = 0
        self.v_fac = 0
        self.eq_fir = 0        # 0: the 3-band equaliser; 7/6/5/4: FIR kernel of a USE_CONVOLUTION build (crt_core.c:85-147)
        # what happens to the output buffer before every field: "keep" (extra/video_convert.c), "fade" the phosphors or "clear"
        # the display (crt_main.c:459-463).  fieldpass(): one display step per image and call; sequence() / seq_*: one per field
        self.phosphor = "keep"
        bpp = bpp4fmt(out_format) or 4
        self.out = out if out is not None else torch.zeros((n, outh, outw, bpp), dtype=torch.uint8, device=self.dev)
        self.state = torch.zeros((n, STATE_INTS), dtype=torch.int32, device=self.dev)
        self.state[:, ST_RN] = 194
        self._analog = None
        self._inp = None
        self._lines = None
        self._settings = None
        self.knob_recs = None      # device records of fieldpass_knobs ([n, 8] int32, allocated by the first upload_knobs) and their bounds
        self._knob_env = None
        self.level_recs = None     # device level records of an (n, 7) upload_knobs ([n, 4] int32), bound to the context while in use
        self._levels_bound = False
        self.hue_recs = None       # device hue records of an (n, 8) upload_knobs ([n, 160] int32), bound likewise
        self._hues_bound = False
        self.size_recs = None      # device size records of fieldpass_sizes / stills_sizes ([n, 8] int32, allocated by the first upload_sizes)
        self._size_env = None
        self._size_buf = None      # ... and the image buffer they describe
        self.use_stream(None)
        self.vhs_hist = None
        if self.sysid == SYSTEM_VHS:
            # per-field rand() generator state (31-word history), see crthip_vhs_history_from_seed
            self.vhs_hist = torch.zeros((n, 32), dtype=torch.int32, device=self.dev)
            self._check(self.L.crthip_vhs_bind_history(self.ctx, C.c_void_p(self.vhs_hist.data_ptr())), "crthip_vhs_bind_history")
            self.srand([1] * n)

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "ctx", None):
            self.L.crthip_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.L.crthip_error_string(self.ctx).decode()))

    def use_stream(self, stream):
        """Launch on a torch stream (default: torch's current stream on this device)."""
        torch = self.torch
        s = stream if stream is not None else torch.cuda.current_stream(self.dev)
        self._check(self.L.crthip_set_stream(self.ctx, C.c_void_p(s.cuda_stream)), "crthip_set_stream")

    def synchronize(self):
        self._check(self.L.crthip_synchronize(self.ctx), "crthip_synchronize")

    def reserve(self, n=None):
        self._check(self.L.crthip_reserve(self.ctx, n or self.n), "crthip_reserve")

    @property
    def analog(self):
        """Device analog[] of every field, [n, fstride] int8 (first input_size bytes are the field)."""
        if self._analog is None:
            self._analog = self.torch.zeros((self.n, self.fstride), dtype=self.torch.int8, device=self.dev)
        return self._analog

    @property
    def inp(self):
        if self._inp is None:
            self._inp = self.torch.zeros((self.n, self.fstride), dtype=self.torch.int8, device=self.dev)
        return self._inp

    @property
    def line_table(self):
        if self._lines is None:
            self._lines = self.torch.zeros((self.n, self.lines, LINE_INTS), dtype=self.torch.int32, device=self.dev)
        return self._lines

    def params(self, s, noise=0, flags=0):
        """The batch-uniform parameter blob for settings ``s`` and this CRT's knobs (``flags``: further CRTHIP_F_* bits)."""
        d = s.data
        if self.sysid == SYSTEM_NES:
            h, w = int(d.shape[1]), int(d.shape[2])
        else:
            h, w = int(d.shape[1]), int(d.shape[2])
        flags |= self.eq_fir << 8                                  # CRTHIP_F_EQ_FIR(taps)
        if self.phosphor not in PHOSPHOR_FLAGS:
            raise ValueError("CRT.phosphor must be one of %s, not %r" % (sorted(PHOSPHOR_FLAGS), self.phosphor))
        flags |= PHOSPHOR_FLAGS[self.phosphor]
        if getattr(s, "draw_aberration", 0):
            flags |= F_VHS_DRAW_ABERRATION                         # sequence mode
        if self._has_spare_row(s):
            flags |= F_IMAGE_SPARE_ROW
        if self.sysid in (SYSTEM_NES, SYSTEM_NESRGB) and not s.initialized:
            flags |= F_NES_SETUP
        return make_params(self.system, w=w, h=h, format=s.format, raw=s.raw, as_color=s.as_color, hue=s.hue,
                           xoffset=s.xoffset, yoffset=s.yoffset, outw=self.outw, outh=self.outh,
                           out_format=self.out_format, mon_hue=self.hue, brightness=self.brightness,
                           contrast=self.contrast, saturation=self.saturation, black_point=self.black_point,
                           white_point=self.white_point, scanlines=self.scanlines, blend=self.blend,
                           v_fac=self.v_fac, noise=noise, flags=flags, nes_border_color=getattr(s, "border_color", 0))

    def _has_spare_row(self, s):
        if s.spare_row is not None:
            return bool(s.spare_row)
        d = s.data
        row = d.stride(1) * d.element_size()
        need = (int(d.shape[1]) + 1) * row
        if d.shape[0] > 1 and d.stride(0) != 0 and d.stride(0) * d.element_size() < need:
            return False                                           # (stride(0) == 0: ONE image expanded to n, stills_knobs)
        last = (d.storage_offset() + (int(d.shape[0]) - 1) * d.stride(0)) * d.element_size() + need
        return d.untyped_storage().nbytes() >= last

    def _load_field_state(self, s):
        torch = self.torch

        def col(v):
            if isinstance(v, int):
                return torch.full((self.n,), v, dtype=torch.int32, device=self.dev)
            return torch.as_tensor(list(v), dtype=torch.int32, device=self.dev)
        if self.sysid not in (SYSTEM_NES, SYSTEM_NESRGB):
            self.state[:, ST_FIELD] = col(s.field)
            self.state[:, ST_FRAME] = col(s.frame)
        self.state[:, ST_AUX] = col(s.dot_crawl_offset if self.sysid in DOT_CRAWL_SYSTEMS else s.aberration)

    def _image_stride(self, s):
        d = s.data
        assert d[0].is_contiguous() and d.device == self.dev   # images may be padded: only stride(0) is free
        return d.stride(0) * d.element_size()

    # ------------------------------------------------------------------ the hot path
    def modulate(self, s):
        """crt_modulate for every field of the batch (stage-level: analog[] is materialised)."""
        p = self.params(s)
        self._load_field_state(s)
        self._settings = s
        rc = self.L.crthip_modulate(self.ctx, C.byref(p), self.n, C.c_void_p(s.data.data_ptr()),
                                    self._image_stride(s), C.c_void_p(self.analog.data_ptr()),
                                    C.c_void_p(self.state.data_ptr()))
        self._check(rc, "crthip_modulate")
        s.initialized = 1

    def demodulate(self, noise):
        """crt_demodulate for every field (stage-level: noise -> sync -> decode on analog[])."""
        s = self._settings
        p = self.params(s, noise) if s is not None else make_params(
            self.system, w=1, h=1, outw=self.outw, outh=self.outh, out_format=self.out_format,
            mon_hue=self.hue, brightness=self.brightness, contrast=self.contrast, saturation=self.saturation,
            black_point=self.black_point, white_point=self.white_point, scanlines=self.scanlines,
            blend=self.blend, v_fac=self.v_fac, noise=noise, flags=self.eq_fir << 8)
        vp = C.c_void_p
        self._check(self.L.crthip_noise(self.ctx, C.byref(p), self.n, vp(self.analog.data_ptr()),
                                        vp(self.inp.data_ptr()), vp(self.state.data_ptr())), "crthip_noise")
        self._check(self.L.crthip_sync(self.ctx, C.byref(p), self.n, vp(self.inp.data_ptr()),
                                       vp(self.state.data_ptr()), vp(self.line_table.data_ptr())), "crthip_sync")
        self._check(self.L.crthip_decode(self.ctx, C.byref(p), self.n, vp(self.inp.data_ptr()),
                                         vp(self.line_table.data_ptr()), vp(self.out.data_ptr()),
                                         self.out.stride(0)), "crthip_decode")

    def fieldpass(self, s, noise, params=None):
        """modulate + demodulate fused for throughput: the encoder writes the noisy field directly,
        analog[] is never materialised, one launch sequence for the whole batch."""
        p = params if params is not None else self.params(s, noise)
        if params is None:
            self._load_field_state(s)
        rc = self.L.crthip_fieldpass(self.ctx, C.byref(p), self.n, C.c_void_p(s.data.data_ptr()),
                                     self._image_stride(s), C.c_void_p(self.out.data_ptr()),
                                     self.out.stride(0), C.c_void_p(self.state.data_ptr()))
        self._check(rc, "crthip_fieldpass")
        s.initialized = 1

    def upload_knobs(self, knobs, params):
        """knobs_prepare for ``params`` + one copy into this CRT's device record buffer (allocated once, then reused: a captured
        fieldpass_knobs reads what the buffer holds at replay).  Returns the KnobsEnv, which fieldpass_knobs(s, None) reuses.
        An (n, 7) array -- (..., black_point, white_point), which then replace this CRT's own -- also uploads the encoder's level
        records into ``level_recs`` and binds them (crthip_bind_levels) for every knob entry point of this object; a following
        (n, 3) / (n, 5) upload unbinds them.  An (n, 8) array -- (..., hue): the ENCODER hue per field, which then replaces
        ``params.hue`` -- uploads the hue records into ``hue_recs`` as well and binds both (crthip_bind_hues); a following
        (n, 3) / (n, 5) / (n, 7) upload unbinds the hues."""
        torch = self.torch
        if _is_knobs8(knobs):
            recs, env = knobs_prepare8(params, knobs)[::3]
        else:
            recs, env = knobs_prepare(params, knobs)
        if recs.shape[0] != self.n:
            raise ValueError("%d knob triples for a batch of %d fields" % (recs.shape[0], self.n))
        if self.knob_recs is None:
            self.knob_recs = torch.zeros((self.n, KNOB_REC_INTS), dtype=torch.int32, device=self.dev)
        self.knob_recs.copy_(torch.from_numpy(recs))
        self._knob_env = env
        # (n, 7): the encoder's level records into their own device buffer (allocated once, like knob_recs), bound to the context
        # for every knob entry point; a following (n, 3) / (n, 5) upload unbinds them
        levs = getattr(env, "levs", None)
        if levs is not None:
            if self.level_recs is None:
                self.level_recs = torch.zeros((self.n, LEVEL_REC_INTS), dtype=torch.int32, device=self.dev)
            self.level_recs.copy_(torch.from_numpy(levs))
            self._check(self.L.crthip_bind_levels(self.ctx, C.c_void_p(self.level_recs.data_ptr()), C.byref(env.lenv)),
                        "crthip_bind_levels")
            self._levels_bound = True
        elif self._levels_bound:
            self._check(self.L.crthip_bind_levels(self.ctx, None, None), "crthip_bind_levels")
            self._levels_bound = False
        hues = getattr(env, "hues", None)
        if hues is not None:
            if self.hue_recs is None:
                self.hue_recs = torch.zeros((self.n, HUE_REC_INTS), dtype=torch.int32, device=self.dev)
            self.hue_recs.copy_(torch.from_numpy(hues))
            self._check(self.L.crthip_bind_hues(self.ctx, C.c_void_p(self.hue_recs.data_ptr()), C.byref(env.henv)), "crthip_bind_hues")
            self._hues_bound = True
        elif self._hues_bound:
            self._check(self.L.crthip_bind_hues(self.ctx, None, None), "crthip_bind_hues")
            self._hues_bound = False
        return env

    def fieldpass_knobs(self, s, knobs, params=None):
        """fieldpass with per-field (noise, mon_hue, saturation): ``knobs`` = (n, 3) integer array or tensor, or (n, 5) with
        (brightness, contrast) per field as well, which then replace this CRT's own (None: the records
        and bounds of the last upload_knobs -- inside a graph capture, where nothing may be copied from the host).  The batch-
        uniform rest comes from ``params`` (or this CRT's settings); its own noise, mon_hue and saturation are ignored."""
        p = params if params is not None else self.params(s, 0)
        if params is None:
            self._load_field_state(s)
        if knobs is not None:
            self.upload_knobs(knobs, p)
        if self.knob_recs is None:
            raise ValueError("fieldpass_knobs(s, None): no knobs uploaded yet (upload_knobs)")
        rc = self.L.crthip_fieldpass_knobs(self.ctx, C.byref(p), self.n, C.c_void_p(s.data.data_ptr()),
                                           self._image_stride(s), C.c_void_p(self.out.data_ptr()),
                                           self.out.stride(0), C.c_void_p(self.state.data_ptr()),
                                           C.c_void_p(self.knob_recs.data_ptr()), C.byref(self._knob_env))
        self._check(rc, "crthip_fieldpass_knobs")
        s.initialized = 1

    # ------------------------------------------------------------------ mixed image sizes
    def sizes_params(self, s, noise=0, flags=0):
        """The parameter blob of a sizes call for settings ``s`` (format, as_color, hue, offsets; ``s.data`` is not used and may be
        None; ``s.spare_row``: every image is followed by its own spare row): w and h are placeholders, the records carry them."""
        flags |= self.eq_fir << 8
        if self.phosphor not in PHOSPHOR_FLAGS:
            raise ValueError("CRT.phosphor must be one of %s, not %r" % (sorted(PHOSPHOR_FLAGS), self.phosphor))
        flags |= PHOSPHOR_FLAGS[self.phosphor]
        if s.spare_row:
            flags |= F_IMAGE_SPARE_ROW
        if self.sysid in (SYSTEM_NES, SYSTEM_NESRGB) and not s.initialized:
            flags |= F_NES_SETUP
        return make_params(self.system, w=1, h=1, format=s.format, raw=s.raw, as_color=s.as_color, hue=s.hue,
                           xoffset=s.xoffset, yoffset=s.yoffset, outw=self.outw, outh=self.outh,
                           out_format=self.out_format, mon_hue=self.hue, brightness=self.brightness,
                           contrast=self.contrast, saturation=self.saturation, black_point=self.black_point,
                           white_point=self.white_point, scanlines=self.scanlines, blend=self.blend,
                           v_fac=self.v_fac, noise=noise, flags=flags)

    def pack_images(self, images, params):
        """A list of n device tensors of shape (h_k [+ 1], w_k[, bpp]) uint8 -> (one uint8 buffer holding them back to back, at
        offsets rounded up to 4 bytes for the 4-byte formats, an (n, 3) int64 array of (w, h, offset)).  With
        CRTHIP_F_IMAGE_SPARE_ROW in ``params`` every tensor carries its spare row: h_k + 1 rows."""
        import numpy as np
        torch = self.torch
        bpp = params.in_bpp
        spare = 1 if params.flags & F_IMAGE_SPARE_ROW else 0
        sizes = np.zeros((len(images), 3), dtype=np.int64)
        off = 0
        for k, t in enumerate(images):
            if t.dtype != torch.uint8 or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != bpp) or t.shape[0] <= spare:
                raise ValueError("image %d: a uint8 tensor of shape (h%s, w, %d) is needed, not %s %s"
                                 % (k, " + 1" if spare else "", bpp, t.dtype, tuple(t.shape)))
            w = int(t.shape[1]) if t.dim() == 3 else int(t.shape[1]) // bpp
            if bpp == 4:
                off = (off + 3) & ~3
            sizes[k] = (w, int(t.shape[0]) - spare, off)
            off += t.numel()
        buf = torch.empty((max(off, 1),), dtype=torch.uint8, device=self.dev)
        for k, t in enumerate(images):
            buf[int(sizes[k, 2]):int(sizes[k, 2]) + t.numel()] = t.to(self.dev).reshape(-1)
        return buf, sizes

    def upload_sizes(self, images, params):
        """``images`` = a LIST of device tensors (pack_images packs them) or a TUPLE (uint8 device buffer, (n, 3) integer array of
        (w, h, byte offset)): sizes_prepare for ``params`` + one copy into this CRT's device record buffer (allocated once, then
        reused: a captured fieldpass_sizes reads what the buffer holds at replay).  Returns the SizesEnv."""
        torch = self.torch
        if isinstance(images, tuple):                              # (a tuple is always the pair; several images come as a list)
            buf, sizes = images
        else:
            buf, sizes = self.pack_images(list(images), params)
        recs, env = sizes_prepare(params, sizes)
        if recs.shape[0] != self.n:
            raise ValueError("%d sizes for a batch of %d fields" % (recs.shape[0], self.n))
        if buf.dtype != torch.uint8 or not buf.is_contiguous() or buf.device != self.dev or buf.numel() < env.extent:
            raise ValueError("the image buffer must be a contiguous uint8 tensor on %s of at least %d bytes" % (self.dev, env.extent))
        if self.size_recs is None:
            self.size_recs = torch.zeros((self.n, SIZE_REC_INTS), dtype=torch.int32, device=self.dev)
        self.size_recs.copy_(torch.from_numpy(recs.view("int32")))
        self._size_env, self._size_buf = env, buf
        return env

    def fieldpass_sizes(self, images, noise, params=None, settings=None):
        """fieldpass for a batch of MIXED image sizes (crthip_fieldpass_sizes): ``images`` as for upload_sizes (None: the buffer,
        records and bounds of the last upload_sizes -- inside a graph capture, where nothing may be copied from the host).
        ``settings``: a Settings whose format / as_color / hue / offsets / field / frame / spare_row apply (its ``data`` is not
        used; default Settings(None)); ``params``: a blob of sizes_params instead (the field state is then the caller's)."""
        s = settings if settings is not None else Settings(None)
        p = params if params is not None else self.sizes_params(s, noise)
        if params is None:
            self._load_field_state(s)
        if images is not None:
            self.upload_sizes(images, p)
        if self.size_recs is None:
            raise ValueError("fieldpass_sizes(None, ...): no sizes uploaded yet (upload_sizes)")
        rc = self.L.crthip_fieldpass_sizes(self.ctx, C.byref(p), self.n, C.c_void_p(self._size_buf.data_ptr()),
                                           C.c_void_p(self.out.data_ptr()), self.out.stride(0), C.c_void_p(self.state.data_ptr()),
                                           C.c_void_p(self.size_recs.data_ptr()), C.byref(self._size_env))
        self._check(rc, "crthip_fieldpass_sizes")
        s.initialized = 1

    def stills_sizes(self, images, noise, interlaced=True, first_field=0, frames=4, schedule=None, params=None, settings=None):
        """stills for images of MIXED sizes (crthip_stills_sizes): ``images`` / ``settings`` / ``params`` as for fieldpass_sizes,
        the schedule as for stills().  At noise 0 every distinct schedule entry is encoded once."""
        buf = self._stills_passes(interlaced, first_field, frames, schedule)
        s = settings if settings is not None else Settings(None)
        p = params if params is not None else self.sizes_params(s, noise)
        if images is not None:
            self.upload_sizes(images, p)
        if self.size_recs is None:
            raise ValueError("stills_sizes(None, ...): no sizes uploaded yet (upload_sizes)")
        rc = self.L.crthip_stills_sizes(self.ctx, C.byref(p), self.n, C.c_void_p(self._size_buf.data_ptr()),
                                        C.c_void_p(self.out.data_ptr()), self.out.stride(0), C.c_void_p(self.state.data_ptr()),
                                        len(buf), buf, C.c_void_p(self.size_recs.data_ptr()), C.byref(self._size_env))
        self._check(rc, "crthip_stills_sizes")
        s.initialized = 1

    # ------------------------------------------------------------------ mixed image sizes, one look per field
    def _sizes_knobs_upload(self, images, knobs, p, what):
        """the uploads of fieldpass_sizes_knobs / stills_sizes_knobs: the counts are compared with each other and with this CRT's n
        BEFORE anything reaches the library"""
        if not hasattr(self.L, "crthip_fieldpass_sizes_knobs"):
            raise RuntimeError("this libcrthip.so has no crthip_fieldpass_sizes_knobs")
        n_img = None if images is None else int(len(images[1])) if isinstance(images, tuple) else len(images)
        n_knob = None if knobs is None else int(knobs.shape[0]) if hasattr(knobs, "shape") else len(knobs)
        if n_img is not None and n_knob is not None and n_img != n_knob:
            raise ValueError("%s: %d images but %d looks" % (what, n_img, n_knob))
        for cnt, noun in ((n_img, "images"), (n_knob, "looks")):
            if cnt is not None and cnt != self.n:
                raise ValueError("%s: %d %s for a batch of %d fields" % (what, cnt, noun, self.n))
        if images is not None:
            self.upload_sizes(images, p)
        if knobs is not None:
            self.upload_knobs(knobs, p)
        if self.size_recs is None:
            raise ValueError("%s(None, ...): no sizes uploaded yet (upload_sizes)" % what)
        if self.knob_recs is None:
            raise ValueError("%s(..., None): no knobs uploaded yet (upload_knobs)" % what)

    def fieldpass_sizes_knobs(self, images, knobs, params=None, settings=None):
        """fieldpass for a batch of MIXED image sizes in which every field has its own look (crthip_fieldpass_sizes_knobs):
        ``images`` as for fieldpass_sizes -- a list of device tensors, a (buffer, (n, 3)) tuple, or None: the last upload_sizes --,
        ``knobs`` as for fieldpass_knobs -- an (n, 3 | 5 | 7 | 8) integer array or tensor, or None: the last upload_knobs.  Row k of
        both belongs to field k; a length mismatch raises ValueError before anything reaches the library.  ``settings`` /
        ``params`` as for fieldpass_sizes; the blob's own noise, mon_hue, saturation (and what wider rows replace) are ignored."""
        s = settings if settings is not None else Settings(None)
        p = params if params is not None else self.sizes_params(s, 0)
        self._sizes_knobs_upload(images, knobs, p, "fieldpass_sizes_knobs")
        if params is None:
            self._load_field_state(s)
        rc = self.L.crthip_fieldpass_sizes_knobs(self.ctx, C.byref(p), self.n, C.c_void_p(self._size_buf.data_ptr()),
                                                 C.c_void_p(self.out.data_ptr()), self.out.stride(0), C.c_void_p(self.state.data_ptr()),
                                                 C.c_void_p(self.size_recs.data_ptr()), C.byref(self._size_env),
                                                 C.c_void_p(self.knob_recs.data_ptr()), C.byref(self._knob_env))
        self._check(rc, "crthip_fieldpass_sizes_knobs")
        s.initialized = 1

    def stills_sizes_knobs(self, images, knobs, interlaced=True, first_field=0, frames=4, schedule=None, params=None, settings=None):
        """stills for images of MIXED sizes, each with its own look (crthip_stills_sizes_knobs): ``images`` / ``knobs`` /
        ``settings`` / ``params`` as for fieldpass_sizes_knobs, the schedule as for stills().  With every still at noise 0 each
        distinct schedule entry is encoded once, with every still's own size, levels and hue."""
        buf = self._stills_passes(interlaced, first_field, frames, schedule)
        s = settings if settings is not None else Settings(None)
        p = params if params is not None else self.sizes_params(s, 0)
        self._sizes_knobs_upload(images, knobs, p, "stills_sizes_knobs")
        rc = self.L.crthip_stills_sizes_knobs(self.ctx, C.byref(p), self.n, C.c_void_p(self._size_buf.data_ptr()),
                                              C.c_void_p(self.out.data_ptr()), self.out.stride(0), C.c_void_p(self.state.data_ptr()),
                                              len(buf), buf, C.c_void_p(self.size_recs.data_ptr()), C.byref(self._size_env),
                                              C.c_void_p(self.knob_recs.data_ptr()), C.byref(self._knob_env))
        self._check(rc, "crthip_stills_sizes_knobs")
        s.initialized = 1

    def stills_reserve(self, n_distinct):
        """Size the workspace of stills() for schedules of up to n_distinct distinct (field, frame, aux) entries: the call then
        allocates nothing (a timed region, a HIP graph)."""
        self._check(self.L.crthip_stills_reserve(self.ctx, self.n, int(n_distinct)), "crthip_stills_reserve")

    def stills(self, s, noise, interlaced=True, first_field=0, frames=4, schedule=None):
        """Finished stills of the n images of ``s``: the passes of the reference's `ntsc` program (crt_main.c:241-255; set
        ``blend = scanlines = 1`` for its pictures) on ``self.out`` / ``self.state`` as they stand -- a fresh CRT is crt_init:
        zeros, rn 194.  ``schedule``: a list of (field, frame) or (field, frame, aux) per pass instead of the CLI's, e.g. dot-crawl
        offsets r % CRT_CC_VPER in aux for NES / PV-1000, aberration heights for VHS.  At noise 0 every distinct entry is encoded
        once.  ``s.field`` / ``s.frame`` / ``s.dot_crawl_offset`` / ``s.aberration`` are not used: the schedule gives them."""
        buf = self._stills_passes(interlaced, first_field, frames, schedule)
        p = self.params(s, noise)
        rc = self.L.crthip_stills(self.ctx, C.byref(p), self.n, C.c_void_p(s.data.data_ptr()), self._image_stride(s),
                                  C.c_void_p(self.out.data_ptr()), self.out.stride(0), C.c_void_p(self.state.data_ptr()),
                                  len(buf), buf)
        self._check(rc, "crthip_stills")
        s.initialized = 1

    @staticmethod
    def _stills_passes(interlaced, first_field, frames, schedule):
        """the crthip_pass array of stills() / stills_knobs(): the CLI's schedule, or the caller's list"""
        sched = stills_schedule(interlaced, first_field, frames) if schedule is None else [tuple(e) for e in schedule]
        if not 0 < len(sched) <= STILLS_MAX_PASSES:
            raise ValueError("a stills schedule has 1 .. %d passes, not %d" % (STILLS_MAX_PASSES, len(sched)))
        buf = (Pass * len(sched))()
        for r, e in enumerate(sched):
            buf[r].field, buf[r].frame, buf[r].aux = int(e[0]), int(e[1]), int(e[2]) if len(e) > 2 else 0
        return buf

    def stills_knobs(self, s, knobs, interlaced=True, first_field=0, frames=4, schedule=None, params=None):
        """stills with one look per still: ``knobs`` = an (n, 3), (n, 5), (n, 7) or (n, 8) integer array or tensor as for
        fieldpass_knobs, row k = still k's look in every pass (None: the records and bounds of the last upload_knobs -- inside a
        graph capture).  The schedule is that of stills().  With every still at noise 0 each distinct entry is encoded once, with
        every still's own levels and hue.  ``s.data`` may be ONE image expanded to n (``img[None].expand(n, ...)``, stride(0) == 0):
        the contact sheet of an image under n looks, without n copies of it."""
        buf = self._stills_passes(interlaced, first_field, frames, schedule)
        p = params if params is not None else self.params(s, 0)
        if knobs is not None:
            self.upload_knobs(knobs, p)
        if self.knob_recs is None:
            raise ValueError("stills_knobs(s, None): no knobs uploaded yet (upload_knobs)")
        rc = self.L.crthip_stills_knobs(self.ctx, C.byref(p), self.n, C.c_void_p(s.data.data_ptr()), self._image_stride(s),
                                        C.c_void_p(self.out.data_ptr()), self.out.stride(0), C.c_void_p(self.state.data_ptr()),
                                        len(buf), buf, C.c_void_p(self.knob_recs.data_ptr()), C.byref(self._knob_env))
        self._check(rc, "crthip_stills_knobs")
        s.initialized = 1

    def sequence(self, s, noise, out_init=None):
        """The n images of ``s.data`` as n CONSECUTIVE fields of one television set (state and output
        buffer carried over, like extra/video_convert.c), processed in parallel.  ``self.state[0]`` holds
        the set's state before field 0; returns the number of sync fixed-point passes."""
        p = self.params(s, noise)
        self._load_field_state(s)
        passes = C.c_int(0)
        rc = self.L.crthip_sequence(self.ctx, C.byref(p), self.n, C.c_void_p(s.data.data_ptr()), self._image_stride(s),
                                    C.c_void_p(self.out.data_ptr()), self.out.stride(0),
                                    C.c_void_p(out_init.data_ptr()) if out_init is not None else None,
                                    C.c_void_p(self.state.data_ptr()), C.byref(passes))
        self._check(rc, "crthip_sequence")
        s.initialized = 1
        return passes.value

    def sequence_knobs(self, s, knobs, out_init=None, params=None):
        """``sequence`` with per-field (noise, mon_hue, saturation): one running television set whose knobs are turned between
        fields (crt_main.c:351-391).  ``knobs`` = (n, 3) integer array or tensor, or (n, 5): brightness and contrast too (None: the records and bounds of the last
        upload_knobs); the uniform rest comes from ``params`` (or this CRT's settings), whose own noise, mon_hue and saturation
        are ignored.  Returns the number of sync fixed-point passes."""
        p = params if params is not None else self.params(s, 0)
        if params is None:
            self._load_field_state(s)
        if knobs is not None:
            self.upload_knobs(knobs, p)
        if self.knob_recs is None:
            raise ValueError("sequence_knobs(s, None): no knobs uploaded yet (upload_knobs)")
        passes = C.c_int(0)
        rc = self.L.crthip_sequence_knobs(self.ctx, C.byref(p), self.n, C.c_void_p(s.data.data_ptr()), self._image_stride(s),
                                          C.c_void_p(self.out.data_ptr()), self.out.stride(0),
                                          C.c_void_p(out_init.data_ptr()) if out_init is not None else None,
                                          C.c_void_p(self.state.data_ptr()),
                                          C.c_void_p(self.knob_recs.data_ptr()), C.byref(self._knob_env), C.byref(passes))
        self._check(rc, "crthip_sequence_knobs")
        s.initialized = 1
        return passes.value

    def _sets_args(self, set_first, out_init):
        first = [int(v) for v in set_first]
        n_sets = len(first) - 1
        if n_sets < 1 or first[-1] != self.n:
            raise ValueError("set_first must run from 0 to the batch size %d in n_sets + 1 entries" % self.n)
        init_ptr, init_stride = None, 0
        if out_init is not None:
            assert out_init.is_contiguous() and out_init.device == self.dev and out_init.dtype == self.torch.uint8
            if out_init.dim() == 4:
                if int(out_init.shape[0]) != n_sets:
                    raise ValueError("out_init holds %d pictures for %d sets" % (int(out_init.shape[0]), n_sets))
                init_stride = out_init.stride(0)
            init_ptr = C.c_void_p(out_init.data_ptr())
        return first, n_sets, init_ptr, init_stride

    def sequence_sets(self, s, noise, set_first, out_init=None, vhs_streams=False):
        """Many television sets in one call: set i = the consecutive fields [set_first[i], set_first[i + 1]) of the batch
        (``set_first``: n_sets + 1 ints from 0 to n, strictly ascending), each processed as ``sequence`` would process it alone.
        ``self.state[set_first[i]]`` holds set i's hsync / vsync / rn before its first field; ``out_init``: None (zeros), one
        picture [outh, outw, bpp] shared by all sets, or [n_sets, outh, outw, bpp]; returns the passes of the joint sync fixed point.
        ``vhs_streams`` (the stock "vhs" build): every set owns one rand() stream, ``vhs_hist[set_first[i]]`` (``srand``) is set i's
        generator before its first field; ``s.draw_aberration`` then draws every field's aberration height from its set's stream."""
        first, n_sets, init_ptr, init_stride = self._sets_args(set_first, out_init)
        p = self.params(s, noise, F_VHS_SET_STREAMS if vhs_streams else 0)
        self._load_field_state(s)
        passes = C.c_int(0)
        rc = self.L.crthip_sequence_sets(self.ctx, C.byref(p), n_sets, (C.c_int * (n_sets + 1))(*first),
                                         C.c_void_p(s.data.data_ptr()), self._image_stride(s),
                                         C.c_void_p(self.out.data_ptr()), self.out.stride(0), init_ptr, init_stride,
                                         C.c_void_p(self.state.data_ptr()), C.byref(passes))
        self._check(rc, "crthip_sequence_sets")
        s.initialized = 1
        return passes.value

    def sequence_sets_knobs(self, s, knobs, set_first, out_init=None, params=None, vhs_streams=False):
        """``sequence_sets`` with per-field (noise, mon_hue, saturation): ``knobs`` = (n, 3) or (n, 5), row k = field k of the batch whatever
        its set (None: the last upload_knobs); equals ``sequence_knobs`` per set on the set's slice of images, state and knobs.
        ``vhs_streams``: as for ``sequence_sets`` (a given ``params`` must carry F_VHS_SET_STREAMS itself)."""
        first, n_sets, init_ptr, init_stride = self._sets_args(set_first, out_init)
        p = params if params is not None else self.params(s, 0, F_VHS_SET_STREAMS if vhs_streams else 0)
        if params is None:
            self._load_field_state(s)
        if knobs is not None:
            self.upload_knobs(knobs, p)
        if self.knob_recs is None:
            raise ValueError("sequence_sets_knobs(s, None, ...): no knobs uploaded yet (upload_knobs)")
        passes = C.c_int(0)
        rc = self.L.crthip_sequence_sets_knobs(self.ctx, C.byref(p), n_sets, (C.c_int * (n_sets + 1))(*first),
                                               C.c_void_p(s.data.data_ptr()), self._image_stride(s),
                                               C.c_void_p(self.out.data_ptr()), self.out.stride(0), init_ptr, init_stride,
                                               C.c_void_p(self.state.data_ptr()),
                                               C.c_void_p(self.knob_recs.data_ptr()), C.byref(self._knob_env), C.byref(passes))
        self._check(rc, "crthip_sequence_sets_knobs")
        s.initialized = 1
        return passes.value

    def seq_bind_knobs(self, knobs, params=None):
        """Per-field knobs for the phases (seq_encode / seq_sync / seq_decode) of THIS object's n fields: ``knobs`` = (n, 3) or (n, 5), row k =
        field first_index + k of the video; None unbinds.  ``params``: the blob the records are prepared for (default: this CRT's
        monitor settings -- the records and bounds depend on nothing else).  sequence(), fieldpass() etc. ignore the binding."""
        if knobs is None:
            self._check(self.L.crthip_seq_bind_knobs(self.ctx, None, None), "crthip_seq_bind_knobs")
            return
        p = params if params is not None else make_params(
            self.system, w=1, h=1, outw=self.outw, outh=self.outh, out_format=self.out_format,
            mon_hue=self.hue, brightness=self.brightness, contrast=self.contrast, saturation=self.saturation,
            black_point=self.black_point, white_point=self.white_point, scanlines=self.scanlines,
            blend=self.blend, v_fac=self.v_fac, noise=0, flags=self.eq_fir << 8)
        env = self.upload_knobs(knobs, p)
        self._check(self.L.crthip_seq_bind_knobs(self.ctx, C.c_void_p(self.knob_recs.data_ptr()), C.byref(env)), "crthip_seq_bind_knobs")

    # the phases of sequence(), for a video cut over several CRT objects / ranks (shard.sequence_sharded)
    def seq_encode(self, s, noise, first_index, rn0):
        """This object's n fields are fields [first_index, first_index + n) of the video; rn0 = the set's rn before field 0."""
        self._seq_p = self.params(s, noise)
        self._load_field_state(s)
        self._check(self.L.crthip_seq_encode(self.ctx, C.byref(self._seq_p), self.n, int(first_index), int(rn0) if rn0 < 2 ** 31 else int(rn0) - 2 ** 32,
                                             C.c_void_p(s.data.data_ptr()), self._image_stride(s), C.c_void_p(self.state.data_ptr())),
                    "crthip_seq_encode")
        s.initialized = 1

    def seq_sync(self, hsync_in, vsync_in):
        """The sync chain from the incoming pair; returns (hsync, vsync) after this object's last field."""
        ho, vo, ps = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self.L.crthip_seq_sync(self.ctx, C.byref(self._seq_p), self.n, C.c_void_p(self.state.data_ptr()), int(hsync_in), int(vsync_in),
                                           C.byref(ho), C.byref(vo), C.byref(ps)), "crthip_seq_sync")
        return ho.value, vo.value

    def seq_decode(self):
        self._check(self.L.crthip_seq_decode(self.ctx, C.byref(self._seq_p), self.n, C.c_void_p(self.out.data_ptr()), self.out.stride(0),
                                             C.c_void_p(self.state.data_ptr())), "crthip_seq_decode")

    def seq_weave(self, out_init=None, patch_only=False):
        self._check(self.L.crthip_seq_weave(self.ctx, C.byref(self._seq_p), self.n, C.c_void_p(self.out.data_ptr()), self.out.stride(0),
                                            C.c_void_p(out_init.data_ptr()) if out_init is not None else None, int(bool(patch_only))),
                    "crthip_seq_weave")

    def last_picture(self):
        return self.out[self.n - 1]

    # ------------------------------------------------------------------ observation
    def srand(self, seeds):
        """VHS: put field k's rand() generator into the state right after srand(seeds[k])."""
        import numpy as np
        h = np.zeros((self.n, 32), dtype=np.uint32)
        buf = (C.c_uint * 31)()
        for k, sd in enumerate(seeds):
            self._check(self.L.crthip_vhs_history_from_seed(C.c_uint(sd & 0xffffffff), buf), "crthip_vhs_history_from_seed")
            h[k, :31] = np.frombuffer(buf, dtype=np.uint32)
        self.vhs_hist.copy_(self.torch.from_numpy(h.view(np.int32)).to(self.dev))

    def set_exact(self, on=True):
        """1/True: force the exact 32-bit-multiply kernels everywhere; 2: allow the 24-bit tier but not the
        64-bit-mad decoder tiers; 3: 64-bit-mad tier, but never drop the I/Q low cascades; 0: normal dispatch
        by proven operand range."""
        self._check(self.L.crthip_set_exact(self.ctx, int(on)), "crthip_set_exact")

    def set_shape(self, shape):
        """Kernel shape: SHAPE_AUTO (by batch size), SHAPE_LANE_PER_SCANLINE (throughput), SHAPE_SCANLINE_PARALLEL
        (latency; a DPP row of lanes per scanline)."""
        self._check(self.L.crthip_set_shape(self.ctx, int(shape)), "crthip_set_shape")

    def set_overlap(self, chunks):
        """fieldpass(): split the batch into `chunks` pieces alternating between two streams."""
        self._check(self.L.crthip_set_overlap(self.ctx, int(chunks)), "crthip_set_overlap")

    def table_generation(self):
        """rebuilds of the encoder's cached tables so far (a HIP graph captured at generation g replays with g's tables)"""
        return int(self.L.crthip_table_generation(self.ctx))

    def set_signal_tile(self, dwords):
        """fieldpass(): the encoder's signal tile -- 0 by batch size (default), 16 = 64-byte store pieces, 32 / 64 = the large ones"""
        self._check(self.L.crthip_set_signal_tile(self.ctx, int(dwords)), "crthip_set_signal_tile")

    def float_stages_used(self):
        """did the last decoder call launch the float-stage kernels (crthip_float_stages_used)"""
        return int(load_library().crthip_float_stages_used(self.ctx))

    def set_signal_layout(self, padded):
        """fieldpass(): 1 (default) = the signal between encoder and decoder in padded, aligned lines; 0 = the reference's flat layout"""
        self._check(self.L.crthip_set_signal_layout(self.ctx, int(bool(padded))), "crthip_set_signal_layout")

    def fieldpass_signal(self):
        """inp[] of the last fieldpass() in the reference's layout ([n, fstride] int8 like ``inp``) and whether it was kept padded"""
        dst = self.torch.zeros((self.n, self.fstride), dtype=self.torch.int8, device=self.dev)
        padded = C.c_int(0)
        self._check(self.L.crthip_fieldpass_signal(self.ctx, self.n, C.c_void_p(dst.data_ptr()), C.byref(padded)), "crthip_fieldpass_signal")
        return dst, bool(padded.value)

    def set_wide_lpw(self, lpw):
        """the wide-run decoder's scanlines per wavefront: 0 by batch size (default), 8 or 16 = always that instantiation"""
        self._check(self.L.crthip_set_wide_lpw(self.ctx, int(lpw)), "crthip_set_wide_lpw")

    def set_pixel_tile(self, px):
        self._check(self.L.crthip_set_pixel_tile(self.ctx, int(px)), "crthip_set_pixel_tile")

    def profile(self, on=True):
        self._check(self.L.crthip_profile_enable(self.ctx, int(on)), "crthip_profile_enable")

    def profile_read(self):
        ms = (C.c_double * 5)()
        cnt = (C.c_int * 5)()
        self._check(self.L.crthip_profile_read(self.ctx, ms, cnt), "crthip_profile_read")
        return {K_NAMES[k]: (ms[k], cnt[k]) for k in range(5)}

    def get(self, name):
        """hsync / vsync / rn of every field as a list (struct CRT members, crt_core.h:89-91)."""
        col = {"hsync": ST_HSYNC, "vsync": ST_VSYNC, "rn": ST_RN, "odd_field": ST_ODD}[name]
        return self.state[:, col].cpu().tolist()

    @property
    def ccf(self):
        return self.state[:, ST_CCF:ST_CCF + MAX_VPER * MAX_CCS].reshape(self.n, MAX_VPER, MAX_CCS).cpu().numpy()

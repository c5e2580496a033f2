/*
 * crt_hip.h -- C ABI of the MI355X (gfx950) implementation of NTSC-CRT's per-field
 * composite encode -> noisy channel -> decode hot path.
 *
 * Two layers live behind this ABI:
 *
 *  (1) The reference's own entry points (crt_core.h:100-139 of LMP88959/NTSC-CRT):
 *      crt_init / crt_resize / crt_reset / crt_modulate / crt_demodulate /
 *      crt_bpp4fmt / crt_sincos14, with layout-identical `struct CRT` and
 *      `struct NTSC_SETTINGS` (include/crt_core.h and friends).  They are exported
 *      by libntsccrt_hip_<system>.so, one library per CRT_SYSTEM exactly like the
 *      reference is one build per CRT_SYSTEM (crt_core.h:39-59), so the unchanged
 *      crt_main.c / extra/video_convert.c drivers link against it.
 *
 *  (2) The device-resident batch ABI below (crthip_*), exported by libcrthip.so.
 *      It has no counterpart in the reference (which has no batching, SURVEY.md
 *      section 2); layer (1) is a thin C89 client of it.  Plain pointers and sizes
 *      only; device pointers are raw `void *` (e.g. torch.Tensor.data_ptr()).
 *
 * Unit of work: a FIELD-PASS = one crt_modulate (crt_ntsc.c:128 / crt_ntscvhs.c:129 /
 * crt_nes.c:106) followed by one crt_demodulate (crt_core.c:291) on one image.
 * All arithmetic is the reference's 32-bit integer fixed point; results are
 * bit-exact with the CPU path (tests/).
 */
#ifndef CRT_HIP_H
#define CRT_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRTHIP_ABI_VERSION 6

/* CRT_SYSTEM_* of crt_core.h:30-36 */
#define CRTHIP_SYSTEM_NTSC    0
#define CRTHIP_SYSTEM_NES     1
#define CRTHIP_SYSTEM_PV1K    2   /* Casio PV-1000: 5 samples per chroma cycle (crt_pv1k.h, crt_core.c:480-510) */
#define CRTHIP_SYSTEM_SNES    3
#define CRTHIP_SYSTEM_TEMP    4   /* crt_template.c */
#define CRTHIP_SYSTEM_NTSCVHS 5
#define CRTHIP_SYSTEM_NESRGB  6

#define CRTHIP_MAX_VPER  5    /* largest CRT_CC_VPER (PV-1000) */
#define CRTHIP_MAX_CCS   5    /* largest CRT_CC_SAMPLES (PV-1000) */
#define CRTHIP_DCO_MAX   5    /* dot_crawl_offset values 0..5 are tabulated exactly (the headers document 0-5) */
#define CRTHIP_CARRIER_ROWS (CRTHIP_MAX_VPER + CRTHIP_DCO_MAX)   /* rows of the per-line-class carrier tables */

/* CRT_PIX_FORMAT_* of crt_core.h:62-67 */
#define CRTHIP_FMT_RGB  0
#define CRTHIP_FMT_BGR  1
#define CRTHIP_FMT_ARGB 2
#define CRTHIP_FMT_RGBA 3
#define CRTHIP_FMT_ABGR 4
#define CRTHIP_FMT_BGRA 5

/* Bytes of `struct CRT` behind inp[] (outw, outh, out_format, zeroed padding) that the
 * reference's filter window can over-read deterministically when ypos == VRES-1 and
 * hsync >= 5 (crt_core.c:511,539-543).  Mirrored behind every
 * device inp[] so those pixels stay bit-exact.  Deeper over-reads are undefined
 * behaviour in the reference and outside the parity contract. */
#define CRTHIP_TAIL 16

/* error codes (0 = ok).  The reference API is all-void (no error channel,
 * crt_core.h:100-139); layer (1) therefore reports on stderr and aborts. */
#define CRTHIP_OK            0
#define CRTHIP_E_ARG        -1   /* bad argument / unsupported configuration */
#define CRTHIP_E_NODEVICE   -2   /* no HIP device, or device is not gfx950 */
#define CRTHIP_E_HIP        -3   /* HIP runtime error, see crthip_error_string */
#define CRTHIP_E_NOMEM      -4

/* crthip_params.flags */
#define CRTHIP_F_NES_SETUP    2  /* crthip_modulate, NES: NTSC_SETTINGS.field_initialized == 0, i.e. also
                                    write the whole-field sync skeleton (setup_field, crt_nes.c:81-104) */
/* Decoder filter of a USE_CONVOLUTION build of the reference (crt_core.c:85-147): a symmetric FIR kernel of
 * 7 (USE_7_SAMPLE_KERNEL, weights 1 4 7 8 7 4 1), 6, 5 or 4 taps instead of the 3-band IIR equaliser.
 * flags |= CRTHIP_F_EQ_FIR(7); 0 taps (the default) = the equaliser of the reference's stock build. */
#define CRTHIP_F_VHS_DRAW_ABERRATION 4  /* crthip_sequence, VHS: draw every field's aberration height (state.aux)
                                           from the rand() stream like crt_modulate does with do_aberration
                                           (crt_ntscvhs.c:205-207) instead of taking state.aux from the caller */
/* CRT_DO_BLOOM build of the reference (crt_core.h:70; crt_core.c:399-402,512-526; encoder geometry crt_ntsc.c:148-161) */
#define CRTHIP_F_BLOOM        8
/* Every image is followed by one more readable row (image_stride covers h + 1 rows, also behind the last image).
 * The reference clamps the source row with `if (sy >= h) sy = h` (crt_ntsc.c:263, sic) and so reads row h -- one
 * past the image -- for odd fields of raw images with h <= desth.  With this flag the kernels read that row like
 * the reference does; without it they read row h - 1 instead and never touch memory behind an image. */
#define CRTHIP_F_IMAGE_SPARE_ROW 16
/* Further build-time switches of the reference as run-time flags (each is a #define in its sources / headers; 0 = the
 * shipped build).  All of them reproduce the corresponding rebuilt reference bit for bit (tests/, oracle/_ref): */
#define CRTHIP_F_NO_HSYNC     0x20    /* CRT_DO_HSYNC 0 (crt_core.h:72; crt_core.c:446-450): hsync = 0 after every line      */
#define CRTHIP_F_NO_VSYNC     0x40    /* CRT_DO_VSYNC 0 (crt_core.h:71; crt_core.c:323-341): field parity found in the CLEAN
                                         signal, vsync = -3 from then on                                                    */
#define CRTHIP_F_VHS_LCG_NOISE 0x80   /* CRT_VHS_NOISE 0 (crt_ntscvhs.h:29; crt_core.c:343-357): the VHS build with the LCG
                                         noise of every other system, no rand() stream                                      */
#define CRTHIP_F_NES_BORDER   0x1000  /* NES_BORDER 1 (crt_nes.c:69,138-160): crthip_params.nes_border_color right of the picture,
                                         lines CRT_TOP .. CRT_BOT + 2, rewritten by every crt_modulate                      */
#define CRTHIP_F_HIPASS       0x800   /* HIPASS 1 (crt_ntsc.c:115-126 and its siblings): iirf returns s - h ("for debugging") */
#define CRTHIP_F_VHS_LP       0x2000  /* VHS_MODE VHS_LP / VHS_EP (crt_ntscvhs.h:102-124): the encoder's band limits of the  */
#define CRTHIP_F_VHS_EP       0x4000  /*   other two tape speeds                                                            */
#define CRTHIP_F_EQ_FIR(taps)  ((taps) << 8)
#define CRTHIP_F_EQ_FIR_MASK   (7 << 8)
/* Display modes of the reference's real-time driver, whose displaycb (crt_main.c:454-463) treats the output buffer D before
 * every field: fadephos on (the default, crt_main.c:308) fades the phosphors, fadephos off clears the display (:462).  One
 * display step is then  D <- fade(D) (or 0);  crt_modulate;  crt_demodulate onto D  -- with blend the decoder blends against the
 * faded picture.  Neither flag = D carried over unchanged (extra/video_convert.c), the default.
 *   fade(c) = (c>>1) + (c>>2) + (c>>3) + (c>>4) on every colour byte (crt_main.c:446-450 on the little-endian word); the alpha
 *   byte of the 4-byte formats -- the one the decoder writes 0xff into, crt_core.c:620-652: byte 3 of RGBA / BGRA, byte 0 of
 *   ARGB / ABGR -- becomes 0; RGB / BGR fade all three bytes.  fade is monotone, fade(c) < c for c > 0, fade^38(c) = 0 for every
 *   byte (and fade^37(255) != 0); clear = every byte 0 = fade applied 38 times or more (crthip_phosphor_table).
 * crthip_sequence / crthip_seq_weave: image k = D after field k (one display step per field).  crthip_fieldpass: every image of
 * d_out is its own display, one display step per call.  The stage-level entry points (crthip_modulate / _noise / _sync /
 * _decode) refuse both flags: there the host owns the buffer, as crt_main.c does.  crthip_params_finalize refuses both at once. */
#define CRTHIP_F_PHOSPHOR_FADE  0x8000
#define CRTHIP_F_PHOSPHOR_CLEAR 0x10000
/* crthip_sequence_sets / _sets_knobs on the stock VHS build (CRTHIP_SYSTEM_NTSCVHS without CRTHIP_F_VHS_LCG_NOISE): every set owns
 * ONE rand() stream, entry set_first[s] of the bound history array is set s's generator before its first field (see there).
 * Every other entry point ignores the flag; crthip_params_finalize refuses it on another system and with CRTHIP_F_VHS_LCG_NOISE. */
#define CRTHIP_F_VHS_SET_STREAMS 0x20000

/*
 * Everything that is uniform over a batch of field-passes.  Plain old data, no
 * pointers: this is also the blob rank 0 broadcasts over RCCL in the multi-GPU
 * driver.  Fill the USER part, then call crthip_params_finalize(), which derives
 * the rest on the host exactly as the reference does per call (crt_ntsc.c:142-203,
 * crt_core.c:272-280, :305-320, :403-407, :528).
 */
typedef struct crthip_params {
    /* ---- user part ------------------------------------------------------- */
    int system;           /* CRTHIP_SYSTEM_*                                   */
    int chroma_pattern;   /* CRT_CHROMA_PATTERN (crt_ntsc.h:25, crt_nes.h:30)  */
    /* encoder input: struct NTSC_SETTINGS minus data/field/frame
     * (crt_ntsc.h:111-124, crt_ntscvhs.h:133-147, crt_nes.h:132-143) */
    int w, h;             /* image size                                        */
    int format;           /* CRTHIP_FMT_* of the input image (ignored for NES) */
    int raw, as_color;
    int hue;              /* encoder hue                                       */
    int xoffset, yoffset;
    /* decoder: the caller-visible part of struct CRT (crt_core.h:77-86) */
    int outw, outh, out_format;
    int mon_hue, brightness, contrast, saturation;
    int black_point, white_point;
    int scanlines, blend;
    unsigned v_fac;
    int noise;            /* crt_demodulate's `noise` argument                 */
    int flags;            /* CRTHIP_F_*                                        */
    /* ---- derived part (crthip_params_finalize) --------------------------- */
    int finalized;        /* magic, set by crthip_params_finalize              */
    int in_bpp, out_bpp;
    int destw, desth, xo, yo;      /* crt_ntsc.c:132-133,163-173,194-203       */
    /* carrier tables [row][t % CC_SAMPLES] (crt_ntsc.c:174-188, crt_snes.c:171-183, crt_nes.c:123-130).
     * row = (line % CC_VPER) + dot_crawl_offset for the systems whose carriers depend on the line class (NES,
     * NES-RGB, SNES, template, PV-1000; the unreduced sum, so that negative angles truncate exactly like the
     * reference's); NTSC / VHS: row = (field == frame), row 1 carrying the inverted line phase of crt_ntsc.c:199-200 */
    int burst[CRTHIP_CARRIER_ROWS][CRTHIP_MAX_CCS];
    int modI[CRTHIP_CARRIER_ROWS][CRTHIP_MAX_CCS];
    int modQ[CRTHIP_CARRIER_ROWS][CRTHIP_MAX_CCS];
    int dem_cs[2][CRTHIP_MAX_CCS]; /* 5-sample demodulator: cos / sin of hue + i*72 (I) and + 90 (Q), crt_core.c:497-505 */
    int dem_sn[2][CRTHIP_MAX_CCS];
    int iir_c[3];                  /* crt_ntsc.c:98-106, Q11                   */
    int eq_lf[3], eq_hf[3];        /* crt_core.c:171-196, Q16                  */
    int eq_g[3][3];                /* crt_core.c:278-280                       */
    int huesn, huecs;              /* crt_core.c:318-320, 4-bit                */
    int bright;                    /* crt_core.c:305                           */
    int white;                     /* WHITE_LEVEL*white_point/100, crt_ntsc.c:318 */
    int ire_base;                  /* BLACK_LEVEL + black_point, crt_ntsc.c:311 */
    int dx;                        /* crt_core.c:528                           */
    int ratio;                     /* crt_core.c:404-405                       */
    int eq_kernel;                 /* 0 or the FIR taps from flags (validated)   */
    int bloom;                     /* flags & CRTHIP_F_BLOOM                     */
    int bloom_max_e;               /* crt_core.c:400                             */
    /* source column of destination sample x, crt_ntsc.c:272: x * w / destw == (x * col_step) >> 32 with
     * col_step = ceil(2^32 * w / destw), exact while x * destw < 2^32 */
    unsigned col_step_lo, col_step_hi;
    /* Decoder envelope: the largest carrier amplitude |wave| for which the I / Q equalisers' low cascades
     * can be dropped.  crthip_params_finalize sets the bound that holds for ANY inp[] (|s| <= 127: 65 532); the fused entry
     * points (crthip_fieldpass, crthip_sequence), which produce inp[] themselves, raise it from the signal range they know
     * (sync level ... white level + noise term).  A performance hint only: every setting gives identical pictures. */
    int loskip_wave_max;
    int nes_border_color; /* user: NTSC_SETTINGS.border_color (crt_nes.h:136), drawn with CRTHIP_F_NES_BORDER */
    int reserved[2];
} crthip_params;

/*
 * Per-field state, device resident, one entry per field-pass of a batch.  These are
 * the members of struct CRT / NTSC_SETTINGS that vary from field to field and carry
 * over between calls.
 */
typedef struct crthip_state {
    int field, frame;     /* in : NTSC_SETTINGS.field / .frame (NTSC, VHS)     */
    int aux;              /* in : dot_crawl_offset (NES, NES-RGB, SNES, template, PV-1000); VHS aberration lines */
    int hsync, vsync;     /* i/o: crt_core.h:89                                */
    int rn;               /* i/o: crt_core.h:91                                */
    int ccf[CRTHIP_MAX_VPER][CRTHIP_MAX_CCS];   /* i/o: crt_core.h:88 (rows >= CRT_CC_VPER, columns >= CRT_CC_SAMPLES unused) */
    int odd_field;        /* out: field parity found by the vsync search        */
    int reserved[4];
} crthip_state;           /* 144 bytes */

/* What the serial sync chain (crt_core.c:428-479) hands to the filter stage, per
 * decoded line (CRT_TOP..CRT_BOT-1), device resident. */
typedef struct crthip_line {
    int pos;              /* first sample of the active window in inp[] (:454) */
    int wave0, wave1;     /* wave[0], wave[1] (:476-477); [2],[3] = negations.  5-sample systems: dci, dcq (:493-494) */
    int beg;              /* first output row (:428)                            */
    int nrows;            /* rows written: 1 + duplicates (:661-664); 0 = line skipped (:431) */
    int hsync;            /* hsync after this line (diagnostic)                 */
    int dx, scanl;        /* resampler step / start, 12-bit fraction (:528-529; per line with bloom, :519-521) */
} crthip_line;            /* 32 bytes */

typedef struct crthip_ctx crthip_ctx;

/* kernels, for crthip_profile_read() */
#define CRTHIP_K_TEMPLATE 0   /* M4: blanking / sync / burst skeleton           */
#define CRTHIP_K_ACTIVE   1   /* M5: RGB->YIQ, band-limit, quadrature modulate  */
#define CRTHIP_K_NOISE    2   /* D1: channel noise                              */
#define CRTHIP_K_SYNC     3   /* D2-D7: vsync, hsync, burst lock (serial chain) */
#define CRTHIP_K_DECODE   4   /* D8-D10: equalisers, resample, YIQ->RGB, rows   */
#define CRTHIP_K_COUNT    5

int  crthip_abi_version(void);
int  crthip_device_count(void);

/* Host-only helpers (no device needed). */
int  crthip_params_default(crthip_params *p, int system, int chroma_pattern);
int  crthip_params_finalize(crthip_params *p);
int  crthip_input_size(int system, int chroma_pattern);      /* CRT_INPUT_SIZE */
int  crthip_hres(int system, int chroma_pattern);            /* CRT_HRES       */
int  crthip_lines(int system);                               /* CRT_LINES      */
size_t crthip_field_stride(int system, int chroma_pattern);  /* bytes between consecutive
                                   fields in analog[] / inp[] device buffers (>= INPUT_SIZE+CRTHIP_TAIL) */
/* lut[c] = fade^age(c) of a colour byte (CRTHIP_F_PHOSPHOR_FADE, crt_main.c:446-450): lut[c] = c for age 0, all zeros from
 * age 38 on; CRTHIP_E_ARG for age < 0.  The table the sequence weave applies to a row that is `age` fields old. */
int  crthip_phosphor_table(int age, unsigned char lut[256]);

/* VHS only.  The reference's VHS noise is the C library's rand() stream (crt_core.c:344-351); on
 * glibc that is y[n] = y[n-31] + y[n-3], rand() = y[n] >> 1.  The kernels take the generator state
 * of every field as its 31-word history (the values preceding the next output), in/out, device
 * resident, 32 words apart.  crthip_vhs_history_from_seed gives the history right after srand(seed). */
int  crthip_vhs_history_from_seed(unsigned seed, unsigned hist[31]);
int  crthip_vhs_bind_history(crthip_ctx *ctx, unsigned *d_hist);     /* n x 32 words, device, 4-byte aligned (else CRTHIP_E_ARG) */

/* Context = one device + one stream + the jump tables of the noise LCG. */
int  crthip_create(crthip_ctx **out, int device, int system, int chroma_pattern);
void crthip_destroy(crthip_ctx *ctx);
int  crthip_set_stream(crthip_ctx *ctx, void *hip_stream);   /* hipStream_t; NULL = the default stream,
                                                                  which is also the initial setting */
int  crthip_synchronize(crthip_ctx *ctx);
const char *crthip_error_string(const crthip_ctx *ctx);

/* Pre-allocate the per-field workspace (inp[], line table) for up to n fields so that
 * crthip_fieldpass() performs no allocation inside a timed region. */
int  crthip_reserve(crthip_ctx *ctx, int n_fields);

/*
 * BUFFER CONTRACT of every device pointer argument below (DESIGN.md "Buffer contract" has the table and says which entry points
 * tests/test_gpu_fence.py runs on fenced buffers with loose strides and offset bases).  Nothing outside the extents named here is read or
 * written, whatever the base and the stride; an alignment this list forbids is refused with CRTHIP_E_ARG (crthip_error_string
 * says which argument) BEFORE anything is launched, copied or reserved -- every buffer of the call is then untouched.
 *   d_images, image_stride : image k = the w*h*bpp bytes from d_images + k*image_stride (w*h 16-bit PPU pixels for the NES), READ
 *              ONLY; with CRTHIP_F_IMAGE_SPARE_ROW one more row (w*bpp bytes) behind each image is read as well, without it not a
 *              byte.  image_stride >= those bytes, otherwise free (the images need not be packed).  Base AND stride: multiples of
 *              4 for the 4-byte pixel formats (the kernels load whole pixels as dwords), of 2 for PPU pixels, any for RGB / BGR.
 *              crthip_stills_knobs alone also takes image_stride == 0: every still then reads the ONE image at d_images (and its one
 *              spare row with CRTHIP_F_IMAGE_SPARE_ROW).
 *   d_out, out_stride     : picture k = the outw*outh*bpp bytes from d_out + k*out_stride, read (blend, rows the field does not
 *              own, the phosphor flags) and written; out_stride >= those bytes, otherwise free.  Base and stride: multiples of 4
 *              for the 4-byte formats (pixels are stored as dwords and 16-byte runs of dwords), any for RGB / BGR.
 *   d_out_init, out_init_stride : as d_out / out_stride, READ ONLY (out_init_stride 0 = one shared picture).
 *   d_state    : n crthip_state, 144 bytes apart, 4-byte aligned; exactly the n records of the call are read and written.
 *   d_lines    : n * CRT_LINES crthip_line, 32 bytes apart, 4-byte aligned.
 *   d_recs     : n crthip_knob_rec, 32 bytes apart, 4-byte aligned, READ ONLY.
 *   d_levs     : n crthip_level_rec (crthip_bind_levels), 16 bytes apart, 4-byte aligned, READ ONLY; checked when it is bound.
 *   d_hues     : n crthip_hue_rec (crthip_bind_hues), 640 bytes apart, 4-byte aligned, READ ONLY; checked when it is bound.
 *   d_srecs    : n crthip_size_rec (crthip_fieldpass_sizes / crthip_stills_sizes), 32 bytes apart, 4-byte aligned, READ ONLY.  In
 *              those two calls d_images has no stride: image k = the w_k*h_k*bpp bytes from d_images + off_k (one more row with
 *              CRTHIP_F_IMAGE_SPARE_ROW), READ ONLY, everything inside [d_images, d_images + crthip_sizes_env.extent); base and
 *              offsets multiples of 4 for the 4-byte formats.
 *   d_hist     : n x 32 words (crthip_vhs_bind_history), 4-byte aligned; checked when it is bound.
 *   d_analog, d_inp, d_inp_flat : n fields crthip_field_stride() bytes apart, 4-byte aligned; ALL crthip_field_stride() bytes of a
 *              field belong to the library (CRT_INPUT_SIZE samples, the CRTHIP_TAIL mirror, slack the 16-byte pieces of the
 *              signal kernels run into).  crthip_modulate writes only the samples the reference writes; d_analog is READ ONLY for
 *              crthip_noise, d_inp for crthip_sync and crthip_decode.
 * Host pointers (params, env, sched, set_first, passes) follow the C rules for their types.
 */
/*
 * One batch of n independent field-passes, everything device resident:
 *   d_images : n images, image k at d_images + k*image_stride (w*h*bpp bytes, or
 *              w*h u16 PPU pixels for NES)
 *   d_out    : n output images, k at d_out + k*out_stride (outw*outh*bpp bytes);
 *              read as well as written when blend != 0, and rows this field does not
 *              own keep their contents (crt_core.c:431,:608,:662)
 *   d_state  : n crthip_state, updated in place
 * Alignment and extents of all three: BUFFER CONTRACT above (4-byte pixel formats: base and stride multiples of 4; else CRTHIP_E_ARG).
 * Each field starts from a crt_init-clean analog[] (all zero where crt_modulate does
 * not write, crt_ntsc.c:236-238).  Asynchronous on the context's stream: once crthip_reserve
 * has sized the workspace a call allocates nothing and does not synchronise, so the launch
 * sequence can be captured into a HIP graph -- the first call of a context included: the
 * tables the context caches (skeleton fields, the NES sample table) are then built at once
 * on a stream of the library's own, outside the capture, and the graph holds only the
 * per-call kernels.  (A graph reads the tables of the settings it was captured with: do not
 * replay it after calls with other settings went through the same context.)
 */
int  crthip_fieldpass(crthip_ctx *ctx, const crthip_params *p, int n,
                      const void *d_images, size_t image_stride,
                      void *d_out, size_t out_stride,
                      crthip_state *d_state);

/*
 * PER-FIELD KNOBS: a batch whose fields differ in channel noise, monitor hue and saturation -- what the reference's interactive
 * driver changes from one field to the next (crt_main.c:351-391) and crt_demodulate reads afresh in every call
 * (crt_core.c:318-320, 362, 476-477).  The other members of crthip_params stay uniform over the batch.
 *
 * crthip_knobs_prepare (host only): recs[k] = what the kernels read for field k -- huesn / huecs exactly as crthip_params_finalize
 * derives them from mon_hue (crt_core.c:318-320), bloom_max_e for the field's noise (crt_core.c:400) -- and env = the batch-wide
 * bounds the library otherwise takes from the uniform values: the largest |noise| (the encoder's 24-bit envelope), the largest
 * |saturation|, and the decoder's no-low-cascade bound (crthip_params.loskip_wave_max) for the widest signal range any field's
 * noise gives.  p must be finalized; p->noise, p->mon_hue and p->saturation are ignored.  CRTHIP_E_ARG: p not finalized, n <= 0, a
 * NULL pointer, or a field whose knobs crthip_params_finalize would refuse in p (bloom builds: noise < 0 or max_e <= 0).
 *
 * crthip_fieldpass_knobs: bit for bit and state for state what n calls of crthip_fieldpass with n = 1 give, call k on field k's
 * slice of d_images, d_out and d_state with p->noise, p->mon_hue and p->saturation replaced by field k's knobs (a field with noise 0
 * inside a noisy batch advances rn like every other).  d_recs: the n records of crthip_knobs_prepare, uploaded by the caller (DEVICE
 * memory, read when the kernels run: a captured graph reads what the buffer holds at replay -- and keeps the bounds of the env it
 * was captured with, so records written later must stay inside them); env: the same call's bounds, host.
 * Everything crthip_fieldpass accepts is accepted with the same meaning (bloom, FIR, the phosphor flags, both kernel shapes and
 * signal layouts, the overlap chunks, the rand()-noise VHS build), what it refuses is refused, and so are env->magic / env->n that
 * do not match, d_recs off its 4-byte alignment and both phosphor flags at once (CRTHIP_E_ARG; d_out and d_state untouched).  Like crthip_fieldpass after
 * crthip_reserve it allocates nothing, does not synchronise and can be captured; crthip_fieldpass_signal works after it.
 * Records that do not come from the prepare call that made env (larger noise, larger |saturation|) give unspecified pictures -- but
 * no access outside the buffers: the knobs only enter arithmetic, never an address.
 * REFUSED: CRTHIP_SYSTEM_PV1K.  The 5-sample decoder rotates its carriers by the monitor hue and scales them by the saturation in
 * its own prologue, from crthip_params (crt_core.c:497-505: ((dci * cos + dcq * sin) >> 15) * saturation -- the shift in front of
 * the product keeps the sync kernel from folding either in exactly).
 *
 * PICTURE KNOBS: brightness and contrast per field as well -- the other two values the interactive driver turns (the arrow keys,
 * crt_main.c:317-391) and crt_demodulate reads afresh in every call (crt_core.c:305, 573-575).  crthip_knobs_prepare5 takes
 * crthip_knobs5 and fills the last three words of every record: bright = brightness - (BLACK_LEVEL + p->black_point) exactly as
 * crthip_params_finalize derives crthip_params.bright, contrast, and tier_floor = the decoder tier (0, 2 or 3: DESIGN.md 5.3) that
 * pair asks of the field's lines; env->pic = 1, env->tier_floors = the batch's smallest floor | the largest << 8, env->bright_abs_lo
 * = the largest |bright| among the fields whose floor is below 2.  p->brightness, p->contrast and p->bright are then ignored too.
 * It refuses what crthip_knobs_prepare refuses.  All six knob entry points take such records through the arguments they have: the
 * sync kernel ORs every field's floor into the tier flags of that field's lines -- a field at contrast 40 000 takes the 24-bit
 * tier, its neighbours stay where they were; a wavefront whose 64 lines straddle two fields decodes once, at the higher tier --
 * and the decoders read bright and contrast from the record of each line's field (the lane-per-scanline and scanline-parallel
 * shapes per lane, the wide-run decoder per wavefront: its 16 scanlines are always one field's).  Such a call runs the INTEGER
 * filter stages (crthip_float_stages_used says 0): the float stages' binade proof is for one |bright|.
 * Records of crthip_knobs_prepare keep those words and env words 0, and a call with them launches exactly the kernels it
 * launched before there were picture knobs.  An env whose picture words contradict each other (pic neither 0 nor 1, floors
 * outside 0..3 or the smallest above the largest, words set without pic) is refused like a wrong magic.  black_point,
 * white_point and the encoder hue also enter the encoder and stay uniform here (LEVEL KNOBS and HUE KNOB below); CRTHIP_SYSTEM_PV1K stays refused.
 *
 * LEVEL KNOBS: black point and white point per field as well -- the keys q / a and w / s of the interactive driver (crt_main.c's
 * controls) -- the first two knobs that reach the ENCODER's arithmetic: crt_modulate computes
 * ire = (BLACK_LEVEL + black_point) + (((y + i + q) * white) >> 10) with white = WHITE_LEVEL * white_point / 100
 * (crt_ntsc.c:311-318 and its siblings), and the black point enters the decoder once more through bright (crt_core.c:305).
 * crthip_knobs_prepare7 takes crthip_knobs7 and gives TWO record arrays: recs / env exactly what crthip_knobs_prepare5 gives, except
 * that every field's bright and tier_floor (and with them env->tier_floors and env->bright_abs_lo) come from THAT field's black
 * point -- env->pic == 1 --, and levs[k] = { white, ire_base } exactly as crthip_params_finalize derives crthip_params.white and
 * .ire_base, with lenv = their largest magnitudes over the batch.  env->loskip_wave_max is the bound for the widest signal range any
 * field's (white, ire_base, noise) gives.  p->black_point, p->white_point, p->white and p->ire_base are then ignored.  It refuses what
 * crthip_knobs_prepare5 refuses (and a NULL levs / lenv).
 * crthip_bind_levels hands the level records to the context: d_levs = the n records, uploaded by the caller (DEVICE memory, read
 * when the kernels run, as d_recs), lenv copied; (NULL, NULL) unbinds.  The six knob entry points read the binding --
 * crthip_fieldpass_knobs, crthip_sequence_knobs, crthip_sequence_sets_knobs, and crthip_seq_encode / _sync / _decode after
 * crthip_seq_bind_knobs; level record k belongs to the field knob record k belongs to -- and each then requires lenv->n == n and an
 * env with pic == 1.  (crthip_knobs_env.pic cannot say it: pic == 2 is refused by contract.)  The encoder then runs its LV
 * instantiations, which load white and ire_base per lane from the record of the lane's field -- a wavefront's 64 rows may belong to
 * two fields -- and chooses between the 24-bit and the exact kernels by lenv->white_abs_max / ire_base_abs_max (both below 2^13 for
 * the 24-bit ones) in place of p->white / p->ire_base: ONE field over the bound sends the whole call to the exact instantiation,
 * with identical samples.  The uniform entry points and crthip_stills behave exactly as before whether or not something is bound, and
 * so does a knob call while nothing is bound.  Everything crthip_fieldpass_knobs accepts is accepted with the same meaning (both
 * chroma patterns, both VHS noise models, SNES, template, NES-RGB, bloom, FIR, the phosphor flags, blend, both kernel shapes and
 * signal layouts, overlap chunks, graph capture: records rewritten between replays must stay inside the captured lenv; records
 * outside it give unspecified samples but no access outside a buffer -- the levels only enter arithmetic).
 * REFUSED (CRTHIP_E_ARG, crthip_error_string says why, nothing launched, d_out and d_state untouched): a lenv whose magic or n does
 * not match; d_levs off its 4-byte alignment; CRTHIP_SYSTEM_PV1K (as for every knob); CRTHIP_SYSTEM_NES, whose samples come from the
 * 512 x 12 table built for ONE (black, white) pair; CRTHIP_F_NES_BORDER, whose border colour is baked into the cached skeleton with
 * one pair.  crthip_knobs7.reserved is ignored; the encoder hue per field is crthip_knobs8.hue, below.
 *
 * HUE KNOB: the ENCODER hue per field as well -- keys 5 / 6 of the interactive driver, NTSC_SETTINGS.hue, the "color artifacting
 * hue" -- the last of the values the viewer turns between two fields that are numbers.  It rotates the three carrier tables burst,
 * modI and modQ (crt_ntsc.c:174-183 and its siblings), which enter the active-video arithmetic, the burst samples of every video
 * line and the ccf preset.  crthip_knobs_prepare8 takes crthip_knobs8 -- crthip_knobs7 with its last word named hue -- and gives
 * THREE record arrays: recs / levs / env / lenv exactly what crthip_knobs_prepare7 gives for the first seven values (the signal
 * range, and with it env->loskip_wave_max, does not move with the hue: the burst stays inside sync level .. white level), and
 * hues[k] = exactly the three tables crthip_params_finalize derives for a copy of p whose hue is field k's (negative angles
 * truncate as C's do; NES-RGB rotates only its burst; as_color == 0 gives all zeros), henv = { magic, n }.  p->hue and the three
 * tables in p are then ignored.  It refuses what crthip_knobs_prepare7 refuses, a NULL hues / henv, CRTHIP_SYSTEM_NES, and a field
 * whose carriers leave the encoder's 24-bit bound (|modI|, |modQ| < 2048; with sn >> 10 no hue does, and it is checked all the same).
 * crthip_bind_hues hands the records to the context, as crthip_bind_levels does and independently of it: d_hues = the n records in
 * DEVICE memory, read when the kernels run, henv copied; (NULL, NULL) unbinds.  The same six knob entry points read the binding and
 * each then requires henv->n == n; hue record k belongs to the field knob record k belongs to.  With hues bound and levels not,
 * p->white and p->ire_base apply.  The encoder then runs its HU instantiations: the active-video kernels load the carriers of the
 * lane's field per lane; the margin kernels still copy the cached skeleton variants -- which a hue call neither rebuilds nor
 * invalidates: crthip_table_generation does not move -- and recompute the bytes of the burst windows from the field's record before
 * the noise is added; the ccf preset comes from the record.  The uniform entry points and crthip_stills behave exactly as before
 * whether or not something is bound.  Graph capture: records rewritten between replays must come from crthip_knobs_prepare8.
 * REFUSED (CRTHIP_E_ARG, crthip_error_string says why, nothing launched, d_out and d_state untouched): a henv whose magic or n does
 * not match; d_hues off its 4-byte alignment; CRTHIP_SYSTEM_PV1K (as for every knob); CRTHIP_SYSTEM_NES, whose PPU encoder has no
 * per-field instantiation (as for the levels).
 * OUT OF SCOPE: as_color and raw per field (keys SPACE and t), NES and PV-1000, knob videos through shard.py / crt_hip_node.h.
 * (Finished stills with one look per still: crthip_stills_knobs, under STILLS below.  Knob records for a batch of MIXED image sizes:
 * crthip_fieldpass_sizes_knobs / crthip_stills_sizes_knobs, under MIXED IMAGE SIZES below.)
 */
typedef struct crthip_knobs     { int noise, mon_hue, saturation, reserved; } crthip_knobs;                                /* 16 bytes */
typedef struct crthip_knobs5    { int noise, mon_hue, saturation, brightness, contrast, reserved[3]; } crthip_knobs5;      /* 32 bytes */
typedef struct crthip_knob_rec  { int noise, huesn, huecs, saturation, bloom_max_e, bright, contrast, tier_floor; } crthip_knob_rec;   /* 32 bytes */
typedef struct crthip_knobs_env { int magic, n, noise_max, sat_abs_max, loskip_wave_max, pic, tier_floors, bright_abs_lo; } crthip_knobs_env;
int  crthip_knobs_prepare(const crthip_params *p, int n, const crthip_knobs *knobs,
                          crthip_knob_rec *recs /* n, host, out */, crthip_knobs_env *env);
int  crthip_knobs_prepare5(const crthip_params *p, int n, const crthip_knobs5 *knobs,
                           crthip_knob_rec *recs /* n, host, out */, crthip_knobs_env *env);
int  crthip_fieldpass_knobs(crthip_ctx *ctx, const crthip_params *p, int n,
                            const void *d_images, size_t image_stride, void *d_out, size_t out_stride,
                            crthip_state *d_state,
                            const crthip_knob_rec *d_recs /* n, DEVICE */, const crthip_knobs_env *env /* host */);
typedef struct crthip_knobs7    { int noise, mon_hue, saturation, brightness, contrast, black_point, white_point, reserved; } crthip_knobs7;   /* 32 bytes */
typedef struct crthip_level_rec { int white, ire_base, reserved[2]; } crthip_level_rec;                                    /* 16 bytes */
typedef struct crthip_levels_env { int magic, n, white_abs_max, ire_base_abs_max, reserved[4]; } crthip_levels_env;
int  crthip_knobs_prepare7(const crthip_params *p, int n, const crthip_knobs7 *knobs,
                           crthip_knob_rec *recs /* n, host, out */, crthip_level_rec *levs /* n, host, out */,
                           crthip_knobs_env *env, crthip_levels_env *lenv);
int  crthip_bind_levels(crthip_ctx *ctx, const crthip_level_rec *d_levs /* n, DEVICE */, const crthip_levels_env *lenv /* host, copied */);
typedef struct crthip_knobs8    { int noise, mon_hue, saturation, brightness, contrast, black_point, white_point, hue; } crthip_knobs8;   /* 32 bytes */
typedef struct crthip_hue_rec {                                                                                           /* 640 bytes */
    int burst[CRTHIP_CARRIER_ROWS][CRTHIP_MAX_CCS];
    int modI[CRTHIP_CARRIER_ROWS][CRTHIP_MAX_CCS];
    int modQ[CRTHIP_CARRIER_ROWS][CRTHIP_MAX_CCS];
    int reserved[10];
} crthip_hue_rec;
typedef struct crthip_hues_env { int magic, n, reserved[6]; } crthip_hues_env;
int  crthip_knobs_prepare8(const crthip_params *p, int n, const crthip_knobs8 *knobs,
                           crthip_knob_rec *recs /* n, host, out */, crthip_level_rec *levs /* n, host, out */,
                           crthip_hue_rec *hues /* n, host, out */,
                           crthip_knobs_env *env, crthip_levels_env *lenv, crthip_hues_env *henv);
int  crthip_bind_hues(crthip_ctx *ctx, const crthip_hue_rec *d_hues /* n, DEVICE */, const crthip_hues_env *henv /* host, copied */);

/*
 * SEQUENCE mode: n consecutive fields of ONE television set -- what the reference's
 * batch driver does (extra/video_convert.c:246-277:  for every frame: crt_modulate; crt_demodulate;
 * write the output image), with the sync state and the output buffer carried from field to field,
 * yet processed by parallel kernels (DESIGN.md "Sequence mode").
 *   d_state[k].field / .frame / .aux : encoder inputs of field k;  d_state[0].hsync/.vsync/.rn : the
 *   set's state before field 0; on return d_state[k] holds the state after field k.
 *   d_out image k = the (single) output buffer as it stands after field k; d_out_init = its content
 *   before field 0 (NULL = zeros, i.e. calloc as in the drivers).
 * blend != 0 (crt_main.c:235) makes the picture a recurrence over the fields: the fields are then decoded in
 * parallel and folded into each other by one small pass per field (needs outh + v_fac >= CRT_LINES).
 * *passes (optional) receives the number of sync fixed-point passes that were needed.
 * d_images / d_out / d_out_init / d_state: alignment and extents as in the BUFFER CONTRACT (d_out_init is one picture, read only).
 * VHS build: the fields also share ONE rand() stream.  Entry 0 of the bound history array
 * (crthip_vhs_bind_history) is the generator before field 0; a serial pre-pass walks the stream's
 * data-dependent part for all fields (about 0.15 ms per field) and on return entry k is the generator after
 * field k.  With CRTHIP_F_VHS_DRAW_ABERRATION the aberration heights are drawn from the stream as well.
 */
int  crthip_sequence(crthip_ctx *ctx, const crthip_params *p, int n,
                     const void *d_images, size_t image_stride,
                     void *d_out, size_t out_stride, const void *d_out_init,
                     crthip_state *d_state, int *passes);

/*
 * Sequence mode for MANY television sets in one call: n_sets independent sets, set s = the consecutive fields
 * [set_first[s], set_first[s + 1]) of the batch (set_first: a HOST array of n_sets + 1 entries, set_first[0] == 0, strictly
 * ascending -- every set has at least one field; n = set_first[n_sets] fields in all; the sets may differ in length).  Byte for
 * byte and state for state what crthip_sequence gives when called once per set on the set's slice of d_images, d_out and
 * d_state -- with or without blend, with the phosphor flags, every system and kernel shape -- at ONE launch sequence: the number
 * of kernel launches and host synchronisations of a call does not depend on n_sets, and on n only through the sync passes.
 *   d_state[k].field / .frame / .aux : encoder inputs of field k;  d_state[set_first[s]].hsync / .vsync / .rn : set s's state
 *   before its first field, read ON THE DEVICE (no state travels through the host); on return d_state[k] = the state after field k.
 *   d_out_init + s * out_init_stride = set s's output buffer before its first field; out_init_stride == 0: one picture shared
 *   by all sets; d_out_init == NULL: zeros.
 *   *passes (optional) = passes of the joint sync fixed point (one pass covers all sets; at most the longest set's length + 1).
 * The VHS build with rand() noise (CRTHIP_SYSTEM_NTSCVHS without CRTHIP_F_VHS_LCG_NOISE) takes CRTHIP_F_VHS_SET_STREAMS: every set
 * owns one rand() stream.  Entry set_first[s] of the bound history array (crthip_vhs_bind_history, n x 32 words) is set s's
 * generator before its first field, read on the device (the other entries are ignored on input); the sets' chains are walked side
 * by side, one wavefront per set, so the serial pre-pass of crthip_sequence costs the longest set's length, not the batch's.  On
 * return entry k is the generator after field k and d_state[k].rn the last value drawn (the incoming .rn is not used); with
 * CRTHIP_F_VHS_DRAW_ABERRATION every field's aberration height is drawn from its own set's stream and left in d_state[k].aux.
 * Again what crthip_sequence gives per set, on the set's slice of the history array as well.
 * Refused (CRTHIP_E_ARG, crthip_error_string says why): anything else in set_first; what crthip_sequence refuses (the BUFFER
 * CONTRACT's alignments included: out_init_stride counts like out_stride); without
 * CRTHIP_F_VHS_SET_STREAMS the VHS build with rand() noise (every set would own a rand() stream) and CRTHIP_F_VHS_DRAW_ABERRATION,
 * which draws from that stream (give the aberration heights in d_state[k].aux); with it, no history array bound.
 */
int  crthip_sequence_sets(crthip_ctx *ctx, const crthip_params *p,
                          int n_sets, const int *set_first,
                          const void *d_images, size_t image_stride,
                          void *d_out, size_t out_stride,
                          const void *d_out_init, size_t out_init_stride,
                          crthip_state *d_state, int *passes);

/*
 * SEQUENCE mode WITH PER-FIELD KNOBS: one running television set whose channel noise, monitor hue and saturation change from field to
 * field -- the reference's interactive driver with its user at the knobs (crt_main.c:351-391 between two displaycb calls): a tape
 * whose noise rises over a clip, a hue drift, a saturation fade-in, a recorded session of the live viewer.
 * crthip_sequence_knobs: byte for byte and state for state the serial loop on ONE struct CRT -- for field k in order: noise, mon_hue
 * and saturation <- field k's knobs; crt_modulate; crt_demodulate(noise_k); image k = the buffer after field k, d_state[k] = the state
 * after field k -- i.e. what crthip_sequence would give if those three members of crthip_params could change per field.  (A field
 * with noise 0 inside a noisy video runs with gain 0 and advances rn like every other: crt_core.c:358-366.)
 * crthip_sequence_sets_knobs == crthip_sequence_knobs called once per set on the set's slices of d_images, d_out, d_state AND d_recs
 * (record k belongs to field k of the batch; ONE crthip_knobs_prepare over all n = set_first[n_sets] fields gives the env).
 *   d_recs / env : exactly as for crthip_fieldpass_knobs -- crthip_knobs_prepare over the n fields of the call, the records uploaded by
 *   the caller (DEVICE memory; read by the kernels on every pass of the sync fixed point), env on the host.
 * Whatever the uniform entry point accepts is accepted with the same meaning (blend, the phosphor flags, FIR, bloom -- max_e per field --,
 * both kernel shapes, every 4-sample system, the rand()-noise VHS build with CRTHIP_F_VHS_DRAW_ABERRATION in the single-set call,
 * CRTHIP_F_VHS_LCG_NOISE in both); whatever it refuses is refused, and so are -- as in crthip_fieldpass_knobs -- CRTHIP_SYSTEM_PV1K,
 * an env whose magic or n does not match, and both phosphor flags at once (CRTHIP_E_ARG, crthip_error_string says why; d_out and
 * d_state untouched).  The launch sequence is the uniform call's: the number of launches and host synchronisations does not depend
 * on how many distinct knob values there are.  Nothing of the call survives it: the uniform entry points behave as before.
 */
int  crthip_sequence_knobs(crthip_ctx *ctx, const crthip_params *p, int n,
                           const void *d_images, size_t image_stride,
                           void *d_out, size_t out_stride, const void *d_out_init,
                           crthip_state *d_state,
                           const crthip_knob_rec *d_recs /* n, DEVICE */, const crthip_knobs_env *env /* host */, int *passes);
int  crthip_sequence_sets_knobs(crthip_ctx *ctx, const crthip_params *p,
                                int n_sets, const int *set_first,
                                const void *d_images, size_t image_stride,
                                void *d_out, size_t out_stride,
                                const void *d_out_init, size_t out_init_stride,
                                crthip_state *d_state,
                                const crthip_knob_rec *d_recs /* n, DEVICE */, const crthip_knobs_env *env /* host */, int *passes);

/*
 * STILLS: finished still pictures for a batch of n images -- what the reference's main program does for one image
 * (`ntsc -op 640 480 0 0 in.ppm out.ppm`; the accumulate loop of crt_main.c:241-255 with blend = 1, scanlines = 1): several
 * field-passes over the SAME image onto the SAME output buffer, 4 when progressive, 8 when interlaced.
 *
 * crthip_stills_schedule (host only) writes that loop's passes: field = first_field & 1, frame = 0; for e = 0 .. n_frames - 1:
 * emit (field, frame); if interlaced: toggle field, emit again, toggle frame when e is even (the field is not reset between
 * iterations, as in the CLI); aux = 0.  Interlaced from field 0: (0,0)(1,0)(1,1)(0,1)(0,1)(1,1)(1,0)(0,0) -- four distinct entries,
 * each used twice; progressive: one entry n_frames times.  Returns the number of passes written (n_frames, or 2 * n_frames), or
 * CRTHIP_E_ARG (sched == NULL, n_frames <= 0, more passes than `cap` or than CRTHIP_STILLS_MAX_PASSES).
 *
 * crthip_stills: bit for bit and state for state what n_passes calls of crthip_fieldpass give on the same n images, the same d_out
 * and the same d_state, with d_state[k].field / .frame / .aux = sched[r] (field and frame masked with 1, crt_ntsc.c:197-198; aux =
 * dot_crawl_offset or the VHS aberration height, as in crthip_state) set on the device before call r:
 *   d_out image k = still k's display before pass 0 (zeros for the CLI), the finished still on return;
 *   d_state[k]    = hsync / vsync / rn / ccf in; on return the state after the last pass, with the last pass's field / frame / aux
 *                   (rand()-noise VHS build: the bound histories carry every still's generator the same way);
 *   everything crthip_fieldpass accepts is accepted with the same meaning, per pass (every system, bloom, FIR, formats, kernel
 *   shapes, both signal layouts, CRTHIP_F_NES_SETUP, the phosphor flags: one display step per pass); what it refuses is refused,
 *   and so are n_passes <= 0, n_passes > CRTHIP_STILLS_MAX_PASSES and sched == NULL (CRTHIP_E_ARG, crthip_error_string says why).
 *   A refused call leaves d_out and d_state untouched.  Pointers and strides: the BUFFER CONTRACT, as for crthip_fieldpass.
 * What the call adds over the loop:
 *   - noise == 0 (the CLI's test configuration) on the fused LCG-noise path (not the rand()-noise VHS build, not CRTHIP_F_NO_VSYNC,
 *     not an input format crt_modulate refuses): crt_modulate writes the same samples whatever the pass, so the clean signal of
 *     every DISTINCT (field, frame, aux) of the schedule is encoded ONCE for the batch -- 4 encoder runs instead of 8 for the
 *     interlaced CLI schedule, 1 instead of 4 for the progressive one -- into a workspace of n_distinct x n fields (in the layout a
 *     field-pass of n fields would take), which the sync chain and the decoder of every pass read; rn, the ccf preset and the VHS
 *     hsync reset are still applied per pass.  Any other noise encodes per pass, as the loop does.
 *   - one asynchronous call: after crthip_stills_reserve(ctx, n, n_distinct) it allocates nothing and does not synchronise with the
 *     host (the schedule entries travel as kernel arguments), so it can be captured into a HIP graph like crthip_fieldpass.
 *     Without the reserve the workspace grows on demand.
 *   - the shared signal lives in a workspace of its own: nothing of it is seen by a following crthip_fieldpass / crthip_sequence*
 *     on the same context, nor the other way round.  crthip_fieldpass_signal after crthip_stills is refused (the passes of a still
 *     may have read different signals; there is no "the" signal of the call).
 *
 * crthip_stills_knobs: finished stills, EACH WITH ITS OWN LOOK -- an augmentation set, a parameter sweep, a contact sheet of one image
 * under n looks.  Bit for bit and state for state what n_passes calls of crthip_fieldpass_knobs give on the same n images, d_out,
 * d_state and records, d_state[k].field / .frame / .aux set to sched[r] before call r exactly as above; record k is still k's look
 * in EVERY pass.  Per still k that is the reference's loop on one struct CRT whose hue, saturation, brightness, contrast,
 * black_point and white_point are still k's, with NTSC_SETTINGS.hue still k's and crt_demodulate(noise_k) in every pass.
 *   d_recs / env : exactly as for crthip_fieldpass_knobs -- the records of crthip_knobs_prepare / 5 / 7 / 8 over the n stills, uploaded
 *   by the caller; level records (crthip_bind_levels) and hue records (crthip_bind_hues) are read while bound and require lenv->n == n
 *   / henv->n == n.  Nothing of the call survives it; crthip_stills itself behaves as before whether or not something is bound.
 *   Accepted: everything crthip_stills accepts, with the same meaning per pass (every 4-sample system, bloom with max_e per still,
 *   FIR, both kernel shapes and signal layouts, CRTHIP_F_NES_SETUP, the phosphor flags, the rand()-noise VHS build with bound
 *   histories: one generator per still).  Refused (CRTHIP_E_ARG, crthip_error_string says why, nothing launched, d_out and d_state
 *   untouched): what crthip_stills refuses and what crthip_fieldpass_knobs refuses -- CRTHIP_SYSTEM_PV1K, an env whose magic or n
 *   does not match or whose picture words contradict each other, both phosphor flags at once, d_recs off its alignment, and with
 *   levels or hues bound the NES (with levels also CRTHIP_F_NES_BORDER).
 *   The shared clean signal: env->noise_max == 0 (every still at noise 0) under the other conditions of crthip_stills' shared path
 *   -- every distinct (field, frame, aux) is encoded once for the batch, with the records' blob: the LV / HU encoder instantiations
 *   when levels / hues are bound (still k's clean signal depends on ITS levels and hue, not on the pass), into the same workspace
 *   (crthip_stills_reserve).  rn, the ccf preset (from the hue record when hues are bound) and the VHS hsync reset are applied per
 *   pass.  A batch in which ANY still has noise above 0 encodes per pass, as the loop does.
 *   Asynchronous and capturable like crthip_stills after crthip_stills_reserve; records rewritten between replays must stay inside
 *   the captured env / lenv / henv (the rule of crthip_fieldpass_knobs).  crthip_fieldpass_signal after the call is refused.
 *   image_stride == 0 is accepted HERE: every still reads the one image at d_images -- exactly the call with n identical images,
 *   without the n copies (with CRTHIP_F_IMAGE_SPARE_ROW the one spare row behind that image is read).
 */
typedef struct crthip_pass { int field, frame, aux, reserved; } crthip_pass;     /* 16 bytes */
#define CRTHIP_STILLS_MAX_PASSES 64
int  crthip_stills_schedule(int interlaced, int first_field, int n_frames, crthip_pass *sched, int cap);
/* workspace for stills of up to n images whose schedules have up to n_distinct distinct entries (plus crthip_reserve(ctx, n)) */
int  crthip_stills_reserve(crthip_ctx *ctx, int n, int n_distinct);
int  crthip_stills(crthip_ctx *ctx, const crthip_params *p, int n,
                   const void *d_images, size_t image_stride,
                   void *d_out, size_t out_stride, crthip_state *d_state,
                   int n_passes, const crthip_pass *sched /* host */);
int  crthip_stills_knobs(crthip_ctx *ctx, const crthip_params *p, int n,
                         const void *d_images, size_t image_stride,
                         void *d_out, size_t out_stride, crthip_state *d_state,
                         int n_passes, const crthip_pass *sched /* host */,
                         const crthip_knob_rec *d_recs /* n, DEVICE */, const crthip_knobs_env *env /* host */);

/*
 * MIXED IMAGE SIZES in one batch: every field with its own w, h and image -- a folder of photos, an augmentation set, a sprite sheet.
 * With raw == 0 the signal geometry (destw, desth, xo, yo) does not depend on the image size; the size enters crt_modulate on the
 * SOURCE side only: the column x * w / destw (crt_ntsc.c:278), the row y * h / desth + field_offset (:258-261), the clamp
 * `if (sy >= h) sy = h` (:263) and the row pitch sy * w.  Margins, noise, sync chain, decoder, signal layout, skeleton cache and the
 * 24-bit envelope are those of the uniform call.
 *
 * crthip_sizes_prepare (host only): sizes[k] = field k's w, h and the byte offset of its image from d_images (off_lo / off_hi) ->
 * recs[k] = what the kernels read for field k -- col_step exactly as crthip_params_finalize derives col_step_lo / _hi for a copy of p
 * with that w -- and env = the bounds over the batch: the smallest and largest w and h, and extent = the end of the furthest image
 * (offset + w * h * bpp bytes, one more row with CRTHIP_F_IMAGE_SPARE_ROW).  p->w, p->h, p->col_step_* and image_stride are then
 * ignored.  Offsets are free: images packed back to back, padded, in any order, or shared (two fields may name one offset).
 * CRTHIP_E_ARG: p not finalized, n <= 0, a NULL pointer; a size crthip_params_finalize would refuse in that copy of p (w <= 0,
 * h <= 0); an offset that is no multiple of 4 for the 4-byte formats; p->raw != 0 (the signal rectangle then depends on w and h);
 * CRTHIP_SYSTEM_NES (its PPU encoder has no per-field instantiation); an input format crt_modulate refuses (no image is read then);
 * a field whose crthip_signal_layout_query verdict differs from that of p itself (the "geometry does not move" premise, checked).
 *
 * crthip_fieldpass_sizes: bit for bit and state for state what n calls of crthip_fieldpass with n = 1 give, call k made with p->w,
 * p->h and d_images replaced by field k's w, h and d_images + off_k, on field k's slice of d_out and d_state.  d_srecs: the n
 * records of crthip_sizes_prepare, uploaded by the caller (DEVICE memory, read when the kernels run: a captured graph reads what the
 * buffer holds at replay); senv: the same call's bounds, host.  Everything crthip_fieldpass accepts is accepted with the same meaning
 * (every 4-sample system and the PV-1000, both chroma patterns and VHS noise models, bloom, FIR, the phosphor flags, blend, all six
 * input formats, both signal layouts and the signal tiles, overlap chunks, graph capture after crthip_reserve: it allocates nothing
 * and does not synchronise); crthip_fieldpass_signal works after it; what crthip_fieldpass refuses is refused.  Images are READ
 * ONLY: image k = the w_k * h_k * bpp bytes from d_images + off_k, with CRTHIP_F_IMAGE_SPARE_ROW its own row h_k as well (what the
 * reference reads for odd fields with h <= desth), without the flag not a byte behind an image.
 * KERNEL SHAPE: a sizes call always takes the lane-per-scanline encoder (k_active's SZ instantiations), whatever crthip_set_shape
 * says -- crthip_set_shape(ctx, 2) is a no-op for the ENCODER of a sizes call, not an error (the decoder follows it as always); the
 * scanline-parallel encoder has no per-field-size instantiation.  Every field gets whole wavefronts: ceil(desth / 64) workgroups,
 * the lanes beyond desth idle, so that w, h, col_step and the image base are wave-uniform and the cooperative tile path stays in use.
 * TEMPLATE CHOICES that the uniform call takes from p->w come from the env's bounds, ONE launch per call: 4-byte pixels go through
 * the cooperative LDS tiles iff senv->w_min >= 4 (else every lane reads its pixels bytewise), the wide image tile iff senv->w_min
 * >= 1280 (every image then fills whole 128-byte lines).  Every choice gives identical bytes.
 * ADDRESS SAFETY: unlike the knobs the size enters ADDRESSES.  The host checks what it can see -- the env; the records are device
 * memory and may be rewritten between graph replays.  So every wavefront checks its field's record against the captured extent
 * before it reads a pixel: w >= 1 (>= 4 on the tile path), h >= 1, off aligned for the format, off + (h [+ 1]) * w * bpp <= extent;
 * a record that fails is replaced by the smallest image at offset 0 (unspecified samples, no access outside
 * [d_images, d_images + extent)).  Rows are clamped to [0, h] and every source column to [0, w) of the record -- on BOTH sides, by one
 * unsigned compare: col_step is not checked, a rewritten one may give any column, negative ones included, and none leaves the row.  Records rewritten between replays must stay inside the captured env to give the contract's pictures.
 * REFUSED before anything is launched (CRTHIP_E_ARG, crthip_error_string says which; d_out and d_state untouched): an env whose
 * magic or n does not match or whose bounds contradict each other, d_srecs off its 4-byte alignment, d_images off its 4-byte
 * alignment for the 4-byte formats, p->raw != 0, CRTHIP_SYSTEM_NES, an input format crt_modulate refuses.
 *
 * crthip_stills_sizes: crthip_stills for stills of mixed sizes -- bit for bit and state for state what n_passes calls of
 * crthip_fieldpass_sizes give on the same images, d_out, d_state and records, d_state[k].field / .frame / .aux set to sched[r] before
 * call r.  It shares its body with crthip_stills: at noise 0 every distinct schedule entry is encoded once (still k's clean signal
 * depends on ITS size, not on the pass), into the same workspace (crthip_stills_reserve).  Accepted and refused: what crthip_stills
 * and crthip_fieldpass_sizes accept and refuse.  crthip_fieldpass_signal after the call is refused, as after crthip_stills.
 * Nothing of either call survives it: every other entry point launches exactly the kernels it launched before.
 *
 * SIZES WITH KNOB RECORDS -- a folder of photos of mixed sizes in which every photo gets its own look, a contact sheet of one picture
 * per file under per-file settings.
 * crthip_fieldpass_sizes_knobs: bit for bit and state for state what n calls of crthip_fieldpass with n = 1 give, call k made with
 * field k's w, h and image (as crthip_fieldpass_sizes) AND field k's noise, monitor hue, saturation, brightness, contrast, black point,
 * white point and encoder hue (as crthip_fieldpass_knobs).  d_srecs / senv: exactly as for crthip_fieldpass_sizes; d_recs / env: exactly
 * as for crthip_fieldpass_knobs -- the records of crthip_sizes_prepare and of crthip_knobs_prepare / 5 / 7 / 8 as they are, no further
 * prepare function; level records (crthip_bind_levels) and hue records (crthip_bind_hues) are read while bound and require lenv->n ==
 * n / henv->n == n.  Record k of each array belongs to field k.
 * crthip_stills_sizes_knobs: what n_passes calls of crthip_fieldpass_sizes_knobs give, d_state[k].field / .frame / .aux set to
 * sched[r] before call r.  It shares its body with crthip_stills; the clean signal is shared when env->noise_max == 0, encoded once
 * per distinct entry with every still's own size, levels and hue.  crthip_fieldpass_signal after it is refused.
 *   Accepted: what BOTH parents accept -- every 4-sample RGB-input system, both VHS noise models, bloom, FIR, the phosphor flags,
 *   blend, all six input formats, both signal layouts, overlap chunks, graph capture after crthip_reserve / crthip_stills_reserve
 *   (records rewritten between replays stay inside the captured senv / env / lenv / henv).
 *   Refused before anything is launched (CRTHIP_E_ARG, crthip_error_string says why; d_out and d_state untouched): what EITHER parent
 *   refuses -- CRTHIP_SYSTEM_NES, CRTHIP_SYSTEM_PV1K, p->raw != 0, an input format crt_modulate refuses, a senv / env / lenv / henv
 *   whose magic or n does not match or whose words contradict each other, records off their 4-byte alignment, d_images off its
 *   alignment for the 4-byte formats, both phosphor flags at once, with levels bound CRTHIP_F_NES_BORDER.
 *   Encoder: lane-per-scanline as for every sizes call -- k_active's SZ instantiations with KN (env->noise_max != 0), LV (levels
 *   bound) and HU (hues bound).  In a sizes grid the field is wave-uniform: the noise gain, white, ire_base and the base of the hue
 *   record are scalar loads there, where crthip_fieldpass_knobs loads them per lane.  These instantiations exist for the 64-byte
 *   signal pieces (bytewise, narrow and wide image tile); the large signal tiles are not taken by such a call.  Identical bytes.
 *   ADDRESS SAFETY is that of crthip_fieldpass_sizes, unchanged: the size is still the only thing that enters an address.
 * Nothing of either call survives it (the context's knob, size, level and hue call marks are cleared on every way out).
 * OUT OF SCOPE: NES, raw images, sequence mode, shard.py / crt_hip_node.h (a video has one size).
 */
typedef struct crthip_size      { int w, h; unsigned off_lo, off_hi; } crthip_size;                                          /* 16 bytes */
typedef struct crthip_size_rec  { int w, h; unsigned col_step_lo, col_step_hi, off_lo, off_hi; int reserved[2]; } crthip_size_rec;   /* 32 bytes */
typedef struct crthip_sizes_env { int magic, n, w_min, w_max, h_min, h_max; unsigned extent_lo, extent_hi; } crthip_sizes_env;
int  crthip_sizes_prepare(const crthip_params *p, int n, const crthip_size *sizes,
                          crthip_size_rec *recs /* n, host, out */, crthip_sizes_env *env);
int  crthip_fieldpass_sizes(crthip_ctx *ctx, const crthip_params *p, int n, const void *d_images,
                            void *d_out, size_t out_stride, crthip_state *d_state,
                            const crthip_size_rec *d_srecs /* n, DEVICE */, const crthip_sizes_env *senv /* host */);
int  crthip_stills_sizes(crthip_ctx *ctx, const crthip_params *p, int n, const void *d_images,
                         void *d_out, size_t out_stride, crthip_state *d_state,
                         int n_passes, const crthip_pass *sched /* host */,
                         const crthip_size_rec *d_srecs /* n, DEVICE */, const crthip_sizes_env *senv /* host */);
int  crthip_fieldpass_sizes_knobs(crthip_ctx *ctx, const crthip_params *p, int n, const void *d_images,
                                  void *d_out, size_t out_stride, crthip_state *d_state,
                                  const crthip_size_rec *d_srecs /* n, DEVICE */, const crthip_sizes_env *senv /* host */,
                                  const crthip_knob_rec *d_recs /* n, DEVICE */, const crthip_knobs_env *env /* host */);
int  crthip_stills_sizes_knobs(crthip_ctx *ctx, const crthip_params *p, int n, const void *d_images,
                               void *d_out, size_t out_stride, crthip_state *d_state,
                               int n_passes, const crthip_pass *sched /* host */,
                               const crthip_size_rec *d_srecs /* n, DEVICE */, const crthip_sizes_env *senv /* host */,
                               const crthip_knob_rec *d_recs /* n, DEVICE */, const crthip_knobs_env *env /* host */);

/*
 * The phases of crthip_sequence, for hosts that cut ONE video over several contexts / devices / processes
 * (include/crt_hip_node.h; ntsc-crt_amd/shard.py over torch.distributed).  A shard holds the n consecutive fields
 * [first_index, first_index + n) of the video; crthip_sequence == encode(0, rn0) + sync + decode + weave on one context.
 *   encode : state[k].rn = the set's generator before field first_index + k (closed form from rn0, the generator before
 *            field 0 of the VIDEO); all fields encoded, noise fused.  VHS: first_index must be 0 (one rand() stream).
 *   sync   : the sync chain from the incoming (hsync_in, vsync_in) = the set's state before the shard's first field;
 *            returns the pair after its last field.  May be called again with another incoming pair (the predecessor
 *            shard's final state became known): it then restarts from its previous finals.
 *   decode : rn after each field, every field decoded (without blend).
 *   weave  : image k = the output buffer after field k, given d_out_init = the buffer before the shard's first field
 *            (NULL = zeros).  patch_only != 0 (blend == 0 only): the images were woven before with a placeholder init;
 *            only the rows no field of the shard wrote are taken from d_out_init now.
 *
 * VHS build: a video's fields share ONE rand() stream, so a shard cannot start in the middle of it -- unless the stream was
 * walked ahead for the whole video first: crthip_vhs_chain does that for n consecutive fields on ONE context (entry 0 of its
 * bound history array = the generator before field 0; on return entry k = the generator at the start of field k, and with
 * draw_aberration state[k].aux = the aberration height crt_modulate draws, crt_ntscvhs.c:205-207).  A context whose bound
 * histories (and aux) were filled from that array is told so with crthip_seq_vhs_prechained(ctx, 1); its crthip_seq_encode
 * then accepts any first_index and does not walk the stream again.  (include/crt_hip_node.h does all of this.)
 * Device pointers of the phases: the BUFFER CONTRACT above, checked by every phase for the arguments it takes.
 */
int  crthip_vhs_chain(crthip_ctx *ctx, int n, crthip_state *d_state, int draw_aberration);
int  crthip_seq_vhs_prechained(crthip_ctx *ctx, int on);
int  crthip_seq_encode(crthip_ctx *ctx, const crthip_params *p, int n, int first_index, int rn0,
                       const void *d_images, size_t image_stride, crthip_state *d_state);
int  crthip_seq_sync(crthip_ctx *ctx, const crthip_params *p, int n, crthip_state *d_state, int hsync_in, int vsync_in,
                     int *hsync_out, int *vsync_out, int *passes);
int  crthip_seq_decode(crthip_ctx *ctx, const crthip_params *p, int n, void *d_out, size_t out_stride, crthip_state *d_state);
int  crthip_seq_weave(crthip_ctx *ctx, const crthip_params *p, int n, void *d_out, size_t out_stride,
                      const void *d_out_init, int patch_only);
/* Per-field knobs for hosts that drive the phases themselves (one video cut over contexts): the records of THIS shard's n fields,
 * record k = field first_index + k of the video, and the env of the crthip_knobs_prepare call that made them (copied; the records
 * stay the caller's DEVICE memory and are read when the kernels run).  (NULL, NULL) unbinds.  Read by crthip_seq_encode / _sync /
 * _decode only, each of which then requires env->n == n and refuses what crthip_sequence_knobs refuses; crthip_sequence*,
 * crthip_fieldpass* and crthip_stills behave exactly as before whether or not something is bound.  Refused: CRTHIP_SYSTEM_PV1K, an env
 * that does not come from crthip_knobs_prepare. */
int  crthip_seq_bind_knobs(crthip_ctx *ctx, const crthip_knob_rec *d_recs /* DEVICE */, const crthip_knobs_env *env /* host */);

/*
 * Stage-level entry points (used by the drop-in layer, which must keep the host's
 * struct CRT coherent between crt_modulate and crt_demodulate, and by the stage
 * parity tests).  d_analog / d_inp hold n fields at crthip_field_stride() spacing, 4-byte aligned; d_lines / d_state 4-byte
 * aligned; d_images / d_out as everywhere (BUFFER CONTRACT above; what it forbids: CRTHIP_E_ARG before any launch).
 */
/* crt_modulate: writes exactly the samples the reference writes (crt_ntsc.c:205-324),
 * leaving all other samples of d_analog untouched; updates state.ccf (and VHS hsync). */
int  crthip_modulate(crthip_ctx *ctx, const crthip_params *p, int n,
                     const void *d_images, size_t image_stride,
                     signed char *d_analog, crthip_state *d_state);
/* crt_demodulate D1: d_inp = clamp(d_analog + noise), state.rn advanced (crt_core.c:346-367) */
int  crthip_noise(crthip_ctx *ctx, const crthip_params *p, int n,
                  const signed char *d_analog, signed char *d_inp, crthip_state *d_state);
/* crt_demodulate D2-D7: vsync, per-line hsync / burst lock -> line table (crt_core.c:379-479) */
int  crthip_sync(crthip_ctx *ctx, const crthip_params *p, int n,
                 const signed char *d_inp, crthip_state *d_state, crthip_line *d_lines);
/* crt_demodulate D8-D10 (crt_core.c:534-664) */
int  crthip_decode(crthip_ctx *ctx, const crthip_params *p, int n,
                   const signed char *d_inp, const crthip_line *d_lines,
                   void *d_out, size_t out_stride);

/* crthip_fieldpass may cut a batch into `chunks` pieces that alternate between the caller's
 * stream and an internal stream (fenced by events on both sides), so that the latency-bound
 * kernels of one piece overlap the ALU-bound kernels of the next.  1 = off, 0 = chosen per launch (default). */
int  crthip_set_overlap(crthip_ctx *ctx, int chunks);

/* Kernel shape.  0 (default): chosen per launch -- lane-per-scanline kernels (64 scanlines per wavefront, the
 * throughput shape) when the batch fills the chip, scanline-parallel kernels (a DPP row of 16 or 32 lanes per
 * scanline: one filter stage per lane, samples handed on with row_shr, pixels emitted by the whole wavefront from
 * LDS -- the latency shape) for small batches.  1 / 2 force the throughput / latency shape (tests, tuning).
 * Bloom builds (a resampler geometry per scanline) take the throughput shape after a counting sort of the batch's scanlines
 * by beam width, so that the 64 scanlines of a wavefront share one geometry (crt_decode3.hip).
 * The automatic choice minimises the time of ONE batch (encoder: latency shape up to 256 fields, decoder up to 128).  A
 * caller that keeps several batches in flight hides the latency anyway and is better off forcing the
 * throughput shape from 128 fields up (256 fields, three in flight: 1.13 M against 1.01 M fields/s). */
int  crthip_set_shape(crthip_ctx *ctx, int shape);


/* HIP graphs: the encoder's cached tables (blanking / sync / burst skeleton, NES sample table) are rebuilt when the settings they
 * derive from change; this counts the rebuilds.  A graph captured at generation g keeps replaying with generation g's tables --
 * they stay allocated until crthip_destroy and are never written again -- i.e. with the settings it was captured with; compare
 * the value at capture with the current one to know whether a kept graph still matches the context's latest settings. */
unsigned crthip_table_generation(const crthip_ctx *ctx);

/* Decoder output tile: 16 or 32 pixels per row and flush (0 = choose by output width, default). */
int  crthip_set_pixel_tile(crthip_ctx *ctx, int pixels);
/* Encoder signal tile of the fused path: how many bytes of a scanline leave the encoder per store piece.  0 (default) = by
 * batch size (64-byte pieces; 128 / 256-byte pieces for batches that keep the chip full at the occupancy their LDS tile
 * leaves), 16 = always the 64-byte pieces, 32 or 64 = always the large ones.  Same bytes either way (tests, A/B measurements).
 * Environment: CRTHIP_SIG_TILE sets the default of new contexts. */
int  crthip_set_signal_tile(crthip_ctx *ctx, int dwords);
/* Signal layout of the fused path (round 6).  The reference addresses analog[] / inp[] flat: line n of a field starts at sample
 * n * CRT_HRES (crt_ntsc.c:322, crt_core.c:438-461), and so do the stage-level entry points above and the drop-in libraries.  The
 * signal crthip_fieldpass keeps in its own workspace between its encoder and its decoder is not visible to anybody; by default
 * (1) it lives in PADDED lines -- 1024 bytes apart (2048 for the PV-1000's 1920-sample lines), active rows on 128-byte boundaries,
 * the head of every line repeated behind its predecessor so that windows over a line end stay contiguous -- which is what lets the
 * encoder store whole aligned cache lines.  0 = the flat layout there too (A/B measurements; also what the library takes by itself
 * where the padded layout does not reach or does not pay: row overhangs of more than 16 samples, x offsets that put the row before
 * column 114, the rand()-noise VHS build, CRT_DO_VSYNC 0, the NES's PPU-pixel encoder, and the batches of up to 256 fields that go to
 * the scanline-parallel encoder).  Same pictures and states either way.  Environment: CRTHIP_SIG_PAD sets the default
 * of new contexts.
 * crthip_fieldpass_signal: the noisy signal of the first n fields of the context's LAST crthip_fieldpass, repacked into the
 * reference's layout (n fields at crthip_field_stride() spacing: CRT_INPUT_SIZE samples + the CRTHIP_TAIL mirror), i.e. what
 * crt_demodulate leaves in CRT.inp -- for parity tests of the fused path; *padded (optional) tells which layout it came from.
 * Refused after crthip_stills (see there). */
int  crthip_set_signal_layout(crthip_ctx *ctx, int padded);
/* Host only (no device needed): which layout a crthip_fieldpass of n_fields with these (finalized) parameters takes under the default
 * switches and kernel shape `shape` (crthip_set_shape) -- returns 1 = padded, 0 = flat, < 0 = error; layout[] = { bytes between line
 * starts, bytes in front of line 0, valid copy bytes behind every line, samples of an active row beyond its line's end }, *field_stride
 * = bytes between the fields of the workspace.  (What crthip_reserve sizes the workspace for, and what the CPU tests check the
 * geometry rules with.) */
int  crthip_signal_layout_query(const crthip_params *p, int n_fields, int shape, int layout[4], size_t *field_stride);

/* The float form of the decoder's one-pole filter stages (k_decode, tiers 0 / 1 of the 4-sample systems).  A stage
 * x' = x + ((c * (u - x) + 2^15) >> 16) runs as v_sub_f32 + v_fma_f32 in round-toward-minus-infinity on floats that hold x + bias
 * inside [2^23, 2^24) (ulp 1).  With ce = c (x-form, 0 < c < 2^15: the chroma cascades) or c - 65536 (u-form, 2^15 <= c < 1.5 * 2^16:
 * the luma ones) = +-2^k * odd, a = +-2^(15 - k) and n = (odd - 1) / 2:   (ce * d + 32768) >> 16 == floor(ce * (d + a) / 65536) - n.
 * The bias of every state of a cascade moves by `drift` per sample (n, u-form: n + a), neighbouring stages are `dstage` apart
 * (n - a, u-form: n), the input carries the bias of stage 0 plus a.  *_bits are float bit patterns: 0x4B000000 + value - 2^23.
 * Cascades: 0 = luma low, 1 = luma high, 2 = I high, 3 = Q high. */
typedef struct crthip_fstage_cascade {
    int c, form, ce, a, n;          /* coefficient; 0 = x-form, 1 = u-form; effective coefficient; see above */
    int drift, dstage;              /* bias step per sample; bias difference between stage j + 1 and stage j */
    int mul_bits;                   /* float ce / 65536 (exact) */
    int x0_bits, in0_bits, out0_bits;   /* bias of stage 0 before the first sample; of the first input; of stage 3 after the first sample */
    int in_max, state_max;          /* envelope: |input|, |any state| */
    int lo, hi;                     /* smallest / largest value any biased input or state can take over the line (verdict: inside the binade) */
} crthip_fstage_cascade;
typedef struct crthip_fstages {
    int ok;                         /* the verdict: ranges_ok and a system of 4 samples per chroma cycle (the 5-sample decoder keeps
                                       its carriers in LDS and its 1 487-sample lines on the integer stages) */
    int ranges_ok;                  /* the arithmetic alone: coefficient ranges and every value inside the binade */
    int steps;                      /* samples per line the ranges were evaluated for */
    crthip_fstage_cascade cas[4];
} crthip_fstages;
/* Host only: constants, starting biases and verdict for these (finalized) parameters and `steps` samples per line (0: the system's
 * AV_LEN + 1).  Returns the verdict (1: every input and state provably stays inside [2^23, 2^24) at the envelope of tiers 0 / 1 --
 * any signal byte, |carrier| <= 120000, this |bright| --, the coefficient ranges hold and the system has 4 samples per chroma cycle;
 * 0: the integer stages run), < 0 = error.  The cascades' constants are filled in wherever their coefficient is in range. */
int  crthip_float_stages_query(const crthip_params *p, int steps, crthip_fstages *out);
/* 1 if the context's last decoder call (stage-level or inside a field-pass) launched the float-stage kernels, 0 if the integer
 * ones: the switch CRTHIP_DEC_FLOAT=0 (read when the context is created), a verdict of no, a batch whose brightness / contrast put it
 * above tier 1, or a kernel shape without them (the scanline-parallel and wide-run decoders). */
int  crthip_float_stages_used(const crthip_ctx *ctx);
int  crthip_fieldpass_signal(crthip_ctx *ctx, int n, signed char *d_inp_flat, int *padded);
/* Wide-run decoder (wide pictures, crt_decode4.hip): scanlines per wavefront.  0 (default) = by batch size (8 below 96 fields of
 * 1920x1080, 16 from there on), 8 / 16 = always that instantiation.  Same pictures either way (tests pin each instantiation to the
 * oracle, A/B measurements).  Environment: CRTHIP_WIDE_LPW sets the default of new contexts. */
int  crthip_set_wide_lpw(crthip_ctx *ctx, int scanlines_per_wave);

/* The decoder and encoder normally run kernels whose multiplies are the full-rate 24-bit
 * instructions; they are dispatched only where every operand is proven to fit (DESIGN.md,
 * "24-bit multiply envelope"), everything else goes to the exact 32-bit instantiation.  Both
 * give identical results; this switch forces the 32-bit kernels everywhere (tests, debugging).
 * on: 0 automatic, 1 exact kernels only, 2 no 64-bit-mad tiers, 3 never drop the I/Q low cascades (= 2 since round 3). */
int  crthip_set_exact(crthip_ctx *ctx, int on);

/* Per-kernel timing with HIP events on the context's stream (bench.py roofline leg).
 * While enabled every launch is bracketed by an event pair. */
int  crthip_profile_enable(crthip_ctx *ctx, int on);
int  crthip_profile_read(crthip_ctx *ctx, double total_ms[CRTHIP_K_COUNT],
                         int launches[CRTHIP_K_COUNT]);   /* synchronises; resets */

/* Raw device memory helpers for hosts without a tensor library (the C89 drop-in layer). */
void *crthip_malloc(crthip_ctx *ctx, size_t bytes);
void  crthip_free(crthip_ctx *ctx, void *d_ptr);
int   crthip_upload(crthip_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int   crthip_download(crthip_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int   crthip_memset(crthip_ctx *ctx, void *d_dst, int value, size_t bytes);
/* page-lock / release a host buffer so that crthip_upload / crthip_download to it run as direct DMA */
int   crthip_host_register(crthip_ctx *ctx, void *h_ptr, size_t bytes);
int   crthip_host_unregister(crthip_ctx *ctx, void *h_ptr);

#ifdef __cplusplus
}
#endif
#endif

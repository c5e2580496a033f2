/*
 * crt_setup.c -- C89 host code: everything the reference computes once per call or
 * once per crt_init on the CPU stays on the CPU here too (last
 * bullet): timing tables, carrier phases, filter coefficients, geometry.  The result
 * is the `crthip_params` blob handed to the HIP kernels (and broadcast over RCCL in
 * the multi-GPU driver).
 */
#include "crt_setup.h"

#include <string.h>

/* ------------------------------------------------------------------------- */
/* fixed-point trig: 14-bit angle (16384 = one turn) -> 15-bit sine / cosine   */
/* reference: crt_core.c:19-61                                                */
/* ------------------------------------------------------------------------- */

/* first quadrant in 16 steps, one guard entry for the interpolation */
static const int sine_knots[18] = {
    0, 3208, 6392, 9512, 12536, 15440, 18200, 20784, 23168,
    25328, 27240, 28896, 30272, 31352, 32136, 32608, 32768, 32608
};

static int
sine_q1(int a)
{
    int k = (a >> 8) & 255;
    int t = a & 255;
    return sine_knots[k] + (((sine_knots[k + 1] - sine_knots[k]) * t) >> 8);
}

void
crt_setup_sincos14(int *s, int *c, int n)
{
    int a, sn, cs;

    n &= 16383;
    a = n & 8191;                 /* position inside the half turn */
    if (a < 4096) {
        sn = sine_q1(a);
        cs = sine_q1(4096 - a);
    } else {
        sn = sine_q1(8192 - a);
        cs = -sine_q1(a - 4096);
    }
    if (n & 8192) {               /* second half turn: both change sign */
        sn = -sn;
        cs = -cs;
    }
    *s = sn;
    *c = cs;
}

int
crt_setup_bpp4fmt(int format)
{
    switch (format) {
    case CRTHIP_FMT_RGB:
    case CRTHIP_FMT_BGR:
        return 3;
    case CRTHIP_FMT_ARGB:
    case CRTHIP_FMT_RGBA:
    case CRTHIP_FMT_ABGR:
    case CRTHIP_FMT_BGRA:
        return 4;
    default:
        return 0;
    }
}

/* ------------------------------------------------------------------------- */
/* Q11 exponential, reference: crt_ntsc.c:25-83                                */
/* ------------------------------------------------------------------------- */
#define Q11 2048

int
crt_setup_expx(int n)
{
    /* e^0 .. e^4 in Q11 */
    static const int e_int[5] = { Q11, 5567, 15133, 41135, 111817 };
    int inverse, ip, r, series, term, fact, k;

    if (n == 0) {
        return Q11;
    }
    inverse = (n < 0);
    if (inverse) {
        n = -n;
    }
    ip = n >> 11;
    r = Q11;
    for (k = ip / 4; k > 0; k--) {
        r = (r * e_int[4]) >> 11;
    }
    if (ip & 3) {
        r = (r * e_int[ip & 3]) >> 11;
    }
    /* Taylor series of the fractional part; same truncation rule as the reference */
    n &= Q11 - 1;
    series = 0;
    term = Q11;
    fact = 1;
    for (k = 1; k < 17; k++) {
        series += term / fact;
        term = (term * n) >> 11;
        fact *= k;
        if (fact > term || term <= 0 || fact <= 0) {
            break;
        }
    }
    r = (r * series) >> 11;
    if (inverse) {
        r = (Q11 << 11) / r;
    }
    return r;
}

/* ------------------------------------------------------------------------- */
/* system tables                                                              */
/* ------------------------------------------------------------------------- */
#define L_FREQ 1431818

int
crt_sysdef_get(struct crt_sysdef *d, int system, int chroma_pattern)
{
    int cc_line;

    memset(d, 0, sizeof(*d));
    d->system = system;
    d->chroma_pattern = chroma_pattern;
    d->vres = 262;
    d->cc_samples = 4;
    d->cb_len = 40;
    d->burst_off = 33;
    d->q_off = -90;
    d->hue_in_mod = 1;
    d->equ_a_lo = 0; d->equ_a_hi = 3; d->equ_b_lo = 7; d->equ_b_hi = 9;     /* crt_ntsc.c:211 */
    d->vs_lo = 4; d->vs_hi = 6; d->vs_by_field = 1;                            /* crt_ntsc.c:217-223 */
    if (system == CRTHIP_SYSTEM_NTSC || system == CRTHIP_SYSTEM_NTSCVHS || system == CRTHIP_SYSTEM_TEMP) {
        /* crt_ntsc.h:25-109 (= crt_ntscvhs.h, crt_template.h): times in ns on a 63500 ns line */
        const int line_ns = 63500;
        if (system == CRTHIP_SYSTEM_TEMP) {
            if (chroma_pattern != 1) {
                return CRTHIP_E_ARG;
            }
        } else if (chroma_pattern != 0 && chroma_pattern != 1) {
            return CRTHIP_E_ARG;
        }
        cc_line = (chroma_pattern == 1) ? 2275 : 2280;
        d->hres = cc_line * 4 / 10;
        d->top = 21;
        d->bot = 261;
        d->vper = (system == CRTHIP_SYSTEM_TEMP) ? 2 : 1;
        d->hsync_window = 8;
        d->vsync_window = 8;
        d->white_level = 100;
        d->burst_level = 20;
        d->black_level = 7;
        d->blank_level = 0;
        d->sync_level = -40;
        d->sync_beg = 1500 * d->hres / line_ns;
        d->bw_beg = 6200 * d->hres / line_ns;
        d->cb_beg = 6800 * d->hres / line_ns;
        d->av_beg = 10900 * d->hres / line_ns;
        d->av_len = 52600 * d->hres / line_ns;
        d->field_rows = 1;
        if (system == CRTHIP_SYSTEM_NTSCVHS) {   /* VHS_SP, crt_ntscvhs.h:109-113 */
            d->y_freq = 300000;
            d->i_freq = 62700;
            d->q_freq = 62700;
        } else {                                 /* crt_ntsc.h:99-102, crt_template.h:107-110 */
            d->y_freq = 420000;
            d->i_freq = 150000;
            d->q_freq = 55000;
        }
        if (system == CRTHIP_SYSTEM_TEMP) {      /* crt_template.h:133-146, crt_template.c:171-183,240 */
            d->line_rows = 1;
            d->burst_off = -60 - 90;
            d->equ_a_hi = 2;
            d->vs_lo = 3;
            d->ccf_row_shift = 3;
        }
    } else if (system == CRTHIP_SYSTEM_PV1K) {
        /* crt_pv1k.h:24-98: 5 samples per chroma cycle; times in units of 4 dots (892 ns), 71 units per line */
        const int unit = 892, line_ns = 71 * 892;
        if (chroma_pattern != 1) {
            return CRTHIP_E_ARG;
        }
        d->hres = 2304 * 5 / 6;
        d->top = 21;
        d->bot = 261;
        d->vper = 5;
        d->cc_samples = 5;
        d->cb_len = 50;
        d->hsync_window = 8;
        d->vsync_window = 8;
        d->white_level = 100;
        d->burst_level = 20;
        d->black_level = 7;
        d->blank_level = 0;
        d->sync_level = -40;
        d->sync_beg = 3 * unit * d->hres / line_ns;
        d->bw_beg = 6 * unit * d->hres / line_ns;
        d->cb_beg = 8 * unit * d->hres / line_ns;
        d->av_beg = 16 * unit * d->hres / line_ns;
        d->av_len = 55 * unit * d->hres / line_ns;
        d->y_freq = 420000;
        d->i_freq = 150000;
        d->q_freq = 55000;
        d->field_rows = 1;
        d->line_rows = 1;
        d->burst_off = -72;                      /* crt_pv1k.c:172: n - step */
        d->q_off = 90;
        d->equ_a_hi = -1;                        /* crt_pv1k.c:197: only lines 7..9 */
        d->vs_lo = 258;                          /* crt_pv1k.c:204 */
        d->vs_hi = 260;
        d->ccf_row_shift = 3;
    } else if (system == CRTHIP_SYSTEM_NES || system == CRTHIP_SYSTEM_NESRGB || system == CRTHIP_SYSTEM_SNES) {
        /* crt_nes.h:30-126, crt_nesrgb.h, crt_snes.h:24-116: positions in PPU pixels on a 341 px line */
        const int line_px = 341;
        if (system == CRTHIP_SYSTEM_SNES) {
            if (chroma_pattern != 1) {
                return CRTHIP_E_ARG;
            }
            cc_line = 2273;
        } else {
            if (chroma_pattern < 0 || chroma_pattern > 2) {
                return CRTHIP_E_ARG;
            }
            cc_line = (chroma_pattern == 1) ? 2275 : ((chroma_pattern == 2) ? 2273 : 2280);
        }
        d->hres = cc_line * 4 / 10;
        d->top = 15;
        d->bot = 255;
        d->vper = 3;
        d->hsync_window = 6;
        d->vsync_window = 6;
        d->blank_level = 0;
        if (system == CRTHIP_SYSTEM_SNES) {
            d->white_level = 100;
            d->burst_level = 20;
            d->black_level = 7;
            d->sync_level = -40;
            d->burst_off = 210 - 90;             /* crt_snes.c:176: n - step + HUE_OFFSET */
            d->equ_a_hi = 2;                     /* crt_snes.h:137-146 */
            d->vs_lo = 3;
            d->vs_by_field = 0;                  /* crt_snes.c:216-218: even pattern only */
            d->ccf_row_shift = 3;
        } else {
            d->white_level = (system == CRTHIP_SYSTEM_NES) ? 110 : 100;
            d->burst_level = 30;
            d->black_level = 0;
            d->sync_level = -37;
            d->nes_timing = 1;
            d->ppu_input = (system == CRTHIP_SYSTEM_NES);
            if (system == CRTHIP_SYSTEM_NESRGB) {
                d->burst_off = 90 + 33;          /* crt_nesrgb.c:72 */
                d->hue_in_mod = 0;
            }
        }
        d->line_rows = 1;
        d->sync_beg = 9 * d->hres / line_px;
        d->bw_beg = 34 * d->hres / line_px;
        d->cb_beg = 38 * d->hres / line_px;
        d->av_beg = 74 * d->hres / line_px;
        d->av_len = 256 * d->hres / line_px;
        d->vs_sep_end = 327 * d->hres / line_px;
    } else {
        return CRTHIP_E_ARG;
    }
    d->vert_step = d->vper > 1 ? 360 / d->vper : 0;
    if (system == CRTHIP_SYSTEM_PV1K) {
        d->vert_step = 360 * 2 / 5;              /* crt_pv1k.c:168 */
    }
    d->input_size = d->hres * d->vres;
    d->lines = d->bot - d->top;
    d->hsync_thresh = 4 * d->sync_level;     /* CRT_HSYNC_THRESH */
    d->vsync_thresh = 94 * d->sync_level;    /* CRT_VSYNC_THRESH */
    return CRTHIP_OK;
}

int
crthip_input_size(int system, int chroma_pattern)
{
    struct crt_sysdef d;
    if (crt_sysdef_get(&d, system, chroma_pattern) != CRTHIP_OK) {
        return 0;
    }
    return d.input_size;
}

int
crthip_hres(int system, int chroma_pattern)
{
    struct crt_sysdef d;
    if (crt_sysdef_get(&d, system, chroma_pattern) != CRTHIP_OK) {
        return 0;
    }
    return d.hres;
}

int
crthip_lines(int system)
{
    struct crt_sysdef d;
    if (crt_sysdef_get(&d, system, (system == CRTHIP_SYSTEM_NES || system == CRTHIP_SYSTEM_NESRGB) ? 2 : 1) != CRTHIP_OK) {
        return 0;
    }
    return d.lines;
}

size_t
crthip_field_stride(int system, int chroma_pattern)
{
    /* INPUT_SIZE + room for the mirrored struct tail and for the widest out-of-contract
     * window (pos <= INPUT_SIZE-1, window AV_LEN, 16-byte vector reads), rounded to 256 */
    struct crt_sysdef d;
    size_t n;
    if (crt_sysdef_get(&d, system, chroma_pattern) != CRTHIP_OK) {
        return 0;
    }
    n = (size_t) d.input_size;
    n += (size_t) (d.av_len > 960 ? 2048 : 1024);
    return (n + 255) & ~(size_t) 255;
}

/* ------------------------------------------------------------------------- */
/* parameter blob                                                             */
/* ------------------------------------------------------------------------- */

int
crthip_params_default(crthip_params *p, int system, int chroma_pattern)
{
    struct crt_sysdef d;

    if (p == 0 || crt_sysdef_get(&d, system, chroma_pattern) != CRTHIP_OK) {
        return CRTHIP_E_ARG;
    }
    memset(p, 0, sizeof(*p));
    p->system = system;
    p->chroma_pattern = chroma_pattern;
    p->format = CRTHIP_FMT_BGRA;
    p->out_format = CRTHIP_FMT_BGRA;
    p->as_color = 1;
    /* crt_reset, crt_core.c:250-261 */
    p->saturation = 10;
    p->contrast = 180;
    p->white_point = 100;
    return CRTHIP_OK;
}

/* one-pole low-pass coefficient, crt_ntsc.c:98-106 (init_iir) */
static int
lowpass_coef(int limit)
{
    int rate = (L_FREQ << 9) / limit;
    return Q11 - crt_setup_expx(-((6434 << 9) / rate));
}

/* fade^age of every byte value (crt_main.c:446-450 per byte: the four shifted terms never carry into the next byte) */
int
crthip_phosphor_table(int age, unsigned char lut[256])
{
    int c, a;

    if (age < 0 || lut == 0) {
        return CRTHIP_E_ARG;
    }
    for (c = 0; c < 256; c++) {
        unsigned v = (unsigned) c;
        for (a = 0; a < age && v != 0; a++) {
            v = (v >> 1) + (v >> 2) + (v >> 3) + (v >> 4);
        }
        lut[c] = (unsigned char) v;
    }
    return CRTHIP_OK;
}

/* The three carrier tables of the RGB-input encoders for one encoder hue (the tables zeroed by the caller): what
 * crthip_params_finalize keeps in crthip_params, and crthip_knobs_prepare8 in every field's crthip_hue_rec. */
static void
rgb_carriers(const struct crt_sysdef *d, int chroma_pattern, int as_color, int hue,
             int burst[CRTHIP_CARRIER_ROWS][CRTHIP_MAX_CCS], int modI[CRTHIP_CARRIER_ROWS][CRTHIP_MAX_CCS],
             int modQ[CRTHIP_CARRIER_ROWS][CRTHIP_MAX_CCS])
{
    const int step = 360 / d->cc_samples;
    int k, r, sn, cs, rows;

    if (as_color || d->nes_timing) {                            /* NES-RGB has no as_color member: always colour */
        rows = d->line_rows ? CRTHIP_CARRIER_ROWS : 1;
        for (r = 0; r < rows; r++) {
            for (k = 0; k < d->cc_samples; k++) {
                /* crt_ntsc.c:175-182; crt_snes.c:171-182; crt_pv1k.c:167-178; crt_nesrgb.c:67-78 */
                int ang = r * d->vert_step + k * step;
                int hue_mod = d->hue_in_mod ? hue : 0;
                crt_setup_sincos14(&sn, &cs, (ang + hue + d->burst_off) * 8192 / 180);
                burst[r][k] = sn >> 10;
                crt_setup_sincos14(&sn, &cs, (ang + hue_mod) * 8192 / 180);
                modI[r][k] = sn >> 10;
                crt_setup_sincos14(&sn, &cs, (ang + hue_mod + d->q_off) * 8192 / 180);
                modQ[r][k] = sn >> 10;
            }
        }
        if (!d->line_rows) {
            /* row 1 = the lines of a field whose parity equals the frame's (inv_phase, crt_ntsc.c:199-200,
             * 243-247): burst advanced by half a cycle, modulation carriers negated -- CRT_CHROMA_PATTERN 1 only */
            for (k = 0; k < 4; k++) {
                if (chroma_pattern == 1) {
                    burst[1][k] = burst[0][(k + 2) & 3];
                    modI[1][k] = -modI[0][k];
                    modQ[1][k] = -modQ[0][k];
                } else {
                    burst[1][k] = burst[0][k];
                    modI[1][k] = modI[0][k];
                    modQ[1][k] = modQ[0][k];
                }
            }
        }
    }
}

/* ceil(2^32 * w / destw) by long division (C89: no 64-bit type): crthip_params.col_step_lo / _hi, and crthip_size_rec's per field */
static void
col_step_for(int w, int destw, unsigned *step_lo, unsigned *step_hi)
{
    unsigned dw = (unsigned) (destw > 0 ? destw : 1), r = (unsigned) w % dw, lo = 0;
    int i;

    *step_hi = (unsigned) w / dw;
    for (i = 0; i < 32; i++) {
        r <<= 1;
        lo <<= 1;
        if (r >= dw) {
            r -= dw;
            lo |= 1u;
        }
    }
    if (r != 0 && ++lo == 0) {
        (*step_hi)++;
    }
    *step_lo = lo;
}

int
crthip_params_finalize(crthip_params *p)
{
    /* crt_core.c:272-286: band edges in kHz and band gains (Q16) for Y, I, Q */
    static const int edge_khz[3][2] = { { 1500, 3000 }, { 80, 1150 }, { 80, 1000 } };
    static const int band_gain4[3][3] = {
        { 65536, 8192, 9175 }, { 65536, 65536, 1311 }, { 65536, 65536, 0 }
    };
    static const int band_gain5[3][3] = {           /* CRT_CC_SAMPLES == 5, crt_core.c:281-283 */
        { 65536, 12192, 7775 }, { 65536, 65536, 1311 }, { 65536, 65536, 0 }
    };
    struct crt_sysdef d;
    int k, r, sn, cs;

    if (p == 0 || crt_sysdef_get(&d, p->system, p->chroma_pattern) != CRTHIP_OK) {
        return CRTHIP_E_ARG;
    }
    p->finalized = 0;
    p->out_bpp = crt_setup_bpp4fmt(p->out_format);
    if (p->outw <= 0 || p->outh <= 0 || p->w <= 0 || p->h <= 0) {
        return CRTHIP_E_ARG;
    }
    p->eq_kernel = (p->flags & CRTHIP_F_EQ_FIR_MASK) >> 8;      /* crt_core.c:85-88 */
    if (p->eq_kernel != 0 && (p->eq_kernel < 4 || p->eq_kernel > 7)) {
        return CRTHIP_E_ARG;
    }
    p->bloom = (p->flags & CRTHIP_F_BLOOM) != 0;                /* crt_core.h:70 */
    if (p->bloom && (d.nes_timing || p->eq_kernel != 0)) {
        return CRTHIP_E_ARG;                                    /* "does not work for NES" (crt_core.h:70) */
    }
    if ((p->flags & (CRTHIP_F_VHS_LP | CRTHIP_F_VHS_EP | CRTHIP_F_VHS_LCG_NOISE)) && p->system != CRTHIP_SYSTEM_NTSCVHS) {
        return CRTHIP_E_ARG;
    }
    if ((p->flags & CRTHIP_F_VHS_LP) && (p->flags & CRTHIP_F_VHS_EP)) {
        return CRTHIP_E_ARG;
    }
    if ((p->flags & CRTHIP_F_VHS_SET_STREAMS) && (p->system != CRTHIP_SYSTEM_NTSCVHS || (p->flags & CRTHIP_F_VHS_LCG_NOISE))) {
        return CRTHIP_E_ARG;                                    /* one rand() stream per set: only the rand() build has one */
    }
    if ((p->flags & CRTHIP_F_NES_BORDER) && p->system != CRTHIP_SYSTEM_NES) {
        return CRTHIP_E_ARG;
    }
    if ((p->flags & CRTHIP_F_PHOSPHOR_FADE) && (p->flags & CRTHIP_F_PHOSPHOR_CLEAR)) {
        return CRTHIP_E_ARG;                                    /* crt_main.c:459-463: fade or clear, never both */
    }

    memset(p->burst, 0, sizeof(p->burst));
    memset(p->modI, 0, sizeof(p->modI));
    memset(p->modQ, 0, sizeof(p->modQ));
    memset(p->dem_cs, 0, sizeof(p->dem_cs));
    memset(p->dem_sn, 0, sizeof(p->dem_sn));
    p->iir_c[0] = p->iir_c[1] = p->iir_c[2] = 0;
    if (d.ppu_input) {
        /* crt_nes.c:110-136.  Row r = (line % 3) + dot_crawl_offset: the reference reduces the ANGLE mod 360 with
         * C's truncating %, not the row, so the unreduced row keeps negative hues exact */
        p->in_bpp = 2;
        p->destw = d.av_len;
        p->desth = d.lines;
        p->xo = (d.av_beg + p->xoffset) & ~3;
        p->yo = d.top + p->yoffset;
        for (r = 0; r < CRTHIP_CARRIER_ROWS; r++) {
            for (k = 0; k < 4; k++) {
                int ang = (p->hue + k * 90 + r * 120 + 33) % 360;
                crt_setup_sincos14(&sn, &cs, ang * 8192 / 180);
                p->burst[r][k] = sn >> 10;
            }
        }
    } else {
        p->in_bpp = crt_setup_bpp4fmt(p->format);
        /* geometry: crt_ntsc.c:132-133, 148-173, 194-203; crt_nesrgb.c:51-52, 85-89 */
        p->destw = d.av_len;
        if (d.nes_timing) {
            p->desth = d.lines;
        } else if (p->bloom) {
            p->destw = (d.av_len * 55500) >> 16;
            p->desth = (d.lines * 63500) >> 16;
        } else {
            p->desth = (d.lines * 64500) >> 16;
        }
        if (p->raw && !d.nes_timing) {
            if (p->w < p->destw) {
                p->destw = p->w;
            }
            if (p->h < p->desth) {
                p->desth = p->h;
            }
        }
        p->xo = d.av_beg + p->xoffset + (d.av_len - p->destw) / 2;
        p->yo = d.top + p->yoffset + (d.lines - p->desth) / 2;
        if (d.line_rows && !d.nes_timing) {
            p->xo = p->xo - (p->xo % d.cc_samples);             /* crt_snes.c:201 */
        } else {
            p->xo &= ~3;
        }
        rgb_carriers(&d, p->chroma_pattern, p->as_color, p->hue, p->burst, p->modI, p->modQ);
        if (d.y_freq != 0) {
            int yf = d.y_freq, jf = d.i_freq, qf = d.q_freq;
            if (p->system == CRTHIP_SYSTEM_NTSCVHS && (p->flags & CRTHIP_F_VHS_LP)) {        /* crt_ntscvhs.h:114-118 */
                yf = 240000; jf = 40000; qf = 40000;
            } else if (p->system == CRTHIP_SYSTEM_NTSCVHS && (p->flags & CRTHIP_F_VHS_EP)) { /* crt_ntscvhs.h:119-123 */
                yf = 200000; jf = 37000; qf = 37000;
            }
            p->iir_c[0] = lowpass_coef(yf);
            p->iir_c[1] = lowpass_coef(jf);
            p->iir_c[2] = lowpass_coef(qf);
        }
    }

    /* crt_core.c:171-196 with EQ_P = 16: cut-off as 2*sin(pi*f/rate), Q16 */
    for (k = 0; k < 3; k++) {
        int f_lo = d.hres * (edge_khz[k][0] * 100) / L_FREQ;
        int f_hi = d.hres * (edge_khz[k][1] * 100) / L_FREQ;
        crt_setup_sincos14(&sn, &cs, 8192 * f_lo / d.hres);
        p->eq_lf[k] = 2 * (sn << 1);
        crt_setup_sincos14(&sn, &cs, 8192 * f_hi / d.hres);
        p->eq_hf[k] = 2 * (sn << 1);
        for (r = 0; r < 3; r++) {
            p->eq_g[k][r] = d.cc_samples == 5 ? band_gain5[k][r] : band_gain4[k][r];
        }
    }

    /* crt_core.c:305, 318-320, 404-405, 528 */
    crt_setup_sincos14(&sn, &cs, ((p->mon_hue % 360) + 33) * 8192 / 180);
    p->huesn = sn >> 11;
    p->huecs = cs >> 11;
    if (d.cc_samples == 5) {
        /* crt_core.c:484,497-505: demodulation carriers rotated by the monitor hue, one entry per sample phase */
        int ang = p->mon_hue % 360;
        for (k = 0; k < 5; k++) {
            crt_setup_sincos14(&sn, &cs, ang * 8192 / 180);
            p->dem_cs[0][k] = cs;
            p->dem_sn[0][k] = sn;
            crt_setup_sincos14(&sn, &cs, (ang + 90) * 8192 / 180);
            p->dem_cs[1][k] = cs;
            p->dem_sn[1][k] = sn;
            ang += 360 / 5;
        }
    }
    p->bright = p->brightness - (d.black_level + p->black_point);
    p->white = d.white_level * p->white_point / 100;
    p->ire_base = d.black_level + p->black_point;
    p->dx = ((d.av_len - 1) << 12) / p->outw;
    p->ratio = (((p->outh << 16) / d.lines) + 32768) >> 16;
    col_step_for(p->w, p->destw, &p->col_step_lo, &p->col_step_hi);
    p->bloom_max_e = (128 + (p->noise / 2)) * d.av_len;         /* crt_core.c:400 */
    if (p->bloom && (p->bloom_max_e <= 0 || p->noise < 0)) {
        /* max_e <= 0: the reference divides by zero (:522).  noise < 0 shrinks max_e, the beam-energy term then drives
         * line_w past AV_LEN + 16 and scanL (:521) below zero: the reference reads in front of its line buffer
         * (undefined there), the row decoder would leave its LDS window -- refused */
        return CRTHIP_E_ARG;
    }
    p->loskip_wave_max = 65532;                                 /* |s| <= 127, see crt_hip.h */
    p->finalized = CRTHIP_PARAMS_MAGIC;
    return CRTHIP_OK;
}

/* NES composite level of PPU pixel p at phase `phase`, crt_nes.c:21-61 (host copy: only used to bound the signal) */
static int
nes_level(int p, int phase)
{
    static const int active[6] = { 0300, 0100, 0500, 0400, 0600, 0200 };
    static const int ire[16] = {
        -12042, 0, 34406, 81427,        /* low, no emphasis  */
        -17203, -8028, 19497, 57342,    /* low, emphasis     */
        43581, 75693, 112965, 112965,   /* high, no emphasis */
        26951, 52181, 83721, 83721      /* high, emphasis    */
    };
    int hue = p & 15, high, emph;

    if (hue >= 14) {
        return 0;
    }
    high = ((hue + phase) % 12) < 6;
    if (hue == 0) {
        high = 1;
    }
    if (hue == 13) {
        high = 0;
    }
    emph = (p & 0700 & active[(phase >> 1) % 6]) != 0;
    return ire[(high << 3) + (emph << 2) + ((p >> 4) & 3)];
}

/*
 * Range [*lo, *hi] of every sample of a field as crt_modulate leaves it in a crt_init-clean analog[] and the noise stage
 * of crt_demodulate hands it on (crt_core.c:359-366).  The struct bytes mirrored behind inp[] (CRTHIP_TAIL) are NOT
 * covered: a line whose window reaches them keeps the any-signal bound (line_tier_flags, crt_dev.h).  Used by
 * the fused entry points to widen the decoder's no-low-cascade envelope (crthip_params.loskip_wave_max); VHS, whose
 * noise gain is data dependent (crt_core.c:349-357), reports the full range.
 */
void
crt_setup_signal_range(const crthip_params *p, int *lo, int *hi)
{
    struct crt_sysdef d;
    int a_lo = 0, a_hi = 0, r, k, v, t0, t1;

    *lo = -128;
    *hi = 127;
    if (crt_sysdef_get(&d, p->system, p->chroma_pattern) != CRTHIP_OK ||
        (p->system == CRTHIP_SYSTEM_NTSCVHS && !(p->flags & CRTHIP_F_VHS_LCG_NOISE))) {
        return;
    }
    /* skeleton: blank, sync tip, burst (crt_ntsc.c:205-252, crt_nes.c:81-104) */
    if (d.sync_level < a_lo) a_lo = d.sync_level;
    if (d.blank_level > a_hi) a_hi = d.blank_level;
    for (r = 0; r < CRTHIP_CARRIER_ROWS; r++) {
        for (k = 0; k < CRTHIP_MAX_CCS; k++) {
            v = (int) (signed char) ((d.blank_level + p->burst[r][k] * d.burst_level) >> 5);
            if (v < a_lo) a_lo = v;
            if (v > a_hi) a_hi = v;
        }
    }
    /* active video */
    if (d.ppu_input) {
        int px, ph;
        for (px = 0; px < 512; px++) {                      /* crt_nes.c:162-193, every pixel value at every phase */
            for (ph = 0; ph < 12; ph++) {
                int ire = d.black_level + p->black_point + nes_level(px, ph) + nes_level(px, ph + 1) +
                          nes_level(px, ph + 2) + nes_level(px, ph + 3);
                v = (int) (signed char) ((ire * p->white_point / 100) >> 12);
                if (v < a_lo) a_lo = v;
                if (v > a_hi) a_hi = v;
            }
        }
    } else {
        if (110 > a_hi) a_hi = 110;                         /* clamped to 0..110, crt_ntsc.c:319-320 */
    }
    /* noise term ((byte - 0x7f) * noise) >> 8, byte = 0..255 (range check first: the products below must not overflow) */
    if (p->noise > (1 << 20) || p->noise < -(1 << 20)) {
        return;
    }
    t0 = (-127 * p->noise) >> 8;
    t1 = (128 * p->noise) >> 8;
    a_lo += t0 < t1 ? t0 : t1;
    a_hi += t0 < t1 ? t1 : t0;
    if (a_lo < -127) a_lo = -127;                           /* crt_core.c:363-364 */
    if (a_hi > 127) a_hi = 127;
    *lo = a_lo;
    *hi = a_hi;
}

/* largest |wave| for which the chroma equaliser input u = (s * wave) >> 9, s in [lo, hi], keeps every state of the
 * cascades inside the hull H of the inputs and 0 with max|H| <= 32767 and width(H) <= 32767 (see eq_step64 in
 * crt_decode.hip): |u| <= |s| * W / 512 + 1 */
int
crt_setup_loskip_bound(int lo, int hi)
{
    int m, wd;
    long a, b;

    if (lo > 0) lo = 0;
    if (hi < 0) hi = 0;
    m = -lo > hi ? -lo : hi;
    wd = hi - lo;
    if (m <= 0 || wd <= 0) {
        return 65532;
    }
    a = (32766L * 512L) / m;
    b = (32765L * 512L) / wd;
    if (b < a) a = b;
    if (a < 65532L) a = 65532L;
    if (a > 120000L) a = 120000L;                           /* T0_WAVE_MAX: the 64-bit-mad tiers end there anyway */
    return (int) a;
}

/* ------------------------------------------------------------------------- */
/* per-field knobs (crthip_fieldpass_knobs)                                    */
/* ------------------------------------------------------------------------- */
static int
abs_sat(int v)
{
    if (v >= 0) {
        return v;
    }
    return v < -0x7fffffff ? 0x7fffffff : -v;
}

/*
 * The per-field records and the batch-wide bounds of n knob triples: field by field what crthip_params_finalize derives from
 * mon_hue (huesn / huecs) and noise (bloom_max_e), its refusals included; the bounds are what the launch code otherwise reads
 * from the uniform noise and saturation.  The signal range grows with the noise on either side of zero, so the no-low-cascade
 * bound of the batch is the smaller of the bounds at the smallest and the largest noise.
 */
/* kn: the caller's knobs as ints, `stride` apart: noise, mon_hue, saturation and -- pic: crthip_knobs5 -- brightness, contrast */
/* levs != 0 (crthip_knobs_prepare7): two more ints per field, black_point and white_point -- the field's bright and tier floor come
 * from ITS black point, levs[k] = the encoder's pair as crthip_params_finalize derives it, lenv = the batch's largest magnitudes */
static int
knobs_prepare_any(const crthip_params *p, int n, const int *kn, int stride, int pic, crthip_knob_rec *recs, crthip_knobs_env *env,
                  crthip_level_rec *levs, crthip_levels_env *lenv)
{
    struct crt_sysdef d;
    crthip_params q;
    int k, sn, cs, lo, hi, bound, b2;
    int noise_lo, noise_hi, noise_abs = 0, sat_abs = 0;
    int floor_lo = 3, floor_hi = 0, bright_abs = 0;
    int white_abs = 0, base_abs = 0;

    if (p == 0 || kn == 0 || recs == 0 || env == 0 || n <= 0 || p->finalized != CRTHIP_PARAMS_MAGIC ||
        crt_sysdef_get(&d, p->system, p->chroma_pattern) != CRTHIP_OK) {
        return CRTHIP_E_ARG;
    }
    memset(env, 0, sizeof(*env));
    noise_lo = noise_hi = kn[0];
    for (k = 0; k < n; k++) {
        const int *const kk = kn + (size_t) k * (size_t) stride;
        const int noise = kk[0];
        const int max_e = (128 + (noise / 2)) * d.av_len;           /* crt_core.c:400 */
        if (p->bloom && (max_e <= 0 || noise < 0)) {
            return CRTHIP_E_ARG;                                    /* as crthip_params_finalize */
        }
        memset(&recs[k], 0, sizeof(recs[k]));
        crt_setup_sincos14(&sn, &cs, ((kk[1] % 360) + 33) * 8192 / 180);                 /* crt_core.c:318-320 */
        recs[k].noise = noise;
        recs[k].huesn = sn >> 11;
        recs[k].huecs = cs >> 11;
        recs[k].saturation = kk[2];
        recs[k].bloom_max_e = max_e;
        if (pic) {
            /* the decoder's two: the luma offset as crthip_params_finalize derives it (crt_core.c:305), the contrast as it is, and
             * the tier they ask of the field's lines (k_hsync_wave turns it into the lines' tier flags) */
            const int black_point = levs ? kk[5] : p->black_point;
            const int bright = kk[3] - (d.black_level + black_point);
            const int fl = crt_setup_decoder_floor(p, bright, kk[4]);
            recs[k].bright = bright;
            recs[k].contrast = kk[4];
            recs[k].tier_floor = fl;
            if (fl < floor_lo) floor_lo = fl;
            if (fl > floor_hi) floor_hi = fl;
            if (fl < 2 && abs_sat(bright) > bright_abs) bright_abs = abs_sat(bright);
        }
        if (levs) {
            memset(&levs[k], 0, sizeof(levs[k]));
            levs[k].white = d.white_level * kk[6] / 100;            /* crt_ntsc.c:318, as crthip_params_finalize */
            levs[k].ire_base = d.black_level + kk[5];               /* crt_ntsc.c:311 */
            if (abs_sat(levs[k].white) > white_abs) white_abs = abs_sat(levs[k].white);
            if (abs_sat(levs[k].ire_base) > base_abs) base_abs = abs_sat(levs[k].ire_base);
        }
        if (noise < noise_lo) noise_lo = noise;
        if (noise > noise_hi) noise_hi = noise;
        if (abs_sat(noise) > noise_abs) noise_abs = abs_sat(noise);
        if (abs_sat(kk[2]) > sat_abs) sat_abs = abs_sat(kk[2]);
    }
    /* The signal range of a field: sync level ... white level + noise term (crt_setup_signal_range).  The RGB encoders clamp the level
     * to 0 .. 110 whatever white and ire_base are (crt_ntsc.c:319-320), so there one evaluation per noise extreme covers every field;
     * the PPU encoder's samples depend on the pair itself, so the bound is taken over the fields' pairs (a run of equal pairs once). */
    q = *p;
    bound = b2 = 0x7fffffff;
    for (k = 0; k < n; k++) {
        if (levs) {
            const int *const kk = kn + (size_t) k * (size_t) stride;
            if (k > 0 && (!d.ppu_input || (kk[5] == q.black_point && kk[6] == q.white_point))) continue;
            q.black_point = kk[5];
            q.white_point = kk[6];
        } else if (k > 0) {
            break;
        }
        q.noise = noise_lo;
        crt_setup_signal_range(&q, &lo, &hi);
        sn = crt_setup_loskip_bound(lo, hi);
        if (sn < bound) bound = sn;
        q.noise = noise_hi;
        crt_setup_signal_range(&q, &lo, &hi);
        sn = crt_setup_loskip_bound(lo, hi);
        if (sn < b2) b2 = sn;
    }
    env->magic = CRTHIP_KNOBS_MAGIC;
    env->n = n;
    env->noise_max = noise_abs;
    env->sat_abs_max = sat_abs;
    env->loskip_wave_max = b2 < bound ? b2 : bound;
    if (pic) {
        env->pic = 1;
        env->tier_floors = floor_lo | (floor_hi << 8);
        env->bright_abs_lo = bright_abs;
    }
    if (levs) {
        memset(lenv, 0, sizeof(*lenv));
        lenv->magic = CRTHIP_LEVELS_MAGIC;
        lenv->n = n;
        lenv->white_abs_max = white_abs;
        lenv->ire_base_abs_max = base_abs;
    }
    return CRTHIP_OK;
}

int
crthip_knobs_prepare(const crthip_params *p, int n, const crthip_knobs *knobs, crthip_knob_rec *recs, crthip_knobs_env *env)
{
    return knobs_prepare_any(p, n, knobs ? &knobs->noise : 0, (int) (sizeof(*knobs) / sizeof(int)), 0, recs, env, 0, 0);
}

/* The same with brightness and contrast per field: the records' last three words and the env's picture words filled in. */
int
crthip_knobs_prepare5(const crthip_params *p, int n, const crthip_knobs5 *knobs, crthip_knob_rec *recs, crthip_knobs_env *env)
{
    return knobs_prepare_any(p, n, knobs ? &knobs->noise : 0, (int) (sizeof(*knobs) / sizeof(int)), 1, recs, env, 0, 0);
}

/* The same with black point and white point per field: the picture words from every field's own black point, and the encoder's
 * level records with their bounds beside them (crthip_bind_levels). */
int
crthip_knobs_prepare7(const crthip_params *p, int n, const crthip_knobs7 *knobs, crthip_knob_rec *recs, crthip_level_rec *levs,
                      crthip_knobs_env *env, crthip_levels_env *lenv)
{
    if (levs == 0 || lenv == 0) {
        return CRTHIP_E_ARG;
    }
    return knobs_prepare_any(p, n, knobs ? &knobs->noise : 0, (int) (sizeof(*knobs) / sizeof(int)), 1, recs, env, levs, lenv);
}

/* The same with the encoder hue per field: the first seven values exactly as crthip_knobs_prepare7 takes them (the signal range the
 * env's no-low-cascade bound comes from does not move with the hue: |burst| <= 32, so the burst samples stay inside sync level ..
 * white level), and hues[k] = the carrier tables crthip_params_finalize derives for field k's hue (crthip_bind_hues).  What that
 * function would refuse for a field is refused here: the PPU encoder, which has no per-field instantiation, and -- checked, although
 * sn >> 10 cannot give it -- a carrier outside the 24-bit encoder's bound (encoder_fast_ok, crt_encode.hip). */
int
crthip_knobs_prepare8(const crthip_params *p, int n, const crthip_knobs8 *knobs, crthip_knob_rec *recs, crthip_level_rec *levs,
                      crthip_hue_rec *hues, crthip_knobs_env *env, crthip_levels_env *lenv, crthip_hues_env *henv)
{
    struct crt_sysdef d;
    int k, r, i, rc;

    if (levs == 0 || lenv == 0 || hues == 0 || henv == 0) {
        return CRTHIP_E_ARG;
    }
    rc = knobs_prepare_any(p, n, knobs ? &knobs->noise : 0, (int) (sizeof(*knobs) / sizeof(int)), 1, recs, env, levs, lenv);
    if (rc != CRTHIP_OK) {
        return rc;
    }
    if (crt_sysdef_get(&d, p->system, p->chroma_pattern) != CRTHIP_OK || d.ppu_input) {
        return CRTHIP_E_ARG;
    }
    for (k = 0; k < n; k++) {
        if (knobs[k].hue > CRTHIP_HUE_ABS_MAX || knobs[k].hue < -CRTHIP_HUE_ABS_MAX) {
            return CRTHIP_E_ARG;                                    /* (angle * 8192 must stay an int) */
        }
        memset(&hues[k], 0, sizeof(hues[k]));
        rgb_carriers(&d, p->chroma_pattern, p->as_color, knobs[k].hue, hues[k].burst, hues[k].modI, hues[k].modQ);
        for (r = 0; r < CRTHIP_CARRIER_ROWS; r++) {
            for (i = 0; i < CRTHIP_MAX_CCS; i++) {
                if (hues[k].modI[r][i] <= -2048 || hues[k].modI[r][i] >= 2048 || hues[k].modQ[r][i] <= -2048 || hues[k].modQ[r][i] >= 2048) {
                    return CRTHIP_E_ARG;
                }
            }
        }
    }
    memset(henv, 0, sizeof(*henv));
    henv->magic = CRTHIP_HUES_MAGIC;
    henv->n = n;
    return CRTHIP_OK;
}

/* ------------------------------------------------------------------------- */
/* mixed image sizes (crthip_fieldpass_sizes, crthip_stills_sizes)             */
/* ------------------------------------------------------------------------- */
/*
 * The per-field size records and their bounds.  Field by field a copy of p with the field's w and h goes through
 * crthip_params_finalize -- its refusals are this call's, its col_step the record's -- and must leave the signal geometry and
 * the layout verdict of p itself where they are: that is what lets ONE launch sequence serve every size.  Offsets and the extent
 * are byte counts in size_t (the ABI's own 64-bit type; the records carry them as two words).
 */
int
crthip_sizes_prepare(const crthip_params *p, int n, const crthip_size *sizes, crthip_size_rec *recs, crthip_sizes_env *env)
{
    struct crt_sysdef d;
    int k, shape, lay0[3][4], verdict0[3];
    size_t fs0[3], extent = 0;
    const size_t size_max = ~(size_t) 0;

    if (p == 0 || sizes == 0 || recs == 0 || env == 0 || n <= 0 || p->finalized != CRTHIP_PARAMS_MAGIC ||
        crt_sysdef_get(&d, p->system, p->chroma_pattern) != CRTHIP_OK) {
        return CRTHIP_E_ARG;
    }
    if (p->raw != 0 || d.ppu_input || p->in_bpp == 0) {
        return CRTHIP_E_ARG;
    }
    for (shape = 0; shape <= 2; shape++) {
        verdict0[shape] = crthip_signal_layout_query(p, n, shape, lay0[shape], &fs0[shape]);
        if (verdict0[shape] < 0) {
            return CRTHIP_E_ARG;
        }
    }
    memset(env, 0, sizeof(*env));
    for (k = 0; k < n; k++) {
        crthip_params q = *p;
        const size_t off = ((size_t) sizes[k].off_hi << 16 << 16) | (size_t) sizes[k].off_lo;
        size_t rows, row_bytes, bytes;
        int lay[4];
        size_t fs;

        q.w = sizes[k].w;
        q.h = sizes[k].h;
        if (crthip_params_finalize(&q) != CRTHIP_OK) {
            return CRTHIP_E_ARG;
        }
        if (q.destw != p->destw || q.desth != p->desth || q.xo != p->xo || q.yo != p->yo || q.in_bpp != p->in_bpp) {
            return CRTHIP_E_ARG;
        }
        for (shape = 0; shape <= 2; shape++) {
            if (crthip_signal_layout_query(&q, n, shape, lay, &fs) != verdict0[shape] || fs != fs0[shape] ||
                memcmp(lay, lay0[shape], sizeof(lay)) != 0) {
                return CRTHIP_E_ARG;
            }
        }
        if (p->in_bpp == 4 && (off & 3) != 0) {
            return CRTHIP_E_ARG;
        }
        rows = (size_t) q.h + ((p->flags & CRTHIP_F_IMAGE_SPARE_ROW) ? 1 : 0);
        row_bytes = (size_t) q.w * (size_t) p->in_bpp;
        if (row_bytes > size_max / rows) {
            return CRTHIP_E_ARG;
        }
        bytes = rows * row_bytes;
        if (bytes > size_max - off) {
            return CRTHIP_E_ARG;
        }
        memset(&recs[k], 0, sizeof(recs[k]));
        recs[k].w = q.w;
        recs[k].h = q.h;
        recs[k].col_step_lo = q.col_step_lo;
        recs[k].col_step_hi = q.col_step_hi;
        recs[k].off_lo = sizes[k].off_lo;
        recs[k].off_hi = sizes[k].off_hi;
        if (k == 0 || q.w < env->w_min) {
            env->w_min = q.w;
        }
        if (k == 0 || q.w > env->w_max) {
            env->w_max = q.w;
        }
        if (k == 0 || q.h < env->h_min) {
            env->h_min = q.h;
        }
        if (k == 0 || q.h > env->h_max) {
            env->h_max = q.h;
        }
        if (off + bytes > extent) {
            extent = off + bytes;
        }
    }
    env->magic = CRTHIP_SIZES_MAGIC;
    env->n = n;
    env->extent_lo = (unsigned) (extent & 0xffffffffu);
    env->extent_hi = (unsigned) (extent >> 16 >> 16);
    return CRTHIP_OK;
}

/*
 * Host half of the decoder envelopes: the lowest decoder tier that is exact for this luma offset and contrast.
 *   3: beyond the 24-bit envelope of the fast decoder (|bright| > FAST_BRIGHT_MAX, |contrast| >= 2^23)
 *   2: beyond the 64-bit-mad tiers -- they need the luma coefficients in [2^15, 1.5 * 2^16), the chroma ones below 2^15, no luma
 *      stage product that wraps in the reference, |bright| <= T0_BRIGHT_MAX, and a contrast product that does not wrap either
 *   0: everything else
 */
int
crt_setup_decoder_floor(const crthip_params *p, int bright, int contrast)
{
    const long b = bright < 0 ? -(long) bright : (long) bright;
    const long ct = contrast < 0 ? -(long) contrast : (long) contrast;
    int coef_ok, cas, k;
    long vmax;

    if (b > FAST_BRIGHT_MAX || ct >= (1L << 23)) {
        return 3;
    }
    /* the 64-bit-mad tiers: luma coefficients near 2^16 (the form x' = hi32(((c - 2^16) << 16) * d + {2^31, u})), chroma ones
     * below 2^15 */
    coef_ok = p->eq_lf[0] >= 32768 && p->eq_lf[0] < 98304 && p->eq_hf[0] >= 32768 && p->eq_hf[0] < 98304 &&
              p->eq_lf[1] > 0 && p->eq_lf[1] < 32768 && p->eq_hf[1] > 0 && p->eq_hf[1] < 32768 &&
              p->eq_lf[2] > 0 && p->eq_lf[2] < 32768 && p->eq_hf[2] > 0 && p->eq_hf[2] < 32768;
    /* ... and no luma stage may wrap in the reference: stage k of a cascade with alpha = c / 2^16 obeys
     * |x_k| <= (alpha |x_(k-1)| + 1) / (1 - |1 - alpha|), its product is c * (x_(k-1) - x_k) */
    for (cas = 0; cas < 2 && coef_ok; cas++) {
        const double cf = cas ? p->eq_hf[0] : p->eq_lf[0], al = cf / 65536.0, den = 1.0 - (al > 1.0 ? al - 1.0 : 1.0 - al);
        double prev = 127.0 + (double) b, worst = 0.0;
        for (k = 0; k < 4; k++) {
            const double cur = (al * prev + 1.0) / den + 1.0;
            if (prev + cur > worst) worst = prev + cur;
            prev = cur;
        }
        if (cf * worst + 32768.0 >= 2147483647.0) coef_ok = 0;
    }
    if (!coef_ok || b > T0_BRIGHT_MAX) {
        return 2;
    }
    /* ... and ((v >> 12) * contrast) >> 8 must not wrap in the reference, because tiers 0 / 1 take it from an exact 64-bit
     * product (D9): |luma| <= 10 U + 64 with U = 127 + |bright| (both luma gain sets), |chroma| <= 3870,
     * |v| <= 4 * 4095 * |luma| + (4530 + 7021) * |chroma| */
    vmax = 16380L * (10L * (127 + b) + 64) + 11551L * 3870L;
    if (((vmax >> 12) + 1) * ct >= (1L << 31)) {
        return 2;
    }
    return 0;
}

/* ------------------------------------------------------------------------- */
/* VHS: the C library's rand() (crt_core.c:344,349-351; crt_ntscvhs.c:206)    */
/* ------------------------------------------------------------------------- */
/*
 * The reference's VHS noise is whatever the process's rand() returns; on the platform the reference
 * is built for (glibc) that is random()'s TYPE_3 additive feedback generator:
 *     y[n] = y[n-31] + y[n-3]  (mod 2^32),   rand() = y[n] >> 1
 * seeded by srand(seed): y[0] = seed, y[i] = 16807*y[i-1] mod (2^31-1) for i < 31, y[31..33] =
 * y[0..2], and the first 310 outputs discarded.  A generator state is handed to the kernels as its
 * "history": the 31 values y[n-31 .. n-1] that precede the next output.
 */
int
crthip_vhs_history_from_seed(unsigned seed, unsigned hist[31])
{
    unsigned y[34 + 310 + 31];
    int i;
    long word;

    if (hist == 0) {
        return CRTHIP_E_ARG;
    }
    if (seed == 0) {
        seed = 1;
    }
    y[0] = seed;
    word = (long) (int) seed;
    for (i = 1; i < 31; i++) {
        /* Schrage: 16807 * word mod 2147483647 without overflow (glibc srandom_r) */
        long hi = word / 127773;
        long lo = word % 127773;
        word = 16807 * lo - 2836 * hi;
        if (word < 0) {
            word += 2147483647;
        }
        y[i] = (unsigned) word;
    }
    for (i = 31; i < 34; i++) {
        y[i] = y[i - 31];
    }
    for (i = 34; i < 34 + 310; i++) {
        y[i] = y[i - 31] + y[i - 3];
    }
    /* the next output is y[344]; its history is y[313 .. 343] */
    for (i = 0; i < 31; i++) {
        hist[i] = y[313 + i];
    }
    return CRTHIP_OK;
}

/* coefficients of x^k modulo x^31 - x^28 - 1 over Z/2^32: y[a+k] = sum_m c[m] * y[a+m] */
static void
poly_mul_mod(const unsigned *a, const unsigned *b, unsigned *out)
{
    unsigned t[61];
    int i, j;

    for (i = 0; i < 61; i++) {
        t[i] = 0;
    }
    for (i = 0; i < 31; i++) {
        if (a[i] == 0) {
            continue;
        }
        for (j = 0; j < 31; j++) {
            t[i + j] += a[i] * b[j];
        }
    }
    for (i = 60; i >= 31; i--) {       /* x^i = x^(i-3) + x^(i-31) */
        t[i - 3] += t[i];
        t[i - 31] += t[i];
    }
    for (i = 0; i < 31; i++) {
        out[i] = t[i];
    }
}

void
crt_setup_vhs_power(unsigned long k, unsigned c[31])
{
    unsigned base[31], acc[31], tmp[31];
    int i;

    for (i = 0; i < 31; i++) {
        base[i] = 0;
        acc[i] = 0;
    }
    base[1] = 1;    /* x   */
    acc[0] = 1;     /* 1   */
    while (k) {
        if (k & 1ul) {
            poly_mul_mod(acc, base, tmp);
            memcpy(acc, tmp, sizeof(acc));
        }
        poly_mul_mod(base, base, tmp);
        memcpy(base, tmp, sizeof(base));
        k >>= 1;
    }
    memcpy(c, acc, sizeof(acc));
}

/* rows[q] = coefficients of x^(first + q*step), q = 0 .. count-1 */
void
crt_setup_vhs_power_table(unsigned long first, unsigned long step, int count, unsigned *rows)
{
    unsigned stepc[31];
    int q;

    crt_setup_vhs_power(step, stepc);
    crt_setup_vhs_power(first, rows);
    for (q = 1; q < count; q++) {
        poly_mul_mod(rows + 31 * (q - 1), stepc, rows + 31 * q);
    }
}

/*
 * The float form of the decoder's filter stages (crt_hip.h): per cascade the rounding pair (a, n), the bias
 * schedule and the proof that nothing leaves the binade [2^23, 2^24) over `steps` samples.
 *   states:  |x_j| <= M_j.  0 < alpha = c / 2^16 <= 1: a stage output lies between its state and its input (round-to-nearest of
 *            alpha * d never exceeds the integer |d|), M_j = M_in.  alpha > 1 overshoots: x' = (1 - alpha) x + alpha u + r,
 *            |r| <= 1/2, so M_j = (alpha M_(j-1) + 1) / (1 - |1 - alpha|) + 1 (the bound decoder_min_tier uses).
 *   inputs:  luma |s + bright| <= 128 + |bright|; chroma |(s * wave) >> 9| <= 128 * 120000 / 512 + 1 (tiers 0 / 1).
 *   biases are linear in the sample index, so the extremes are at the line's two ends.
 */
#define FSTAGE_WAVE_MAX 120000L                     /* T0_WAVE_MAX, crt_dev.h */
static int
fstage_bits(double v)
{
    return (int) (0x4B000000L + (long) (v - 8388608.0));
}

int
crthip_float_stages_query(const crthip_params *p, int steps, crthip_fstages *out)
{
    struct crt_sysdef d;
    int k, j, t, ok = 1;
    long b;

    if (!p || !out || p->finalized != CRTHIP_PARAMS_MAGIC || steps < 0 ||
        crt_sysdef_get(&d, p->system, p->chroma_pattern) != CRTHIP_OK) {
        return CRTHIP_E_ARG;
    }
    memset(out, 0, sizeof *out);
    if (steps == 0) steps = d.av_len + 1;
    out->steps = steps;
    b = p->bright < 0 ? -(long) p->bright : (long) p->bright;
    if (b > 130000L) ok = 0;                        /* FAST_BRIGHT_MAX: beyond it no fast tier runs at all */
    for (k = 0; k < 4; k++) {
        crthip_fstage_cascade *q = &out->cas[k];
        int c = k == 0 ? p->eq_lf[0] : k == 1 ? p->eq_hf[0] : k == 2 ? p->eq_hf[1] : p->eq_hf[2];
        int ce, odd, sh = 0, cas_ok = 1;
        double m_in, m, lo, hi, x0, span;
        float mul;

        q->c = c;
        q->form = k < 2;
        if (q->form ? (c < 32768 || c >= 98304) : (c <= 0 || c >= 32768)) cas_ok = 0;
        ce = q->form ? c - 65536 : c;
        q->ce = ce;
        if (ce == 0) cas_ok = 0;                    /* alpha = 1 exactly: no odd part */
        if (!cas_ok) {
            ok = 0;
            continue;
        }
        odd = ce < 0 ? -ce : ce;
        while (!(odd & 1)) {
            odd >>= 1;
            sh++;
        }                                           /* |ce| <= 2^15: sh <= 15 */
        q->a = ce < 0 ? -(1 << (15 - sh)) : 1 << (15 - sh);
        q->n = (odd - 1) / 2;
        q->drift = q->form ? q->n + q->a : q->n;
        q->dstage = q->form ? q->n : q->n - q->a;
        mul = (float) ce / 65536.0f;                /* exact: |ce| < 2^24, a power-of-two divisor */
        memcpy(&q->mul_bits, &mul, sizeof q->mul_bits);
        m_in = k < 2 ? 128.0 + (double) b : (double) (128L * FSTAGE_WAVE_MAX / 512L + 1L);
        q->in_max = (int) m_in;
        /* range of input and states relative to the bias of stage 0 at sample 0 */
        lo = hi = 0.0;
        for (t = 0; t < 2; t++) {
            const double at = (double) q->drift * (t ? (double) steps : 0.0);
            if (at + q->a - m_in < lo) lo = at + q->a - m_in;
            if (at + q->a + m_in > hi) hi = at + q->a + m_in;
        }
        m = m_in;
        for (j = 0; j < 4; j++) {
            const double al = (double) c / 65536.0;
            if (al > 1.0) m = (al * m + 1.0) / (1.0 - (al - 1.0)) + 1.0;
            for (t = 0; t < 2; t++) {
                const double at = (double) q->drift * (t ? (double) steps : 0.0) + (double) q->dstage * j;
                if (at - m < lo) lo = at - m;
                if (at + m > hi) hi = at + m;
            }
        }
        q->state_max = m < 2147483647.0 ? (int) m + 1 : 2147483647;
        lo = (double) (long) lo - 1.0;              /* whole numbers, outwards (the overshoot bound is no integer) */
        hi = (double) (long) hi + 1.0;
        span = hi - lo;
        if (span > 8388608.0 - 4.0) {
            ok = 0;
            continue;
        }
        x0 = 8388608.0 + (double) (long) ((8388608.0 - span) / 2.0) - lo;      /* centred in the binade */
        q->lo = (int) (x0 + lo);
        q->hi = (int) (x0 + hi);
        q->x0_bits = fstage_bits(x0);
        q->in0_bits = fstage_bits(x0 + q->a);
        q->out0_bits = fstage_bits(x0 + 3.0 * q->dstage + q->drift);
    }
    out->ranges_ok = ok;
    if (d.cc_samples != 4) ok = 0;                  /* k_decode's float loop is the 4-sample one */
    out->ok = ok;
    return ok;
}

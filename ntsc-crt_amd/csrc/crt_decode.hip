/* crt_decode.hip -- host side of the lane-per-scanline decoder (kernel: crt_decode_lane.h).  See crt_dev.h. */
#include "crt_decode_lane.h"

/* host half of the decoder envelopes: the batch-wide floor of the decoder tier -- what the brightness and the contrast ask
 * for (crt_setup_decoder_floor, crt_setup.c: the one definition, shared with the per-field floors of crthip_knobs_prepare5), raised by
 * the context's switches.  A call with picture knobs starts from the smallest floor among its fields instead: the sync kernel has
 * ORed every field's own floor into its lines' tier flags. */
int crt_decoder_min_tier(const crthip_ctx *c, const crthip_params *p)
{
    const int fl = c->call.pic ? c->call.floor_lo : crt_setup_decoder_floor(p, p->bright, p->contrast);
    if (c->force_exact || fl >= 3) return 3;
    if (c->no_tier0 || c->no_loskip) return 2;  /* crthip_set_exact(2) / (3): keep the I/Q low cascades = the 24-bit tier */
    return fl;
}
static int decoder_min_tier(const crthip_ctx *c, const crthip_params *p) { return crt_decoder_min_tier(c, p); }

/* Float filter stages for tier group 0 (crt_decode_lane.h, eq_stepf_yiq)?  Yes where the switch is on (CRTHIP_DEC_FLOAT, default),
 * the system has 4 samples per chroma cycle (the PV-1000's 1 487-sample lines stay on the integer stages) and the host's proof holds
 * for these coefficients, this brightness and the system's line length (crthip_float_stages_query, crt_setup.c); *fs = the kernel's
 * constants then.  Any no: the integer stages, as before. */
bool crt_decode_fstages(crthip_ctx *c, const crthip_params *p, int min_tier, FStageArgs *fs)
{
    memset(fs, 0, sizeof *fs);
    c->last_fstage = 0;
    /* picture knobs: the integer stages (the binade proof below is for ONE |bright|) */
    if (!c->dec_float || min_tier > 1 || c->call.pic) return false;
    crthip_fstages q;
    if (crthip_float_stages_query(p, 0, &q) != 1) return false;
    for (int k = 0; k < 4; k++) {
        fs->mul[k] = q.cas[k].mul_bits; fs->x0[k] = q.cas[k].x0_bits; fs->dstage[k] = q.cas[k].dstage;
        fs->in0[k] = q.cas[k].in0_bits; fs->out0[k] = q.cas[k].out0_bits; fs->drift[k] = q.cas[k].drift;
    }
    c->last_fstage = 1;
    return true;
}

/* what the decoder refuses, whatever the fields hold: checked by crt_run_decode before it launches anything, and by crthip_stills
 * before its first pass (a refused call must not have run the passes in front of its first decoder) */
int crt_decode_check(crthip_ctx *c, const crthip_params *p)
{
    if (p->dx <= 0)     /* more than 4096 output pixels per sample: the resampler's step (crt_core.c:528) rounds to 0 */
        return set_err(c, CRTHIP_E_ARG, "outw too large for the 12-bit resampler (dx == 0)", hipSuccess);
    /* kernel shape (crthip_set_shape): the FIR build only exists in the lane-per-scanline shape; a bloom build has a
     * per-scanline resampler geometry, which the scanline-parallel shape takes as it comes and the lane-per-scanline shape
     * after sorting the lines by their width (crt_decode3.hip) */
    if (c->sd.cc_samples != 4 && p->eq_kernel)
        return set_err(c, CRTHIP_E_ARG, "the FIR decoder (USE_CONVOLUTION build) is not available for the 5-sample system", hipSuccess);
    {
        /* k_decode has the band gains of crt_core.c:272-286 compiled in */
        const int five = c->sd.cc_samples == 5;
        const int want[3][3] = { { 65536, five ? 12192 : 8192, five ? 7775 : 9175 }, { 65536, 65536, 1311 }, { 65536, 65536, 0 } };
        for (int k = 0; k < 3; k++)
            for (int b = 0; b < 3; b++)
                if (p->eq_g[k][b] != want[k][b])
                    return set_err(c, CRTHIP_E_ARG, "equaliser gains differ from crt_core.c:272-286", hipSuccess);
    }
    return CRTHIP_OK;
}

int crt_run_decode(crthip_ctx *c, const crthip_params *p, int n, const signed char *d_inp,
                   const crthip_line *d_lines, void *d_out, size_t ostride, size_t fstride)
{
    /* fstride: bytes between the fields of d_inp -- the flat layout's (0) or the padded one's of the fused path (crt_dev.h, sig_layout);
     * crthip_line.pos is an offset into the field either way, the kernels do not know the difference */
    if (!fstride) fstride = c->fstride;
    c->last_fstage = 0;
    {
        const int rc = crt_decode_check(c, p);
        if (rc) return rc;
    }
    /* ... and a WIDE picture leaves the scanline-parallel shape early: from WIDE_SHAPE_MIN_FIELDS fields on the wide-run decoder
     * (crt_decode4.hip: 16 scanlines per wave, so 32 fields are already two waves per CU) is the faster one -- 1080p x 64: 0.178 ->
     * 0.135 ms, x 128: 0.359 -> 0.191, x 32: 0.126 / 0.130, x 16: 0.114 / 0.126 (profiles/r04_experiments.txt, section 15) */
    const bool wide_px = c->px_tile ? c->px_tile >= 32 : p->outw >= 1280;
    const bool rows_shape = !p->eq_kernel && (c->shape == 2 || (c->shape == 0 && n <= ROWS_SHAPE_MAX_FIELDS &&
                            !(n >= WIDE_SHAPE_MIN_FIELDS && !p->bloom && crt_decode_wide_ok(c, p, decoder_min_tier(c, p), wide_px))));
    if (rows_shape) return crt_run_decode_rows(c, p, n, d_inp, d_lines, d_out, ostride, fstride);
    /* picture knobs on the lane-per-scanline shape: the PK instantiations of k_decode (crt_decode_pk.hip; the bloom build's: crt_decode3.hip) */
    if (c->call.pic && !p->bloom) return crt_run_decode_pk(c, p, n, d_inp, d_lines, d_out, ostride, fstride, wide_px);
    if (p->bloom) return crt_run_decode_bloom_lanes(c, p, n, d_inp, d_lines, d_out, ostride, decoder_min_tier(c, p), fstride);
    /* FIR build: the filters only add, their outputs stay inside the hull of the inputs, so the 24-bit envelope
     * of tier 2 carries over (tier 4); beyond it the exact instantiation (tier 5) */
    const int min_tier = p->eq_kernel ? (decoder_min_tier(c, p) == 3 ? 5 : 4) : decoder_min_tier(c, p);
    const bool wide = wide_px;
    const bool use_wide = crt_decode_wide_ok(c, p, min_tier, wide);
    FStageArgs fsa;
    const bool fstage = crt_decode_fstages(c, p, min_tier, &fsa) && !use_wide;     /* (the wide-run decoder keeps its integer stages) */
    c->last_fstage = fstage;
    /* lines per output row when the picture is shorter than the raster: one pass per rank */
    const unsigned span = (unsigned) p->outh + p->v_fac;
    const int passes = span >= (unsigned) c->sd.lines ? 1 : (int) (((unsigned) c->sd.lines + span - 1) / (span ? span : 1));
    return dispatch_system(c->system, c->pattern, [&](auto tag) {
        using S = decltype(tag);
        {
        const int total = n * S::LINES;
        const block_order bo = make_block_order((total + 63) / 64, c->dec_order_env == -1 ? n : c->dec_order_env);
        unsigned char *o = (unsigned char *) d_out;
        ProfScope ps(c, CRTHIP_K_DECODE);
        const auto group = [&](int tg, int rank) {                /* (the uniform call's part of decode_built, crt_decode_lane.h) */
            return launch_decode<S, false, false>(c, p, n, d_inp, fstride, d_lines, o, ostride, tg, wide, fstage, fsa, min_tier, rank, nullptr, bo);
        };
        for (int rank = 0; rank < passes; rank++) {
            int rc = CRTHIP_OK;
            /* wide pictures in tiers 0 / 1: the 16-scanlines-per-wave kernel with 1 KB row runs (crt_decode4.hip); the groups
             * of the higher tiers stay with k_decode */
            if (use_wide) {
                rc = crt_run_decode_wide(c, p, n, d_inp, d_lines, d_out, ostride, min_tier, rank, fstride);
                if (rc == CRTHIP_OK) rc = group(1, rank);
            } else {
                /* one launch per tier GROUP that can be populated (0: tiers 0 / 1, 1: tiers 2 / 3, 2: the FIR tiers); waves of the
                 * other group leave at once */
                if (min_tier <= 1) rc = group(0, rank);
                if (min_tier <= 3 && rc == CRTHIP_OK) rc = group(1, rank);
                if (min_tier >= 4 && rc == CRTHIP_OK) rc = group(2, rank);
            }
            if (rc) return rc;
        }
        return CRTHIP_OK;
        }
    });
}


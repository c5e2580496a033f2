/* crt_decode_pk.hip -- the lane-per-scanline decoder for calls with PICTURE KNOBS (crthip_knobs_prepare5): the PK instantiations
 * of k_decode (crt_decode_lane.h), which read brightness and contrast from the crthip_knob_rec of every scanline's field, and their
 * launch code.  A translation unit of its own so that the instantiations compile beside those of crt_decode.hip, not after them.
 *
 * What differs from crt_run_decode's launches (crt_decode.hip), which this mirrors:
 *   - min_tier starts from the smallest tier floor among the call's fields (crt_decoder_min_tier); the fields above it were flagged line
 *     by line by k_hsync_wave<KN = 2>, so a field at contrast 40 000 sends its own wavefronts to tier group 1 and nobody else's;
 *   - the integer filter stages only (crt_decode_fstages says no for such a call);
 *   - the 4-sample systems only: the PV-1000 is refused by every knob entry point before anything is launched.
 * The wide-run decoder takes its tiers 0 / 1 as in the uniform call (crt_decode4.hip has its own PK instantiation). */
#include "crt_decode_lane.h"

int crt_run_decode_pk(crthip_ctx *c, const crthip_params *p, int n, const signed char *d_inp, const crthip_line *d_lines,
                      void *d_out, size_t ostride, size_t fstride, bool wide)
{
    const int floor_tier = crt_decoder_min_tier(c, p);
    /* FIR build: tiers 4 / 5, as in crt_run_decode */
    const int min_tier = p->eq_kernel ? (floor_tier == 3 ? 5 : 4) : floor_tier;
    const bool use_wide = crt_decode_wide_ok(c, p, min_tier, wide);
    c->last_fstage = 0;
    const unsigned span = (unsigned) p->outh + p->v_fac;
    const int passes = span >= (unsigned) c->sd.lines ? 1 : (int) (((unsigned) c->sd.lines + span - 1) / (span ? span : 1));
    return dispatch_system(c->system, c->pattern, [&](auto tag) {
        using S = decltype(tag);
        if constexpr (S::CCS != 4) {
            return set_err(c, CRTHIP_E_ARG, "knobs: the 5-sample decoder (PV-1000) takes its knobs from the uniform parameters", hipSuccess);
        } else {
            const int total = n * S::LINES;
            const block_order bo = make_block_order((total + 63) / 64, c->dec_order_env == -1 ? n : c->dec_order_env);
            unsigned char *o = (unsigned char *) d_out;
            const FStageArgs fsa = {};
            ProfScope ps(c, CRTHIP_K_DECODE);
            const auto group = [&](int tg, int rank) {            /* (the PK part of decode_built, crt_decode_lane.h) */
                return launch_decode<S, false, true>(c, p, n, d_inp, fstride, d_lines, o, ostride, tg, wide, false, fsa, min_tier, rank, nullptr, bo);
            };
            for (int rank = 0; rank < passes; rank++) {
                int rc = CRTHIP_OK;
                if (use_wide) {
                    rc = crt_run_decode_wide(c, p, n, d_inp, d_lines, d_out, ostride, min_tier, rank, fstride);
                    if (rc == CRTHIP_OK) rc = group(1, rank);
                } else {
                    /* one launch per tier group that can be populated, as in crt_run_decode */
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

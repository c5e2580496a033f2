/* crt_host.hip -- context, the crthip_* C ABI (include/crt_hip.h), sequence mode.  See crt_dev.h. */
#include "crt_dev.h"

#include <type_traits>

/* ------------------------------------------------------------------------- */
/* Sequence mode: n consecutive fields of ONE television set  */
/* ------------------------------------------------------------------------- */
/* Sequential semantics of   for k: crt_modulate(field k); crt_demodulate(); save(out)   (the loop of
 * extra/video_convert.c:246-277) reproduced with parallel kernels:
 *   rn      : closed form, rn_k = J^k(rn_0), J = INPUT_SIZE steps of the LCG;
 *   encoder : independent per field (fused, writes the noisy field);
 *   sync    : field k starts from field k-1's final (hsync, vsync).  Solved as a fixed point: every
 *             pass runs k_hsync_wave for ALL fields in parallel with init_k = final_{k-1} of the
 *             previous pass; after pass j fields 0..j-1 are final for good, and because a field's final
 *             state hardly ever depends on its initial one the iteration normally stops after 2-3 passes;
 *   decoder : independent per field given its line table (blend must be 0: with blend the output is a
 *             recurrence over fields);
 *   weave   : output image k = the single output buffer after field k: rows field k does not write come
 *             from the latest earlier field that wrote them (or the initial buffer). */
/* (m, a) = J^e by square and multiply, J = whole_field: rn -> m * rn + a is e whole fields of the LCG */
__device__ __forceinline__ uint2 lcg_pow(uint2 whole_field, unsigned e)
{
    unsigned pm = whole_field.x, pa = whole_field.y, m = 1u, a = 0u;
    for (; e; e >>= 1) {
        if (e & 1u) { m = pm * m; a = pm * a + pa; }
        pa = pm * pa + pa;
        pm = pm * pm;
    }
    return make_uint2(m, a);
}

/* state[k].rn = J^(first_index + k)(rn0): the set's generator before field first_index + k of the video, rn0 = before
 * field 0 (a shard of a longer video starts at first_index > 0) */
__global__ void k_seq_rn(int n_fields, crthip_state *state, uint2 whole_field, unsigned first_index, unsigned rn0)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_fields) return;
    const uint2 j = lcg_pow(whole_field, first_index + (unsigned) k);
    state[k].rn = (int) (j.x * rn0 + j.y);
}

/* init_k = (k ? guess[k-1] : first); also remembers nothing else */
__global__ void k_seq_load(int n_fields, crthip_state *state, const int2 *guess, int2 first)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_fields) return;
    const int2 v = k ? guess[k - 1] : first;
    state[k].hsync = v.x;
    state[k].vsync = v.y;
}

/* guess <- finals; *changed |= any difference */
__global__ void k_seq_compare(int n_fields, const crthip_state *state, int2 *guess, int *changed)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_fields) return;
    const int2 f = make_int2(state[k].hsync, state[k].vsync);
    const int2 g = guess[k];
    if (f.x != g.x || f.y != g.y) {
        guess[k] = f;
        atomicOr(changed, 1);
    }
}

/* rows written by field k (crt_core.c:552,661-664) -> owner[k][row] = 1 */
__global__ void k_seq_rows(int n_fields, int lines_per_field, int outh, const crthip_line *lines, unsigned char *owner)
{
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_fields * lines_per_field) return;
    const int k = gid / lines_per_field;
    const crthip_line lp = lines[gid];
    const int nrows = lp.nrows & CRTHIP_LINE_NROWS_MASK;
    for (int r = 0; r < nrows; r++) {
        if (lp.beg + r < outh) owner[(size_t) k * outh + lp.beg + r] = 1;
    }
}

/* latest[k][r] for the fields [range[0], range[1]) of one set = the last field of the set, <= k, that wrote row r (an absolute field
 * index), -1 = none: serial in k, one lane per (set, row).  The range is read where it lies: k_seq_latest's is in registers, a set
 * table in memory is read again every field (the compiler cannot know that `latest` does not overlap it). */
__device__ __forceinline__ void latest_column(const int *range, int r, int outh, const unsigned char *owner, int *latest)
{
    int last = -1;
    for (int k = range[0]; k < range[1]; k++) {
        if (owner[(size_t) k * outh + r]) last = k;
        latest[(size_t) k * outh + r] = last;
    }
}

__global__ void k_seq_latest(int n_fields, int outh, const unsigned char *owner, int *latest)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= outh) return;
    const int range[2] = { 0, n_fields };
    latest_column(range, r, outh, owner, latest);
}

/* Display modes (CRTHIP_F_PHOSPHOR_FADE / _CLEAR, crt_hip.h): what happens to the output buffer before every field.  KEEP = carried
 * over unchanged (extra/video_convert.c), FADE = crt_main.c:438-451, CLEAR = crt_main.c:462. */
enum { PH_KEEP = 0, PH_FADE = 1, PH_CLEAR = 2 };

/* fade of four bytes at once, crt_main.c:446-450: per byte (c>>1) + (c>>2) + (c>>3) + (c>>4) <= 236, so no term carries into the
 * next byte.  The caller clears the alpha byte of the 4-byte formats (alpha_mask). */
__device__ __forceinline__ unsigned phos_fade4(unsigned w)
{
    return ((w >> 1) & 0x7f7f7f7fu) + ((w >> 2) & 0x3f3f3f3fu) + ((w >> 3) & 0x1f1f1f1fu) + ((w >> 4) & 0x0f0f0f0fu);
}
__device__ __forceinline__ unsigned phos_fade1(unsigned c) { return (c >> 1) + (c >> 2) + (c >> 3) + (c >> 4); }
/* byte `o` of a row (rows start on a pixel) is the alpha byte of its pixel */
__device__ __forceinline__ bool phos_is_alpha(size_t o, unsigned alpha_mask) { return ((alpha_mask >> (8 * (o & 3))) & 0xffu) != 0; }

/* one row of the weave, by a block of 256: dst <- src (nullptr: zeros) as it looks `age` fields later.  FADE: fade^age, which is
 * uniform over the block: a loop of `age` word fades (all zeros from CRTHIP_PHOSPHOR_DEPTH on, without reading the source).
 * CLEAR: zeros, without reading the source.  16-byte strips, the last bytes of a row one by one. */
template <int PH>
__device__ __forceinline__ void weave_row(unsigned char *dst, const unsigned char *src, int age, size_t pitch, unsigned alpha_mask)
{
    if (PH == PH_CLEAR || age >= CRTHIP_PHOSPHOR_DEPTH) src = nullptr;
    for (size_t b = (size_t) threadIdx.x * 16; b < pitch; b += 256 * 16) {
        const size_t nb = pitch - b < 16 ? pitch - b : 16;
        if (nb == 16) {
            v4i v = { 0, 0, 0, 0 };
            if (src) v = load16u(src + b);
            if (PH == PH_FADE && src) {
                unsigned w0 = (unsigned) v.x, w1 = (unsigned) v.y, w2 = (unsigned) v.z, w3 = (unsigned) v.w;
                for (int a = 0; a < age; a++) { w0 = phos_fade4(w0); w1 = phos_fade4(w1); w2 = phos_fade4(w2); w3 = phos_fade4(w3); }
                v.x = (int) (w0 & ~alpha_mask); v.y = (int) (w1 & ~alpha_mask); v.z = (int) (w2 & ~alpha_mask); v.w = (int) (w3 & ~alpha_mask);
            }
            store16u(dst + b, v);
        } else {
            for (size_t c = 0; c < nb; c++) {
                unsigned x = src ? src[b + c] : 0u;
                if (PH == PH_FADE && src) {
                    for (int a = 0; a < age; a++) x = phos_fade1(x);
                    if (phos_is_alpha(b + c, alpha_mask)) x = 0;
                }
                dst[b + c] = (unsigned char) x;
            }
        }
    }
}

/* rows of image k that field k did not write <- the same row of image latest[k][row], k - latest fields old (or the initial image,
 * k + 1 fields old) */
template <int PH>
__global__ void __launch_bounds__(256)
k_seq_weave(int n_fields, int outh, size_t pitch, unsigned char *out, size_t ostride, const unsigned char *init,
            const int *latest, int patch_only, unsigned alpha_mask)
{
    const int row = blockIdx.x % outh, k = blockIdx.x / outh;
    if (k >= n_fields) return;
    const int src_k = latest[(size_t) k * outh + row];
    if (src_k == k) return;
    if (patch_only && src_k >= 0) return;       /* second visit (cross-shard chain): only the rows nobody here wrote */
    unsigned char *dst = out + (size_t) k * ostride + (size_t) row * pitch;
    const unsigned char *src = src_k >= 0 ? out + (size_t) src_k * ostride + (size_t) row * pitch
                                          : (init ? init + (size_t) row * pitch : nullptr);
    const int age = PH == PH_FADE ? (src_k >= 0 ? k - src_k : k + 1) : 0;
    weave_row<PH>(dst, src, age, pitch, alpha_mask);
}

/* (field-pass) one display step of FADE / CLEAR on every image of the batch, each its own display, before the decoder writes
 * field k into it: ALL (blend) treats every row -- the decoder then blends against the faded picture --, otherwise only the rows
 * field k does not write (beg .. beg + nrows - 1 of its line table, clipped to outh, as k_seq_rows), which the decoder leaves alone.
 * A block = PHOS_ROWS rows of one field, one wave per row at a time; the block's row ownership is a bitmap in LDS built from the
 * field's line table (no workspace: a field-pass stays allocation-free and graph-capturable). */
constexpr int PHOS_ROWS = 64;
template <int PH, bool ALL>
__global__ void __launch_bounds__(256)
k_phosphor_rows(int n_fields, int lines_per_field, int outh, int row_blocks, size_t pitch, unsigned char *out, size_t ostride,
                const crthip_line *lines, unsigned alpha_mask)
{
    __shared__ unsigned own[PHOS_ROWS / 32];
    const int k = (int) (blockIdx.x / (unsigned) row_blocks), r0 = (int) (blockIdx.x % (unsigned) row_blocks) * PHOS_ROWS;
    if (k >= n_fields) return;
    const int r1 = r0 + PHOS_ROWS < outh ? r0 + PHOS_ROWS : outh;
    if (!ALL) {
        if (threadIdx.x < PHOS_ROWS / 32) own[threadIdx.x] = 0u;
        __syncthreads();
        const crthip_line *lf = lines + (size_t) k * lines_per_field;
        for (int i = threadIdx.x; i < lines_per_field; i += 256) {
            const int beg = lf[i].beg, nr = lf[i].nrows & CRTHIP_LINE_NROWS_MASK;
            const int lo = beg > r0 ? beg : r0, hi = beg + nr < r1 ? beg + nr : r1;
            for (int r = lo; r < hi; r++) atomicOr(&own[(r - r0) >> 5], 1u << ((r - r0) & 31));
        }
        __syncthreads();
    }
    const int wave = (int) (threadIdx.x >> 6), lane = (int) (threadIdx.x & 63);
    for (int r = r0 + wave; r < r1; r += 4) {
        if (!ALL && ((own[(r - r0) >> 5] >> ((r - r0) & 31)) & 1u)) continue;
        unsigned char *dst = out + (size_t) k * ostride + (size_t) r * pitch;
        for (size_t b = (size_t) lane * 16; b < pitch; b += 64 * 16) {
            const size_t nb = pitch - b < 16 ? pitch - b : 16;
            if (nb == 16) {
                v4i v = { 0, 0, 0, 0 };
                if (PH == PH_FADE) {
                    v = load16u(dst + b);
                    v.x = (int) (phos_fade4((unsigned) v.x) & ~alpha_mask); v.y = (int) (phos_fade4((unsigned) v.y) & ~alpha_mask);
                    v.z = (int) (phos_fade4((unsigned) v.z) & ~alpha_mask); v.w = (int) (phos_fade4((unsigned) v.w) & ~alpha_mask);
                }
                store16u(dst + b, v);
            } else {
                for (size_t c = 0; c < nb; c++) {
                    unsigned x = 0u;
                    if (PH == PH_FADE && !phos_is_alpha(b + c, alpha_mask)) x = phos_fade1(dst[b + c]);
                    dst[b + c] = (unsigned char) x;
                }
            }
        }
    }
}

/* blend != 0 in sequence mode (crt_main.c:235 sets blend = 1): the picture is a recurrence over the fields,
 *     v_k = ((new_k & 0xfefeff) >> 1) + ((v_{k-1} & 0xfefeff) >> 1)        (crt_core.c:584-609)
 * on the first row of every line; the duplicated rows below it are copies of that BLENDED row (:661-664).  The fields
 * are decoded in parallel without blend (image k = new_k, duplicates included), then one pass per field, parallel
 * over the picture, folds the previous image in:  src[k][row] = the first row of the line that wrote `row` (-1: nobody
 * did, the row is carried over). */
__global__ void k_seq_rowsrc(int n_fields, int lines_per_field, int outh, const crthip_line *lines, int *rowsrc)
{
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_fields * lines_per_field) return;
    const int k = gid / lines_per_field;
    const crthip_line lp = lines[gid];
    const int nrows = lp.nrows & CRTHIP_LINE_NROWS_MASK;
    for (int r = 0; r < nrows; r++) {
        if (lp.beg + r < outh) rowsrc[(size_t) k * outh + lp.beg + r] = lp.beg;
    }
}

/* one word of that recurrence: `o` = the old word, already taken at the row the line started on (the word is one pixel of a 4-byte
 * format, or four bytes of a 3-byte one with alpha_mask 0).  FADE: the old word is faded in registers first (the picture the
 * decoder blends against is the faded one, and rows field k does not write become fade(prev)), then its alpha is cleared; CLEAR:
 * the old picture is all zeros.  A written word: every colour byte (new >> 1) + (old >> 1) -- what the 0xfefeff mask computes per
 * channel -- and alpha stays 0xff; an unwritten one passes `o` through. */
template <int PH> __device__ __forceinline__ unsigned fold_word(unsigned n, unsigned o, bool written, unsigned alpha_mask)
{
    if (PH == PH_CLEAR) o = 0u;
    if (PH == PH_FADE) o = phos_fade4(o) & ~alpha_mask;
    return written ? ((((n >> 1) & 0x7f7f7f7fu) + ((o >> 1) & 0x7f7f7f7fu)) | alpha_mask) : o;
}

/* one row of one field's step, by a block of 256: cur = image k's row, src = its rowsrc entry, prev_img = image k - 1 or the initial
 * picture (nullptr: zeros, as calloc leaves them -- also what CLEAR makes of it without reading it, so fold_word's `o = 0` and the
 * unread pointer are the same rule).  Written out by hand for one field of one set -- o = fade4(o) & ~alpha under FADE, then
 * v = src < 0 ? o : ((n >> 1) & 0x7f7f7f7f) + ((o >> 1) & 0x7f7f7f7f) | alpha -- the step is fold_word with written = (src >= 0),
 * so k_seq_blend_step and k_sets_blend_step share this body.  I = the type of the byte counter of a word, the one thing the compiler
 * does not see through: size_t (k_seq_blend_step) costs 20 registers, int (k_sets_blend_step) 18, and neither has been measured
 * against the other, so each kernel names its own. */
template <int PH, class I>
__device__ __forceinline__ void blend_row(unsigned char *cur, const unsigned char *prev_img, int row, int src, size_t pitch, unsigned alpha_mask)
{
    if (PH == PH_CLEAR) prev_img = nullptr;
    const unsigned char *old = prev_img ? prev_img + (size_t) (src < 0 ? row : src) * pitch : nullptr;
    for (size_t b = (size_t) threadIdx.x * 4; b < pitch; b += 256 * 4) {
        const I nb = pitch - b < 4 ? (I) (pitch - b) : 4;
        unsigned o = 0, n = 0;
        for (I c = 0; c < nb; c++) {
            o |= (unsigned) (old ? old[b + c] : 0) << (8 * c);
            n |= (unsigned) cur[b + c] << (8 * c);
        }
        const unsigned v = fold_word<PH>(n, o, src >= 0, alpha_mask);
        for (I c = 0; c < nb; c++) cur[b + c] = (unsigned char) (v >> (8 * c));
    }
}

template <int PH>
__global__ void __launch_bounds__(256)
k_seq_blend_step(int k, int outh, size_t pitch, unsigned char *out, size_t ostride, const unsigned char *init,
                 const int *rowsrc, unsigned alpha_mask)
{
    const int row = blockIdx.x;
    const int src = rowsrc[(size_t) k * outh + row];
    unsigned char *cur = out + (size_t) k * ostride + (size_t) row * pitch;
    blend_row<PH, size_t>(cur, k ? out + (size_t) (k - 1) * ostride : init, row, src, pitch, alpha_mask);
}

/* ------------------------------------------------------------------------- */
/* Sequence mode for MANY sets in one call (crthip_sequence_sets)               */
/* ------------------------------------------------------------------------- */
/* n_sets independent television sets, set s = the consecutive fields [set_first[s], set_first[s + 1]) of the batch.  The encoder,
 * sync and decoder kernels run over all fields as above; the small kernels around them learn where a set begins from a per-field
 * table tab[k] = (first field of k's set, index of the set).  Nothing of a set's state ever travels through the host. */

/* inc[s] = (hsync, vsync, rn) of set s before its first field, taken before anything writes the states */
__global__ void k_sets_incoming(int n_sets, const int *set_first, const crthip_state *state, int4 *inc)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_sets) return;
    const crthip_state *st = state + set_first[s];
    inc[s] = make_int4(st->hsync, st->vsync, st->rn, 0);
}

/* state[k].rn = J^(k - first)(the set's incoming rn) as k_seq_rn; guess[k] = the set's incoming pair ("nobody's sync state moves") */
__global__ void k_sets_rn(int n_fields, crthip_state *state, const int2 *tab, const int4 *inc, int2 *guess, uint2 whole_field)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_fields) return;
    const int2 t = tab[k];
    const int4 in = inc[t.y];
    const uint2 j = lcg_pow(whole_field, (unsigned) (k - t.x));
    state[k].rn = (int) (j.x * (unsigned) in.z + j.y);
    guess[k] = make_int2(in.x, in.y);
}

/* k_sets_rn without the generator, for the rand() streams of the VHS build (whose rn is the last value drawn: k_vhs_tail leaves it) */
__global__ void k_sets_guess(int n_fields, const int2 *tab, const int4 *inc, int2 *guess)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_fields) return;
    const int4 in = inc[tab[k].y];
    guess[k] = make_int2(in.x, in.y);
}

/* init_k = the set's incoming pair for the first field of a set, guess[k-1] otherwise */
__global__ void k_sets_load(int n_fields, crthip_state *state, const int2 *tab, const int4 *inc, const int2 *guess)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_fields) return;
    const int2 t = tab[k];
    int2 v;
    if (k == t.x) { const int4 in = inc[t.y]; v = make_int2(in.x, in.y); }
    else v = guess[k - 1];
    state[k].hsync = v.x;
    state[k].vsync = v.y;
}

/* k_seq_latest per set: one lane per (set, row) */
__global__ void k_sets_latest(int n_sets, int outh, const int *set_first, const unsigned char *owner, int *latest)
{
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_sets * outh) return;
    const int s = gid / outh;
    latest_column(set_first + s, gid - s * outh, outh, owner, latest);
}

/* k_seq_weave with the set boundary: the initial picture is the one of the field's own set, and it is k - first + 1 fields old */
template <int PH>
__global__ void __launch_bounds__(256)
k_sets_weave(int n_fields, int outh, size_t pitch, unsigned char *out, size_t ostride, const unsigned char *init, size_t init_stride,
             const int2 *tab, const int *latest, unsigned alpha_mask)
{
    const int row = blockIdx.x % outh, k = blockIdx.x / outh;
    if (k >= n_fields) return;
    const int src_k = latest[(size_t) k * outh + row];
    if (src_k == k) return;
    const int2 t = tab[k];
    unsigned char *dst = out + (size_t) k * ostride + (size_t) row * pitch;
    const unsigned char *src = src_k >= 0 ? out + (size_t) src_k * ostride + (size_t) row * pitch
                                          : (init ? init + (size_t) t.y * init_stride + (size_t) row * pitch : nullptr);
    const int age = PH == PH_FADE ? (src_k >= 0 ? k - src_k : k - t.x + 1) : 0;
    weave_row<PH>(dst, src, age, pitch, alpha_mask);
}

/* 16 bytes of a row, or the nb < 16 that are left of it (zero filled) */
__device__ __forceinline__ v4i strip_load(const unsigned char *p, int nb)
{
    if (nb == 16) return load16u(p);
    unsigned w[4] = { 0u, 0u, 0u, 0u };
    for (int c = 0; c < nb; c++) w[c >> 2] |= (unsigned) p[c] << (8 * (c & 3));
    v4i v = { (int) w[0], (int) w[1], (int) w[2], (int) w[3] };
    return v;
}
__device__ __forceinline__ void strip_store(unsigned char *p, v4i v, int nb)
{
    if (nb == 16) { store16u(p, v); return; }
    const unsigned w[4] = { (unsigned) v.x, (unsigned) v.y, (unsigned) v.z, (unsigned) v.w };
    for (int c = 0; c < nb; c++) p[c] = (unsigned char) (w[c >> 2] >> (8 * (c & 3)));
}
/* blend != 0 for all sets in ONE launch.  The recurrence v_k[row] = src < 0 ? f(v_{k-1}[row]) : blend(new_k[row], f(v_{k-1}[src]))
 * takes the old value at row src = the first row of the line that wrote `row`, so with duplicated rows a row's chain crosses into
 * other rows from field to field: rows are not independent -- but byte columns are.  A workgroup owns one set x one strip of 16
 * bytes of the row (4 pixels of the 4-byte formats; the rows start on a pixel and the strip on a multiple of 4 bytes, so every word
 * is a pixel and takes alpha_mask; RGB / BGR have mask 0 and the fold is bytewise) over ALL rows, keeps that strip of v_{k-1} in
 * LDS (two buffers of 16 B x outh, so one barrier per field) and walks its set's fields in order: every image is read once and
 * written once, and what the workgroup has just stored is never read back through the vector cache.  Work items are dealt so that
 * the eight strips of a 128-byte line go to workgroups of the same XCD (block_item, crt_dev.h). */
template <int PH>
__global__ void __launch_bounds__(256)
k_sets_fold(int n_items, int order_k, int order_per, int strips, int outh, size_t pitch, unsigned char *out, size_t ostride,
            const unsigned char *init, size_t init_stride, const int *set_first, const int *rowsrc, unsigned alpha_mask)
{
    extern __shared__ v4i fold_lds[];                  /* [2][outh] */
    const int item = block_item(blockIdx.x, order_k, order_per);
    if (item >= n_items) return;
    const int s = item / strips;
    const size_t b = (size_t) (item - s * strips) * 16;
    const int nb = pitch - b < 16 ? (int) (pitch - b) : 16;
    const int k0 = set_first[s], k1 = set_first[s + 1];
    for (int r = threadIdx.x; r < outh; r += 256) {
        v4i v = { 0, 0, 0, 0 };
        if (init && PH != PH_CLEAR) v = strip_load(init + (size_t) s * init_stride + (size_t) r * pitch + b, nb);
        fold_lds[r] = v;
    }
    __syncthreads();
    int cur = 0;
    for (int k = k0; k < k1; k++) {
        unsigned char *img = out + (size_t) k * ostride + b;
        const int *src_k = rowsrc + (size_t) k * outh;
        const v4i *old = fold_lds + (size_t) cur * outh;
        v4i *nxt = fold_lds + (size_t) (cur ^ 1) * outh;
        for (int r = threadIdx.x; r < outh; r += 256) {
            const int src = src_k[r];
            const bool written = src >= 0;
            v4i n = { 0, 0, 0, 0 };
            if (written) n = strip_load(img + (size_t) r * pitch, nb);
            const v4i o = old[written ? src : r];
            v4i v;
            v.x = (int) fold_word<PH>((unsigned) n.x, (unsigned) o.x, written, alpha_mask);
            v.y = (int) fold_word<PH>((unsigned) n.y, (unsigned) o.y, written, alpha_mask);
            v.z = (int) fold_word<PH>((unsigned) n.z, (unsigned) o.z, written, alpha_mask);
            v.w = (int) fold_word<PH>((unsigned) n.w, (unsigned) o.w, written, alpha_mask);
            strip_store(img + (size_t) r * pitch, v, nb);
            nxt[r] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
}

/* the same recurrence where the strips of a picture do not fit the LDS (pictures taller than FOLD_LDS_MAX_ROWS): field j of EVERY set
 * per launch, a block per (set, row) as k_seq_blend_step -- as many launches as the longest set has fields */
constexpr int FOLD_LDS_MAX_ROWS = 2048;                /* 2 x 16 B x 2048 rows = the 64 KB of LDS a workgroup may take */
template <int PH>
__global__ void __launch_bounds__(256)
k_sets_blend_step(int j, int outh, size_t pitch, unsigned char *out, size_t ostride, const unsigned char *init, size_t init_stride,
                  const int *set_first, const int *rowsrc, unsigned alpha_mask)
{
    const int row = blockIdx.x % outh, s = blockIdx.x / outh;
    const int k = set_first[s] + j;
    if (k >= set_first[s + 1]) return;
    const int src = rowsrc[(size_t) k * outh + row];
    unsigned char *cur = out + (size_t) k * ostride + (size_t) row * pitch;
    const unsigned char *prev_img = j ? out + (size_t) (k - 1) * ostride : (init ? init + (size_t) s * init_stride : nullptr);
    blend_row<PH, int>(cur, prev_img, row, src, pitch, alpha_mask);
}

/* ------------------------------------------------------------------------- */
/* Stills (crthip_stills): several field-passes of the same images onto the same pictures */
/* ------------------------------------------------------------------------- */
/* the encoder inputs of one pass of the schedule into every still's state, before the pass (field and frame masked as
 * crt_ntsc.c:197-198 does); `pass` arrives as a kernel argument: nothing of the schedule lives in memory */
__global__ void k_stills_pass(int n, crthip_state *state, crthip_pass pass)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    state[k].field = pass.field & 1;
    state[k].frame = pass.frame & 1;
    state[k].aux = pass.aux;
}


/* (r6) the fused path's padded signal (crt_dev.h, sig_layout) back in the reference's flat layout, 16 samples per lane: what
 * crthip_fieldpass_signal hands out (tests compare it with the oracle's inp[] byte for byte; nothing in a field-pass needs it) */
template <class S>
__global__ void __launch_bounds__(256)
k_unpad(int n_fields, const signed char *__restrict__ src, size_t sstride, int shift, signed char *__restrict__ dst, size_t dstride)
{
    constexpr int CHUNKS = (S::INPUT_SIZE + CRTHIP_TAIL + 15) / 16;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= CHUNKS) return;
    for (int f = blockIdx.y; f < n_fields; f += (int) gridDim.y)
        store16u(dst + (size_t) f * dstride + q * 16, load16u(src + (size_t) f * sstride + shift + sig_phys<S>(q * 16)));
}

int crt_run_unpad(crthip_ctx *c, int n, const sig_layout *lay, const signed char *d_src, signed char *d_dst)
{
    return dispatch_system(c->system, c->pattern, [&](auto tag) {
        using S = decltype(tag);
        if (lay->pitch == S::HRES) {
            if (hipMemcpy2DAsync(d_dst, c->fstride, d_src, lay->fstride, (size_t) S::INPUT_SIZE + CRTHIP_TAIL, (size_t) n,
                                 hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return CRTHIP_E_HIP;
            return CRTHIP_OK;
        }
        constexpr int CHUNKS = (S::INPUT_SIZE + CRTHIP_TAIL + 15) / 16;
        hipLaunchKernelGGL((k_unpad<S>), dim3((CHUNKS + 255) / 256, n < 65535 ? n : 65535), dim3(256), 0, c->stream, n, d_src, lay->fstride,
                           lay->shift, d_dst, c->fstride);
        return CRTHIP_OK;
    });
}

/* Which layout the signal of a fused field-pass takes (crt_dev.h, sig_layout): padded lines whenever the geometry allows --
 *   the row's overhang over its line (wrap = xo + destw - HRES) is at most 16 samples and ends inside the field,
 *   the row starts at or behind column PADW (what is copied behind a line is then margin, never picture), and
 *   the copies the margin kernel makes reach at least 80 columns (sync windows: 69, burst windows: 48 / 64)
 * -- and the flat layout otherwise (odd x offsets, the rand()-noise VHS build, CRT_DO_VSYNC 0, the NES, small batches,
 * crthip_set_signal_layout(ctx, 0)). */
/* (the rule without a context: crthip_signal_layout_query lets a host -- and the CPU tests -- ask it) */
static bool layout_rule(int system, int pattern, const struct crt_sysdef &sd, size_t flat_stride, const crthip_params *p, int n, int shape,
                        int sig_pad, sig_layout *lay)
{
    lay->pitch = sd.hres; lay->shift = 0; lay->padv = 0; lay->wrap = 0; lay->fstride = flat_stride;
    if (!sig_pad || system == CRTHIP_SYSTEM_NTSCVHS || (p->flags & CRTHIP_F_NO_VSYNC)) return false;
    /* ... and only where it pays (profiles/r06_ab_padded_by_system.txt, one box, padded against flat): the lane-per-row RGB encoder,
     * whose row stores it aligns -- NTSC 640x480 x 1024 +5 %, SNES +5.6 %, PV-1000 +4.5 %, bloom +5.4 % -- but not the NES's table
     * encoder (never store-bound: the margin kernel's copies cost 1.1 % and buy nothing) and not the batches the library gives to the
     * scanline-parallel encoder by itself (dword stores per lane: 640x480 x 64 -0.8 %, 1080p x 64 -3.5 %).  A FORCED scanline-parallel
     * shape keeps the padded lines (tests run k_active_row's padded stores that way). */
    if (sd.ppu_input) return false;
    if (shape == 0 && n <= ROWS_SHAPE_MAX_FIELDS_ENC) return false;
    if (p->in_bpp == 0) return false;                 /* crt_modulate refuses the format: the noise kernel writes the (flat) field */
    return dispatch_system(system, pattern, [&](auto tag) {
        using S = decltype(tag);
        using G = PadGeom<S>;
        const int over = p->xo + p->destw - S::HRES, wrap = over > 0 ? over : 0;
        if (wrap > 16 || p->xo < G::PADW || p->destw < 16 || p->yo < 0 || p->yo + p->desth + (wrap ? 1 : 0) > S::VRES) return 0;
        /* k_margin_pad copies whole 16-byte chunks: [wrap, wrap + 16 m) behind a line that carries a row, [0, 16 m') elsewhere */
        const int a = wrap + (G::PADC - wrap) / 16 * 16, b = G::PADC / 16 * 16;
        const int padv = a < b ? a : b;
        if (padv < 80) return 0;
        lay->pitch = G::PITCH;
        lay->shift = (128 - p->xo % 128) % 128;
        lay->padv = padv;
        lay->wrap = wrap;
        lay->fstride = G::FSTRIDE;
        return 1;
    }) == 1;
}

bool crt_fused_layout(const crthip_ctx *c, const crthip_params *p, int n, sig_layout *lay)
{
    return layout_rule(c->system, c->pattern, c->sd, c->fstride, p, n, c->shape, c->sig_pad, lay);
}

/* the reference's flat layout: what a field-pass falls back to, and what sequence mode always keeps (its phases are separate calls
 * over the same workspace) */
static sig_layout flat_layout(const crthip_ctx *c)
{
    sig_layout lay;
    lay.pitch = c->sd.hres; lay.shift = 0; lay.padv = 0; lay.wrap = 0; lay.fstride = c->fstride;
    return lay;
}

/* the byte the decoder writes 0xff into (crt_core.c:620-652): byte 3 of RGBA / BGRA, byte 0 of ARGB / ABGR, none for RGB / BGR */
static unsigned out_alpha_mask(const crthip_params *p)
{
    const int fmt = p->out_format;
    return p->out_bpp == 3 ? 0u : ((fmt == CRTHIP_FMT_ARGB || fmt == CRTHIP_FMT_ABGR) ? 0x000000ffu : 0xff000000u);
}

static int phosphor_mode(const crthip_params *p)
{
    return (p->flags & CRTHIP_F_PHOSPHOR_FADE) ? PH_FADE : (p->flags & CRTHIP_F_PHOSPHOR_CLEAR) ? PH_CLEAR : PH_KEEP;
}

/* f(std::integral_constant<int, PH_*>{}) for the display mode `ph`, in the idiom of dispatch_system: the one place that turns the
 * run-time mode into the kernels' template argument */
template <class F> static void dispatch_phosphor(int ph, F &&f)
{
    if (ph == PH_FADE) f(std::integral_constant<int, PH_FADE>{});
    else if (ph == PH_CLEAR) f(std::integral_constant<int, PH_CLEAR>{});
    else f(std::integral_constant<int, PH_KEEP>{});
}

/* a field-pass's display step on fields [0, n) of `out` (their line tables at `ln`), before their decoder runs: CRTHIP_F_PHOSPHOR_*,
 * displaycb's fade / clear (crt_main.c:459-463) between the sync chain and the decoder; KEEP has none */
static void launch_phosphor_rows(crthip_ctx *c, const crthip_params *p, int n, const crthip_line *ln, unsigned char *out, size_t ostride)
{
    dispatch_phosphor(phosphor_mode(p), [&](auto ph) {
        constexpr int PH = decltype(ph)::value;
        if constexpr (PH != PH_KEEP) {
            const int rb = (p->outh + PHOS_ROWS - 1) / PHOS_ROWS;
            const size_t pitch = (size_t) p->outw * p->out_bpp;
            const dim3 grid((unsigned) n * (unsigned) rb);
            dispatch_bools([&](auto blend) {
                hipLaunchKernelGGL((k_phosphor_rows<PH, blend>), grid, dim3(256), 0, c->stream, n, c->sd.lines, p->outh, rb, pitch, out, ostride, ln,
                                   out_alpha_mask(p));
            }, p->blend != 0);
        }
    });
}

/* scratch of sequence mode (seq_carve below), and the last phase of crthip_sequence_sets by display mode */
struct SetsScratch { int *set_first; int2 *tab; int4 *inc; int2 *guess; int *changed; unsigned char *owner; int *latest; };
template <int PH>
static void launch_sets_weave(crthip_ctx *c, const crthip_params *p, int n_sets, int n, int max_len, unsigned char *out, size_t ostride,
                              const unsigned char *init, size_t init_stride, const SetsScratch &sc)
{
    const int outh = p->outh;
    const size_t pitch = (size_t) p->outw * p->out_bpp;
    const unsigned alpha = out_alpha_mask(p);
    if (!p->blend) {
        hipLaunchKernelGGL((k_sets_weave<PH>), dim3((unsigned) n * (unsigned) outh), dim3(256), 0, c->stream, n, outh, pitch, out, ostride,
                           init, init_stride, sc.tab, sc.latest, alpha);
    } else if (outh <= FOLD_LDS_MAX_ROWS) {
        const int strips = (int) ((pitch + 15) / 16);
        const block_order o = make_block_order(n_sets * strips, 8);
        hipLaunchKernelGGL((k_sets_fold<PH>), dim3(o.grid), dim3(256), 2 * sizeof(v4i) * (size_t) outh, c->stream, n_sets * strips, o.K, o.per,
                           strips, outh, pitch, out, ostride, init, init_stride, sc.set_first, sc.latest, alpha);
    } else {
        for (int j = 0; j < max_len; j++)
            hipLaunchKernelGGL((k_sets_blend_step<PH>), dim3((unsigned) n_sets * (unsigned) outh), dim3(256), 0, c->stream, j, outh, pitch, out,
                               ostride, init, init_stride, sc.set_first, sc.latest, alpha);
    }
}

extern "C" {

int crthip_abi_version(void) { return CRTHIP_ABI_VERSION; }

int crthip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int crthip_create(crthip_ctx **out, int device, int system, int chroma_pattern)
{
    if (!out) return CRTHIP_E_ARG;
    *out = 0;
    struct crt_sysdef sd;
    if (crt_sysdef_get(&sd, system, chroma_pattern) != CRTHIP_OK) return CRTHIP_E_ARG;
    if (dispatch_system(system, chroma_pattern, [&](auto tag) {
            return sysdef_matches<decltype(tag)>(sd) ? CRTHIP_OK : CRTHIP_E_ARG; }) != CRTHIP_OK) {
        fprintf(stderr, "crthip: host/device system tables disagree (system %d pattern %d)\n", system, chroma_pattern);
        return CRTHIP_E_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return CRTHIP_E_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return CRTHIP_E_NODEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "crthip: device %d is %s, this library is built for gfx950 only\n", device, prop.gcnArchName);
        return CRTHIP_E_NODEVICE;
    }
    crthip_ctx *c = new (std::nothrow) crthip_ctx();
    if (!c) return CRTHIP_E_NOMEM;
    memset(c, 0, sizeof(*c));
    c->device = device; c->system = system; c->pattern = chroma_pattern; c->sd = sd;
    c->fstride = crthip_field_stride(system, chroma_pattern);
    if (hipSetDevice(device) != hipSuccess) {
        delete c;
        return CRTHIP_E_HIP;
    }
    c->stream = 0;              /* the device's default stream until crthip_set_stream() */
    c->overlap_chunks = 0;      /* automatic */
    { const char *e = getenv("CRTHIP_SYNC_KERNEL"); c->sync_kernel = e ? atoi(e) : 0; }
    { const char *e = getenv("CRTHIP_ROW_TILE"); c->row_tile = e ? atoi(e) : 0; }
    { const char *e = getenv("CRTHIP_WIDE_DECODE"); c->wide_decode = e ? atoi(e) != 0 : 1; }     /* A/B switch, crt_decode4.hip */
    { const char *e = getenv("CRTHIP_AC_TILE"); c->ac_tile_env = e && (atoi(e) == 16 || atoi(e) == 32) ? atoi(e) : 0; }   /* A/B switch, k_active */
    { const char *e = getenv("CRTHIP_WIDE_LPW"); c->wide_lpw_env = e && (atoi(e) == 8 || atoi(e) == 16) ? atoi(e) : 0; }   /* A/B switch, k_decode_wide */
    { const char *e = getenv("CRTHIP_MARGIN_SIDE"); c->margin_side = e ? atoi(e) != 0 : 1; }   /* A/B switch: k_margin beside k_active (crt_encode.hip) */
    { const char *e = getenv("CRTHIP_SIG_PAD"); c->sig_pad = e ? atoi(e) != 0 : 1; }       /* A/B switch: the fused path's signal layout (crt_dev.h, sig_layout) */
    c->fstride_pad = 0;
    dispatch_system(system, chroma_pattern, [&](auto tag) { c->fstride_pad = PadGeom<decltype(tag)>::FSTRIDE; return CRTHIP_OK; });
    { const char *e = getenv("CRTHIP_WIDE_ORDER"); c->wide_order_env = e ? atoi(e) : 0; }   /* A/B switches: workgroup order (crt_dev.h, block_item) */
    { const char *e = getenv("CRTHIP_DEC_ORDER"); c->dec_order_env = e ? atoi(e) : 0; }
    { const char *e = getenv("CRTHIP_ACT_ORDER"); c->act_order_env = e ? atoi(e) : 0; }
    { const char *e = getenv("CRTHIP_DEC_FLOAT"); c->dec_float = e ? atoi(e) != 0 : 1; c->last_fstage = 0; }   /* A/B switch: float filter stages in k_decode (crt_decode_lane.h) */
    { const char *e = getenv("CRTHIP_SIG_TILE"); c->sig_tile_env = e && (atoi(e) == 16 || atoi(e) == 32 || atoi(e) == 64) ? atoi(e) : 0; }   /* A/B switch, k_active */
    c->own_stream = false;
    /* noise LCG jump tables: state after 16*q steps, q = 0 .. INPUT_SIZE/16 */
    const int nq = sd.input_size / 16 + 2;
    uint2 *h = (uint2 *) malloc(sizeof(uint2) * (size_t) nq);
    if (!h) { crthip_destroy(c); return CRTHIP_E_NOMEM; }
    unsigned m16, a16;
    lcg_jump_host(16, &m16, &a16);
    h[0].x = 1u; h[0].y = 0u;
    for (int q = 1; q < nq; q++) { h[q].x = m16 * h[q - 1].x; h[q].y = m16 * h[q - 1].y + a16; }
    lcg_jump_host((unsigned) sd.input_size, &c->whole_field.x, &c->whole_field.y);
    if (hipMalloc((void **) &c->d_jump16, sizeof(uint2) * (size_t) nq) != hipSuccess ||
        hipMemcpy(c->d_jump16, h, sizeof(uint2) * (size_t) nq, hipMemcpyHostToDevice) != hipSuccess) {
        free(h);
        crthip_destroy(c);
        return CRTHIP_E_HIP;
    }
    free(h);
    if (system == CRTHIP_SYSTEM_NES && (hipMalloc((void **) &c->d_nes_tab, NES_TAB_SIZE) != hipSuccess ||
                                        hipMalloc((void **) &c->d_nes_tab_alt, NES_TAB_SIZE) != hipSuccess)) {
        crthip_destroy(c);
        return CRTHIP_E_NOMEM;
    }
    {
        uint2 j1[16];
        j1[0] = make_uint2(1u, 0u);
        for (int k = 1; k < 16; k++) j1[k] = make_uint2(LCG_MUL * j1[k - 1].x, LCG_MUL * j1[k - 1].y + LCG_ADD);
        if (hipMalloc((void **) &c->d_skel, (size_t) SKEL_VARIANTS * c->fstride) != hipSuccess ||
            hipMalloc((void **) &c->d_skel_alt, (size_t) SKEL_VARIANTS * c->fstride) != hipSuccess ||
            hipMalloc((void **) &c->d_jump1, sizeof(j1)) != hipSuccess ||
            hipMemcpy(c->d_jump1, j1, sizeof(j1), hipMemcpyHostToDevice) != hipSuccess) {
            crthip_destroy(c);
            return CRTHIP_E_NOMEM;
        }
    }
    if (system == CRTHIP_SYSTEM_NTSCVHS) {
        /* jump coefficients of the rand() recurrence: one row per parallel chunk, one for the first call of
         * the tail, and the tail's 64 block offsets (transposed: [m][block]) */
        const int chunks = vhs_tail_start(sd.input_size, sd.hres) / VHS_CHUNK;
        const size_t words = 31 * (size_t) (chunks + 1) + 31 * 64;
        unsigned *rows = (unsigned *) malloc(sizeof(unsigned) * words);
        if (!rows) { crthip_destroy(c); return CRTHIP_E_NOMEM; }
        crt_setup_vhs_power_table(1ul, 2ul * VHS_CHUNK, chunks, rows);
        crt_setup_vhs_power(1ul + 2ul * (unsigned long) chunks * VHS_CHUNK, rows + 31 * (size_t) chunks);
        {
            unsigned blk[31 * 64];
            unsigned *t = rows + 31 * (size_t) (chunks + 1);
            crt_setup_vhs_power_table(0ul, (unsigned long) VHS_BLK, 64, blk);
            for (int b = 0; b < 64; b++) {
                for (int m = 0; m < 31; m++) t[m * 64 + b] = blk[b * 31 + m];
            }
        }
        c->vhs_chunks = chunks;
        /* the same coefficients as SIGNED BYTE DIGITS for the matrix-core jump (crt_noise.hip, vhs_jump_mfma): a 32-bit word
         * x == d0 + d1 * 2^8 + d2 * 2^16 + d3 * 2^24 (mod 2^32), every d in [-128, 127]; per row 4 digit planes of 32 bytes
         * (coefficient m at byte m, byte 31 = 0): rows 0 .. chunks-1 the parallel chunks, then the tail's 64 blocks */
        const size_t dig_rows = (size_t) chunks + 64;
        signed char *dig = (signed char *) calloc(dig_rows, VHS_DIG_ROW);
        if (!dig) { free(rows); crthip_destroy(c); return CRTHIP_E_NOMEM; }
        for (size_t r = 0; r < dig_rows; r++) {
            for (int m = 0; m < 31; m++) {
                unsigned x = r < (size_t) chunks ? rows[r * 31 + m] : rows[31 * (size_t) (chunks + 1) + (size_t) m * 64 + (r - chunks)];
                for (int pl = 0; pl < 4; pl++) {
                    const int d = (int) (signed char) (x & 255u);
                    dig[r * VHS_DIG_ROW + pl * 32 + m] = (signed char) d;
                    x = (x - (unsigned) d) >> 8;
                }
            }
        }
        { const char *e = getenv("CRTHIP_VHS_MFMA"); c->vhs_mfma = e ? atoi(e) != 0 : 1; }       /* A/B switch: 0 = the jump on the vector unit */
        if (hipMalloc((void **) &c->d_vhs_rows, sizeof(unsigned) * words) != hipSuccess ||
            hipMemcpy(c->d_vhs_rows, rows, sizeof(unsigned) * words, hipMemcpyHostToDevice) != hipSuccess ||
            hipMalloc((void **) &c->d_vhs_dig, dig_rows * VHS_DIG_ROW) != hipSuccess ||
            hipMemcpy(c->d_vhs_dig, dig, dig_rows * VHS_DIG_ROW, hipMemcpyHostToDevice) != hipSuccess) {
            free(rows); free(dig);
            crthip_destroy(c);
            return CRTHIP_E_HIP;
        }
        free(rows); free(dig);
    }
    *out = c;
    return CRTHIP_OK;
}

void crthip_destroy(crthip_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    for (int i = 0; i < c->npend; i++) { hipEventDestroy(c->pend[i].a); hipEventDestroy(c->pend[i].b); }
    free(c->pend);
    if (c->aux_stream) {
        hipStreamSynchronize(c->aux_stream); hipStreamDestroy(c->aux_stream); hipEventDestroy(c->ev_fork); hipEventDestroy(c->ev_join);
        if (c->ev_mfork) hipEventDestroy(c->ev_mfork);
        if (c->ev_mjoin) hipEventDestroy(c->ev_mjoin);
        for (int k = 0; k < CRTHIP_MAX_CHUNKS; k++) hipEventDestroy(c->ev_chunk[k]);
    }
    if (c->d_jump16) hipFree(c->d_jump16);
    if (c->d_vhs_rows) hipFree(c->d_vhs_rows);
    if (c->d_vhs_dig) hipFree(c->d_vhs_dig);
    if (c->d_vhs_next) hipFree(c->d_vhs_next);
    if (c->d_seq) hipFree(c->d_seq);
    if (c->d_still_sig) hipFree(c->d_still_sig);
    free(c->seq_sets_host);
    if (c->d_bloom) hipFree(c->d_bloom);
    if (c->table_stream) { hipStreamSynchronize(c->table_stream); hipStreamDestroy(c->table_stream); }
    if (c->d_nes_tab) hipFree(c->d_nes_tab);
    if (c->d_nes_tab_alt) hipFree(c->d_nes_tab_alt);
    if (c->d_skel) hipFree(c->d_skel);
    if (c->d_skel_alt) hipFree(c->d_skel_alt);
    for (int i = 0; i < c->n_retired; i++) if (c->retired[i]) hipFree(c->retired[i]);
    if (c->d_jump1) hipFree(c->d_jump1);
    if (c->d_analog) hipFree(c->d_analog);
    if (c->d_inp) hipFree(c->d_inp);
    if (c->d_lines) hipFree(c->d_lines);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int crthip_set_stream(crthip_ctx *c, void *hip_stream)
{
    if (!c) return CRTHIP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = (hipStream_t) hip_stream;       /* NULL = the default stream */
    return CRTHIP_OK;
}

int crthip_synchronize(crthip_ctx *c)
{
    if (!c) return CRTHIP_E_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CRTHIP_OK;
}

const char *crthip_error_string(const crthip_ctx *c) { return c ? c->err : "null context"; }

int crthip_reserve(crthip_ctx *c, int n)
{
    if (!c || n <= 0) return CRTHIP_E_ARG;
    if (n <= c->cap_fields) return CRTHIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->d_analog) hipFree(c->d_analog);
    if (c->d_inp) hipFree(c->d_inp);
    if (c->d_lines) hipFree(c->d_lines);
    if (c->d_vhs_next) hipFree(c->d_vhs_next);
    c->d_analog = 0; c->d_inp = 0; c->d_lines = 0; c->d_vhs_next = 0; c->cap_fields = 0; c->last_n = 0;
    const size_t bytes = c->fstride * (size_t) n + 4096;
    /* inp[] of the fused path: padded lines + a scratch row per decoded line (crt_dev.h, sig_layout) -- about twice the flat field */
    const size_t inp_bytes = (c->fstride_pad > c->fstride ? c->fstride_pad : c->fstride) * (size_t) n + 4096;
    if (hipMalloc((void **) &c->d_inp, inp_bytes) != hipSuccess) return set_err(c, CRTHIP_E_NOMEM, "hipMalloc inp", hipSuccess);
    if (hipMalloc((void **) &c->d_analog, bytes) != hipSuccess) return set_err(c, CRTHIP_E_NOMEM, "hipMalloc analog", hipSuccess);
    if (hipMalloc((void **) &c->d_lines, sizeof(crthip_line) * (size_t) n * c->sd.lines) != hipSuccess)
        return set_err(c, CRTHIP_E_NOMEM, "hipMalloc lines", hipSuccess);
    if (c->system == CRTHIP_SYSTEM_NTSCVHS &&
        hipMalloc((void **) &c->d_vhs_next, sizeof(unsigned) * 32 * (size_t) n) != hipSuccess)
        return set_err(c, CRTHIP_E_NOMEM, "hipMalloc VHS histories", hipSuccess);
    /* the internal second stream (VHS noise pair, overlap chunks) exists from here on: a field-pass creates nothing (graph capture) */
    if (crt_ensure_aux(c) != CRTHIP_OK) return set_err(c, CRTHIP_E_HIP, "internal stream", hipGetLastError());
    HIPCHK(c, hipMemsetAsync(c->d_inp, 0, inp_bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_analog, 0, bytes, c->stream));
    if (!c->sd.nes_timing) {                    /* bloom builds (none with the NES timing): the decoder's sort scratch, 4 bytes per scanline */
        const int rc = crt_reserve_bloom(c, n);
        if (rc) return rc;
    }
    c->cap_fields = n;
    return CRTHIP_OK;
}

static int check_params(crthip_ctx *c, const crthip_params *p, int n)
{
    if (!c || !p || n <= 0) return CRTHIP_E_ARG;
    if (p->finalized != CRTHIP_PARAMS_MAGIC) return set_err(c, CRTHIP_E_ARG, "params not finalized", hipSuccess);
    if (p->system != c->system || p->chroma_pattern != c->pattern) return set_err(c, CRTHIP_E_ARG, "params are for another system", hipSuccess);
    return CRTHIP_OK;
}

/* The buffer contract of include/crt_hip.h ("Buffer contract"; DESIGN.md has the table): the kernels move 4-byte pixels as dwords
 * and in 16-byte pieces typed to 4-byte alignment (crt_dev.h: gload32 / gstore32, the _nt pieces; crt_encode.hip: k_active_row),
 * PPU pixels as 16-bit words, and every record array as ints.  A base or a stride off that grid is refused HERE, before anything
 * is launched, copied or reserved; 3-byte pixels travel bytewise and take any base and stride. */
static bool off_grid(const void *ptr, size_t stride, size_t a)
{
    return a > 1 && ((((size_t) ptr) | stride) & (a - 1)) != 0;
}
static int check_images(crthip_ctx *c, const crthip_params *p, const void *d_images, size_t istride)
{
    const bool ppu = c->system == CRTHIP_SYSTEM_NES;
    if (off_grid(d_images, istride, ppu ? 2 : p->in_bpp == 4 ? 4 : 1))
        return set_err(c, CRTHIP_E_ARG, ppu ? "d_images / image_stride: PPU pixels need 2-byte alignment"
                                            : "d_images / image_stride: 4-byte pixels need 4-byte alignment", hipSuccess);
    return CRTHIP_OK;
}
static int check_out(crthip_ctx *c, const crthip_params *p, const void *d_out, size_t ostride, const void *d_init = nullptr, size_t init_stride = 0)
{
    const size_t a = p->out_bpp == 4 ? 4 : 1;
    if (off_grid(d_out, ostride, a)) return set_err(c, CRTHIP_E_ARG, "d_out / out_stride: 4-byte pixels need 4-byte alignment", hipSuccess);
    if (off_grid(d_init, init_stride, a)) return set_err(c, CRTHIP_E_ARG, "d_out_init / out_init_stride: 4-byte pixels need 4-byte alignment", hipSuccess);
    return CRTHIP_OK;
}
/* crthip_state, crthip_line, crthip_knob_rec, the VHS histories; d_analog / d_inp (the signal kernels move dwords too) */
static int check_word(crthip_ctx *c, const void *ptr, const char *msg)
{
    return off_grid(ptr, 0, 4) ? set_err(c, CRTHIP_E_ARG, msg, hipSuccess) : CRTHIP_OK;
}
#define CHECK_WORD(c, ptr) check_word(c, ptr, #ptr " needs 4-byte alignment")

/* the stage-level entry points: the host owns the output buffer between the stages (crt_main.c:459-463 fades it itself) */
static int check_stage_params(crthip_ctx *c, const crthip_params *p, int n)
{
    const int rc = check_params(c, p, n);
    if (rc) return rc;
    if (p->flags & CRTHIP_PHOSPHOR_MASK)
        return set_err(c, CRTHIP_E_ARG, "phosphor fade / clear: only crthip_fieldpass and the sequence entry points own the output buffer", hipSuccess);
    return CRTHIP_OK;
}

/* The encoder contract.  The reference writes analog[(x + xo) + (y + yo) * HRES] (crt_ntsc.c:322) -- a FLAT index:
 * a rectangle that runs over the end of a line (xoffset = 4 in standard NTSC: 160 + 753 > 910) simply continues in
 * the next line's front porch, and the kernels do exactly the same (they work on flat indices too).  What is refused
 * is only what is undefined in the reference: samples outside analog[], and negative origins (negative carrier
 * table index, crt_ntsc.c:314). */
static int check_encoder(crthip_ctx *c, const crthip_params *p)
{
    if (c->system != CRTHIP_SYSTEM_NES && p->in_bpp == 0) return 1;   /* silent no-op, crt_ntsc.c:190-193 */
    if (p->col_step_hi == 0 && p->col_step_lo == 0)                    /* ceil(2^32 * w / destw) is never 0 */
        return set_err(c, CRTHIP_E_ARG, "params were finalized by an older library (no col_step): call crthip_params_finalize again", hipSuccess);
    const long long end = (long long) p->yo * c->sd.hres + p->xo + (long long) (p->desth - 1) * c->sd.hres + p->destw;
    if (p->xo < 0 || p->yo < 0 || p->destw <= 0 || p->desth <= 0 || p->destw > c->sd.hres || end > c->sd.input_size)
        return set_err(c, CRTHIP_E_ARG, "active rectangle leaves analog[] (xoffset/yoffset out of contract)", hipSuccess);
    return CRTHIP_OK;
}

int crthip_modulate(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                    signed char *d_analog, crthip_state *d_state)
{
    int rc = check_stage_params(c, p, n);
    if (rc) return rc;
    rc = check_encoder(c, p);
    if (rc) return rc < 0 ? rc : CRTHIP_OK;
    if (!d_images || !d_analog || !d_state) return CRTHIP_E_ARG;
    if ((rc = check_images(c, p, d_images, istride)) || (rc = CHECK_WORD(c, d_analog)) || (rc = CHECK_WORD(c, d_state))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = crt_run_encoder_prepare(c, p, false);
    if (rc) return rc;
    rc = crt_run_encoder(c, p, n, d_images, istride, d_analog, d_state, false, (p->flags & CRTHIP_F_NES_SETUP) != 0, true);
    HIPCHK(c, hipGetLastError());
    return rc;
}

int crthip_noise(crthip_ctx *c, const crthip_params *p, int n, const signed char *d_analog, signed char *d_inp,
                 crthip_state *d_state)
{
    int rc = check_stage_params(c, p, n);
    if (rc) return rc;
    if (p->out_bpp == 0) return CRTHIP_OK;                       /* crt_core.c:312-315 */
    if (!d_analog || !d_inp || !d_state) return CRTHIP_E_ARG;
    if ((rc = CHECK_WORD(c, d_analog)) || (rc = CHECK_WORD(c, d_inp)) || (rc = CHECK_WORD(c, d_state))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (p->flags & CRTHIP_F_NO_VSYNC) {                         /* CRT_DO_VSYNC 0: crt_core.c:323-341, before the noise */
        rc = crt_run_clean_vsync(c, n, d_analog, d_state);
        if (rc) return rc;
    }
    rc = crt_run_noise(c, p, n, d_analog, d_inp, d_state, true);
    HIPCHK(c, hipGetLastError());
    return rc;
}

int crthip_sync(crthip_ctx *c, const crthip_params *p, int n, const signed char *d_inp, crthip_state *d_state,
                crthip_line *d_lines)
{
    int rc = check_stage_params(c, p, n);
    if (rc) return rc;
    if (p->out_bpp == 0) return CRTHIP_OK;
    if (!d_inp || !d_state || !d_lines) return CRTHIP_E_ARG;
    if ((rc = CHECK_WORD(c, d_inp)) || (rc = CHECK_WORD(c, d_state)) || (rc = CHECK_WORD(c, d_lines))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = crt_run_sync(c, p, n, d_inp, d_state, d_lines, 0);
    HIPCHK(c, hipGetLastError());
    return rc;
}

int crthip_decode(crthip_ctx *c, const crthip_params *p, int n, const signed char *d_inp, const crthip_line *d_lines,
                  void *d_out, size_t ostride)
{
    int rc = check_stage_params(c, p, n);
    if (rc) return rc;
    if (p->out_bpp == 0) return CRTHIP_OK;
    if (!d_inp || !d_lines || !d_out) return CRTHIP_E_ARG;
    if ((rc = CHECK_WORD(c, d_inp)) || (rc = CHECK_WORD(c, d_lines)) || (rc = check_out(c, p, d_out, ostride))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = crt_run_decode(c, p, n, d_inp, d_lines, d_out, ostride);
    HIPCHK(c, hipGetLastError());
    return rc;
}

/* ---- the records of the call in flight (crt_dev.h: rec_call, and the table of the blob words) ----------------------------- */

/* the picture words of an env (crthip_knobs_prepare5; all 0 from crthip_knobs_prepare): do they agree with each other? */
static bool knobs_env_pic_ok(const crthip_knobs_env *env)
{
    if (env->pic == 0) return env->tier_floors == 0 && env->bright_abs_lo == 0;
    const int lo = env->tier_floors & 0xff, hi = (env->tier_floors >> 8) & 0xff;
    return env->pic == 1 && (env->tier_floors & ~0xffff) == 0 && lo <= hi && hi <= 3 && lo != 1 && hi != 1 &&
           env->bright_abs_lo >= 0 && env->bright_abs_lo <= T0_BRIGHT_MAX && (lo < 2 || env->bright_abs_lo == 0);
}

/* what a crthip_knobs_env must say wherever it arrives: with a call of n fields, or (n == 0) at crthip_seq_bind_knobs */
static int knobs_env_check(crthip_ctx *c, const crthip_knobs_env *env, int n)
{
    if (env->magic != CRTHIP_KNOBS_MAGIC) return set_err(c, CRTHIP_E_ARG, "knobs: env does not come from crthip_knobs_prepare", hipSuccess);
    if (n && env->n != n) return set_err(c, CRTHIP_E_ARG, "knobs: env was prepared for another number of fields", hipSuccess);
    if (c->sd.cc_samples == 5)
        return set_err(c, CRTHIP_E_ARG, "knobs: the 5-sample decoder (PV-1000) takes monitor hue and saturation from the uniform parameters", hipSuccess);
    if (env->n <= 0 || env->noise_max < 0 || env->sat_abs_max < 0) return set_err(c, CRTHIP_E_ARG, "knobs: env bounds", hipSuccess);
    if (!knobs_env_pic_ok(env)) return set_err(c, CRTHIP_E_ARG, "knobs: the env's picture words contradict each other (not from crthip_knobs_prepare5)", hipSuccess);
    return CRTHIP_OK;
}

/* The one place that writes record pointers into a blob: for a launch that starts at field `first` of the call, every record array
 * of c->call, advanced to that field, into its words of *q (the table in crt_dev.h).  Sizes: the images have no stride -- the
 * records' offsets count from the base of the image buffer whatever the launch's first field. */
static void launch_blob(const crthip_ctx *c, int first, crthip_params *q)
{
    const rec_call &k = c->call;
    if (k.knobs) blob_put_ptr(q->reserved, k.knobs + first);
    if (k.levels) blob_put_ptr(&q->white, k.levels + first);
    if (k.hues) blob_put_ptr(&q->burst[0][0], k.hues + first);
    if (k.sizes) blob_put_ptr(k.knobs ? (void *) &q->col_step_lo : (void *) q->reserved, k.sizes + first);
}

/* which records a call brings: none (the uniform call), knob records, size records, both, or -- the phases of sequence mode --
 * whatever crthip_seq_bind_knobs has bound */
enum { REC_KNOBS = 1, REC_SIZES = 2, REC_SEQ_BOUND = 4 };

/* The one way in.  Checks the records and envs of a call of n fields (p went through check_params), sizes first, and only then
 * says so in c->call -- a refused call leaves the uniform call standing.  *q = the blob the call's launch code decides by and its
 * kernels receive: the caller's, with the knob env's bounds where that code reads the uniform values (noise != 0, the encoder's
 * 24-bit envelope; mon_hue / huesn / huecs / bloom_max_e are read by the KN kernels alone, from the records) and the pointers to the
 * records of field 0 (launch_blob).  The bindings (crthip_bind_levels / _hues, crthip_seq_bind_knobs) are read here and nowhere else:
 * every knob call runs with the level and hue records that are bound -- or is refused, before anything is launched.  The host sees
 * envs, not records: what it checks of the sizes is that the image a wavefront falls back to for a record it refuses
 * (size_rec_checked, crt_dev.h) lies inside the extent. */
static int call_begin(crthip_ctx *c, const crthip_params *p, int n, int kinds, const crthip_knob_rec *d_recs, const crthip_knobs_env *env,
                      const void *d_images, const crthip_size_rec *d_srecs, const crthip_sizes_env *senv, crthip_params *q)
{
    rec_call k = {};
    if (kinds & REC_SEQ_BOUND) {
        d_recs = c->seq_knob_recs;
        env = &c->seq_knob_env;
        if (d_recs) kinds |= REC_KNOBS;                   /* nothing bound: exactly the uniform phase */
    }
    *q = *p;
    if (kinds & REC_SIZES) {
        if (!d_srecs || !senv) return set_err(c, CRTHIP_E_ARG, "sizes: no records / no env", hipSuccess);
        if (CHECK_WORD(c, d_srecs)) return CRTHIP_E_ARG;
        if (senv->magic != CRTHIP_SIZES_MAGIC) return set_err(c, CRTHIP_E_ARG, "sizes: env does not come from crthip_sizes_prepare", hipSuccess);
        if (senv->n != n) return set_err(c, CRTHIP_E_ARG, "sizes: env was prepared for another number of fields", hipSuccess);
        if (p->raw != 0) return set_err(c, CRTHIP_E_ARG, "sizes: raw images (the signal rectangle then depends on w and h)", hipSuccess);
        if (c->system == CRTHIP_SYSTEM_NES) return set_err(c, CRTHIP_E_ARG, "sizes: the NES encoder (PPU pixels) has no per-field instantiation", hipSuccess);
        if (p->in_bpp == 0) return set_err(c, CRTHIP_E_ARG, "sizes: an input format crt_modulate refuses", hipSuccess);
        const size_t extent = ((size_t) senv->extent_hi << 32) | senv->extent_lo;
        const bool spare = (p->flags & CRTHIP_F_IMAGE_SPARE_ROW) != 0;
        const bool tiles = p->in_bpp == 4 && senv->w_min >= 4;
        if (senv->w_min < 1 || senv->w_min > senv->w_max || senv->h_min < 1 || senv->h_min > senv->h_max ||
            extent < (size_t) (tiles ? 4 : 1) * (size_t) p->in_bpp * (spare ? 2 : 1))
            return set_err(c, CRTHIP_E_ARG, "sizes: the env's bounds contradict each other (not from crthip_sizes_prepare)", hipSuccess);
        if (d_images && p->in_bpp == 4 && off_grid(d_images, 0, 4))
            return set_err(c, CRTHIP_E_ARG, "d_images: 4-byte pixels need 4-byte alignment", hipSuccess);
        k.sizes = d_srecs;
        k.size_env = *senv;
    }
    if (kinds & REC_KNOBS) {
        if (!d_recs || !env) return CRTHIP_E_ARG;
        if (CHECK_WORD(c, d_recs)) return CRTHIP_E_ARG;
        const int rc = knobs_env_check(c, env, n);
        if (rc) return rc;
        if ((p->flags & CRTHIP_PHOSPHOR_MASK) == CRTHIP_PHOSPHOR_MASK)
            return set_err(c, CRTHIP_E_ARG, "phosphor fade and clear at once (crt_main.c:459-463: one or the other)", hipSuccess);
        if (c->lev_recs) {
            if (c->lev_env.n != n) return set_err(c, CRTHIP_E_ARG, "levels: the bound crthip_levels_env was prepared for another number of fields", hipSuccess);
            if (env->pic != 1)
                return set_err(c, CRTHIP_E_ARG, "levels: bound level records go with the records of crthip_knobs_prepare7 (env->pic == 1: bright per field)", hipSuccess);
            if (p->flags & CRTHIP_F_NES_BORDER)
                return set_err(c, CRTHIP_E_ARG, "levels: CRTHIP_F_NES_BORDER bakes the border colour into the cached skeleton with ONE (black point, white point) pair", hipSuccess);
            if (c->system == CRTHIP_SYSTEM_NES)
                return set_err(c, CRTHIP_E_ARG, "levels: the NES encoder's samples come from a 512 x 12 table built for ONE (black point, white point) pair", hipSuccess);
        }
        if (c->hue_recs) {                                /* likewise, and independently of the levels */
            if (c->hue_env.n != n) return set_err(c, CRTHIP_E_ARG, "hues: the bound crthip_hues_env was prepared for another number of fields", hipSuccess);
            if (c->system == CRTHIP_SYSTEM_NES)
                return set_err(c, CRTHIP_E_ARG, "hues: the NES encoder (PPU pixels) has no per-field instantiation", hipSuccess);
        }
        k.knobs = d_recs;
        k.levels = c->lev_recs;
        k.lev_env = c->lev_env;
        k.hues = c->hue_recs;
        k.burst0[0] = p->burst[0][0];
        k.burst0[1] = p->burst[0][1];
        k.pic = env->pic;
        k.floor_lo = env->pic ? (env->tier_floors & 0xff) : 0;
        k.loskip = env->loskip_wave_max < LOSKIP_WAVE_MAX ? LOSKIP_WAVE_MAX : env->loskip_wave_max > T0_WAVE_MAX ? T0_WAVE_MAX : env->loskip_wave_max;
        q->noise = env->noise_max;
        q->saturation = env->sat_abs_max;
    }
    c->call = k;
    launch_blob(c, 0, q);
    return CRTHIP_OK;
}

/* The one way out: c->call is the uniform call again, whichever return leaves the scope (refusals and HIPCHK included) */
struct CallScope {
    crthip_ctx *c;
    explicit CallScope(crthip_ctx *ctx) : c(ctx) {}
    ~CallScope() { c->call = rec_call{}; }
};

/* A record entry point: check_params, the way in, body(blob), the way out.  No other line of the library writes c->call. */
extern "C++" template <class Body>
int with_records(crthip_ctx *c, const crthip_params *p, int n, int kinds, const crthip_knob_rec *d_recs, const crthip_knobs_env *env,
                 const void *d_images, const crthip_size_rec *d_srecs, const crthip_sizes_env *senv, Body &&body)
{
    int rc = check_params(c, p, n);
    if (rc) return rc;
    CallScope scope(c);
    crthip_params q;
    rc = call_begin(c, p, n, kinds, d_recs, env, d_images, d_srecs, senv, &q);
    if (rc) return rc;
    return body(&q);
}

/* The blob a sync chain runs on.  Where inp[] was produced here, from a clean analog[] and the encoder, its sample range is known and
 * the decoder's no-low-cascade envelope can be as wide as that range allows (crthip_params.loskip_wave_max; crt_setup_signal_range)
 * -- with knob records, as wide as it is at the call's widest noise (crthip_knobs_prepare).  A signal that is not encoder-made (and
 * the stage-level crthip_sync) keeps the caller's any-signal bound. */
static crthip_params sync_blob(const crthip_ctx *c, const crthip_params *p, bool encoder_made)
{
    crthip_params q = *p;
    if (encoder_made && c->call.knobs) q.loskip_wave_max = c->call.loskip;
    else if (encoder_made) {
        int lo, hi;
        crt_setup_signal_range(p, &lo, &hi);
        q.loskip_wave_max = crt_setup_loskip_bound(lo, hi);
    }
    return q;
}

/* one chunk of a batch, fields [first, first+n), on the context's current stream.  `part` (bits): 1 = encoder + channel
 * noise, 4 = the sync chain up to the line table, 2 = the decoder (the rand()-noise VHS build and CRT_DO_VSYNC 0 run 1 and 4
 * as one unit under bit 1) */
static int fieldpass_chunk(crthip_ctx *c, const crthip_params *p, int enc, int first, int n, int part, const sig_layout &lay,
                           const void *d_images, size_t istride, void *d_out, size_t ostride, crthip_state *d_state)
{
    /* lay: where this field-pass keeps its signal (crt_fused_layout; the same for every chunk and part of a call) */
    const unsigned char *img = (const unsigned char *) d_images + (size_t) first * istride;
    unsigned char *out = (unsigned char *) d_out + (size_t) first * ostride;
    crthip_state *st = d_state + first;
    signed char *inp = c->d_inp + (size_t) first * lay.fstride;
    signed char *analog = c->d_analog + (size_t) first * c->fstride;
    crthip_line *ln = c->d_lines + (size_t) first * c->sd.lines;
    int rc = CRTHIP_OK;
    bool preset = false;
    crthip_params pk = *p;
    launch_blob(c, first, &pk);                           /* the records of THIS chunk's first field */
    p = &pk;
    if (part & 1) {
        const bool vhs_rand = c->system == CRTHIP_SYSTEM_NTSCVHS && !(p->flags & CRTHIP_F_VHS_LCG_NOISE);
        if (vhs_rand || (p->flags & CRTHIP_F_NO_VSYNC)) {
            /* (CRT_DO_VSYNC 0 needs the clean field as well: its vertical sync search reads analog[], crt_core.c:323-341) */
            /* VHS noise follows the C library's rand() stream, not the LCG: the fused encoder (margins + active
             * rectangle = every sample of the field) runs with noise 0 into analog[], then the dedicated noise
             * kernels (which also produce rn) */
            if (enc == 0) {
                crthip_params clean = *p;
                clean.noise = 0;
                rc = crt_run_encoder(c, &clean, n, img, istride, analog, st, true, 1, true);
            } else {
                hipMemsetAsync(analog, 0, c->fstride * (size_t) n, c->stream);   /* crt_modulate refused the format */
            }
            if (rc) return rc;
            if (p->out_bpp == 0) return CRTHIP_OK;
            unsigned *saved = c->d_vhs_hist;
            if (vhs_rand) c->d_vhs_hist = saved + (size_t) first * 32;
            crthip_params pn = *p;
            pn.flags &= ~CRTHIP_PHOSPHOR_MASK;            /* the display step belongs to the decoder part below */
            rc = crthip_noise(c, &pn, n, analog, inp, st);
            c->d_vhs_hist = saved;
            if (rc) return rc;
            rc = crt_run_sync(c, p, n, inp, st, ln, 0);
            part &= ~4;
        } else {
            if (enc == 0) {
                /* the encoder writes the noisy field straight into inp[]; analog[] is never materialised.  What crt_modulate
                 * leaves in the state (ccf preset, M6) is applied by the sync chain's own waves when it follows at once
                 * (k_hsync_wave, preset_ccf): one launch less per field-pass */
                preset = (part & 4) && p->out_bpp != 0 && c->system != CRTHIP_SYSTEM_NTSCVHS;   /* (VHS also resets hsync there) */
                if (c->call.hues) preset = false;     /* the preset comes from every field's own burst table: k_encoder_state's HU instantiation */
                rc = crt_run_encoder(c, p, n, img, istride, inp, st, true, 1, !preset, &lay);
            } else {
                /* invalid input format: crt_modulate is a no-op, the decoder sees a clean field + noise
                 * (rn is advanced by k_vsync below) */
                hipMemsetAsync(analog, 0, c->fstride * (size_t) n, c->stream);
                rc = crt_run_noise(c, p, n, analog, inp, st, false);
            }
        }
        if (rc) return rc;
    }
    if ((part & 4) && p->out_bpp != 0) {
        const crthip_params q = sync_blob(c, p, enc == 0);
        rc = crt_run_sync(c, &q, n, inp, st, ln, 1, preset ? 1 : 0, &lay);
        if (rc) return rc;
    }
    if ((part & 2) && p->out_bpp != 0) {
        launch_phosphor_rows(c, p, n, ln, out, ostride);
        rc = crt_run_decode(c, p, n, inp, ln, out, ostride, lay.fstride);
    }
    return rc;
}

/* Room for n fields in the workspace, no claim on the signal it holds -- what crthip_fieldpass_signal may unpad is the signal of the
 * last call that was enqueued COMPLETELY, and a call refused half-way leaves none --, and (tables) the encoder's tables for p, (re)built
 * on the caller's stream before anything forks */
static int encoder_ready(crthip_ctx *c, const crthip_params *p, int n, bool tables)
{
    if (n > c->cap_fields) {
        const int rc = crthip_reserve(c, n);
        if (rc) return rc;
    }
    c->last_n = 0;
    return tables ? crt_run_encoder_prepare(c, p, true) : CRTHIP_OK;
}

/* What crthip_fieldpass* and crthip_stills* do with their arguments before the first launch (p went through check_params): the buffer
 * contract (null_msg: what the error string says of a null pointer, nullptr = nothing), the encoder's (*enc: 0 = encodes, 1 = an
 * input format crt_modulate refuses), the workspace and the tables, and *lay = the signal between the call's encoder and its decoder:
 * padded lines where the fused LCG-noise encoder writes it (crt_dev.h) */
static int fused_front(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride, void *d_out, size_t ostride,
                       crthip_state *d_state, const char *null_msg, int *enc, sig_layout *lay)
{
    int rc;
    if (!d_images || !d_out || !d_state) return null_msg ? set_err(c, CRTHIP_E_ARG, null_msg, hipSuccess) : CRTHIP_E_ARG;
    if ((rc = check_images(c, p, d_images, istride)) || (rc = check_out(c, p, d_out, ostride)) || (rc = CHECK_WORD(c, d_state))) return rc;
    const bool vhs_rand = c->system == CRTHIP_SYSTEM_NTSCVHS && !(p->flags & CRTHIP_F_VHS_LCG_NOISE);
    if (vhs_rand && !c->d_vhs_hist)
        return set_err(c, CRTHIP_E_ARG, "VHS: no generator histories bound (crthip_vhs_bind_history)", hipSuccess);
    *enc = check_encoder(c, p);
    if (*enc < 0) return *enc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = encoder_ready(c, p, n, *enc == 0);
    if (rc) return rc;
    if (*enc != 0 || vhs_rand || !crt_fused_layout(c, p, n, lay)) *lay = flat_layout(c);
    return CRTHIP_OK;
}

/* every crthip_fieldpass* entry point, on the blob of its records (call_begin) */
static int fieldpass_body(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                          void *d_out, size_t ostride, crthip_state *d_state)
{
    int enc;
    sig_layout lay;
    int rc = fused_front(c, p, n, d_images, istride, d_out, ostride, d_state, nullptr, &enc, &lay);
    if (rc) return rc;
    /* Fields are independent, so a large batch can be cut into chunks (crthip_set_overlap) -- the idea: run the vector / latency bound
     * encoder + sync chain of one chunk under the HBM-write bound decoder of the previous one.  0 = automatic = one chunk: no
     * configuration gains.  Measured on MI355X (profiles/r02_overlap_sweep.txt): at 1080p the encoder's image reads and the decoder's
     * picture writes already saturate what HBM delivers for this access mix, running them side by side is slower than one after the
     * other (2 chunks -3 %, 8 chunks -19 %); at 640x480 every kernel is vector bound and chunks only add latency.  Round 3 also tried
     * only the sync chain of the second half of the batch under the decoder of the first: 3-4 % slower at 640x480 and 1080p alike
     * (profiles/r03_1080p_experiments.txt). */
    const int want_chunks = c->overlap_chunks ? c->overlap_chunks : 1;
    const int nchunks = (want_chunks > 1 && n >= 256 * want_chunks && !c->prof) ? want_chunks : 1;
    if (nchunks == 1) {
        rc = fieldpass_chunk(c, p, enc, 0, n, 7, lay, d_images, istride, d_out, ostride, d_state);
    } else {
        /* Two-stage software pipeline over the chunks: the encoder + sync chain of ALL chunks run back to back on an
         * internal stream, the decoders on the caller's stream, decoder k waiting for the event behind sync chain k.
         * While decoder k streams its picture out (HBM-write bound at 1080p), the vector-bound encoder of chunk k+1
         * and the latency-bound sync chain run beside it.  (Alternating whole chunks between two streams, the first
         * version of this, ends up running decoder next to decoder: profiles/r02_overlap_timeline_1080p.txt.) */
        if (crt_ensure_aux(c) != CRTHIP_OK) return set_err(c, CRTHIP_E_HIP, "internal stream", hipGetLastError());
        hipStream_t main_stream = c->stream;
        HIPCHK(c, hipEventRecord(c->ev_fork, main_stream));
        HIPCHK(c, hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0));
        const int per = ((n + nchunks - 1) / nchunks + 3) & ~3;
        c->stream = c->aux_stream;
        int used = 0;
        for (int k = 0, first = 0; first < n && rc == CRTHIP_OK; k++, first += per) {
            const int cnt = n - first < per ? n - first : per;
            rc = fieldpass_chunk(c, p, enc, first, cnt, 1 | 4, lay, d_images, istride, d_out, ostride, d_state);
            if (rc == CRTHIP_OK && hipEventRecord(c->ev_chunk[k], c->aux_stream) != hipSuccess) rc = CRTHIP_E_HIP;
            used = k + 1;
        }
        c->stream = main_stream;
        for (int k = 0, first = 0; k < used && rc == CRTHIP_OK; k++, first += per) {
            const int cnt = n - first < per ? n - first : per;
            HIPCHK(c, hipStreamWaitEvent(main_stream, c->ev_chunk[k], 0));
            rc = fieldpass_chunk(c, p, enc, first, cnt, 2, lay, d_images, istride, d_out, ostride, d_state);
        }
        /* the caller's stream has waited for every event of the internal stream: nothing is left running there */
    }
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    c->last_lay = lay;
    c->last_n = n;
    return CRTHIP_OK;
}

int crthip_fieldpass(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                     void *d_out, size_t ostride, crthip_state *d_state)
{
    return with_records(c, p, n, 0, nullptr, nullptr, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return fieldpass_body(c, q, n, d_images, istride, d_out, ostride, d_state); });
}

int crthip_fieldpass_knobs(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                           void *d_out, size_t ostride, crthip_state *d_state, const crthip_knob_rec *d_recs, const crthip_knobs_env *env)
{
    return with_records(c, p, n, REC_KNOBS, d_recs, env, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return fieldpass_body(c, q, n, d_images, istride, d_out, ostride, d_state); });
}

/* (a call with size records has no image stride: `istride` carries the extent of the image buffer to the SZ kernels, crt_encode.hip) */
int crthip_fieldpass_sizes(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, void *d_out, size_t ostride,
                           crthip_state *d_state, const crthip_size_rec *d_srecs, const crthip_sizes_env *senv)
{
    return with_records(c, p, n, REC_SIZES, nullptr, nullptr, d_images, d_srecs, senv, [&](const crthip_params *q) {
        return fieldpass_body(c, q, n, d_images, 0, d_out, ostride, d_state); });
}

int crthip_fieldpass_sizes_knobs(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, void *d_out, size_t ostride,
                                 crthip_state *d_state, const crthip_size_rec *d_srecs, const crthip_sizes_env *senv,
                                 const crthip_knob_rec *d_recs, const crthip_knobs_env *env)
{
    return with_records(c, p, n, REC_SIZES | REC_KNOBS, d_recs, env, d_images, d_srecs, senv, [&](const crthip_params *q) {
        return fieldpass_body(c, q, n, d_images, 0, d_out, ostride, d_state); });
}

/* ---- stills ---------------------------------------------------------------------------------------------------------------- */
int crthip_stills_schedule(int interlaced, int first_field, int n_frames, crthip_pass *sched, int cap)
{
    if (!sched || n_frames <= 0 || n_frames > CRTHIP_STILLS_MAX_PASSES) return CRTHIP_E_ARG;
    const int total = interlaced ? 2 * n_frames : n_frames;
    if (total > cap || total > CRTHIP_STILLS_MAX_PASSES) return CRTHIP_E_ARG;
    int field = first_field & 1, frame = 0, r = 0;
    for (int e = 0; e < n_frames; e++) {                  /* crt_main.c:241-255 */
        sched[r].field = field; sched[r].frame = frame; sched[r].aux = 0; sched[r].reserved = 0; r++;
        if (interlaced) {
            field ^= 1;
            sched[r].field = field; sched[r].frame = frame; sched[r].aux = 0; sched[r].reserved = 0; r++;
            if ((e & 1) == 0) frame ^= 1;                 /* a frame is two fields */
        }
    }
    return r;
}

/* the shared-signal workspace for n_fields fields of `fstride` bytes (0: the largest a layout of this system takes) */
static int stills_workspace(crthip_ctx *c, size_t n_fields, size_t fstride)
{
    if (!fstride) fstride = c->fstride_pad > c->fstride ? c->fstride_pad : c->fstride;
    const size_t need = fstride * n_fields + 4096;
    if (need <= c->still_cap) return CRTHIP_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->d_still_sig) hipFree(c->d_still_sig);
    c->d_still_sig = 0; c->still_cap = 0;
    if (hipMalloc((void **) &c->d_still_sig, need) != hipSuccess) return set_err(c, CRTHIP_E_NOMEM, "hipMalloc stills signal workspace", hipSuccess);
    c->still_cap = need;
    c->still_lay.pitch = 0;                               /* holds nothing yet: the first call clears what it will use */
    return CRTHIP_OK;
}

int crthip_stills_reserve(crthip_ctx *c, int n, int n_distinct)
{
    if (!c || n <= 0 || n_distinct <= 0 || n_distinct > CRTHIP_STILLS_MAX_PASSES) return CRTHIP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = crthip_reserve(c, n);
    if (rc) return rc;
    return stills_workspace(c, (size_t) n * n_distinct, 0);
}

/* every crthip_stills* entry point, on the blob of its records (call_begin: with knob records p->noise = the call's largest noise,
 * which decides the shared path) */
static int stills_body(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                       void *d_out, size_t ostride, crthip_state *d_state, int n_passes, const crthip_pass *sched)
{
    if (n_passes <= 0 || n_passes > CRTHIP_STILLS_MAX_PASSES)
        return set_err(c, CRTHIP_E_ARG, "crthip_stills: n_passes must be 1 .. CRTHIP_STILLS_MAX_PASSES", hipSuccess);
    if (!sched) return set_err(c, CRTHIP_E_ARG, "crthip_stills: no schedule (sched == NULL)", hipSuccess);
    int rc;
    if (p->out_bpp != 0 && (rc = crt_decode_check(c, p))) return rc;      /* what the decoder of pass 0 would refuse, before anything runs */
    /* the rest as a field-pass of these n fields, its layout included; crthip_fieldpass_signal is refused after a stills call (crt_hip.h) */
    int enc;
    sig_layout lay;
    rc = fused_front(c, p, n, d_images, istride, d_out, ostride, d_state, "crthip_stills: null device pointer", &enc, &lay);
    if (rc) return rc;
    const bool vhs_rand = c->system == CRTHIP_SYSTEM_NTSCVHS && !(p->flags & CRTHIP_F_VHS_LCG_NOISE);
    const dim3 gn((n + 63) / 64), b64(64);
    const bool shared = p->noise == 0 && enc == 0 && !vhs_rand && !(p->flags & CRTHIP_F_NO_VSYNC) && p->out_bpp != 0;
    if (!shared) {
        /* the loop itself: every pass encodes (its noise differs from pass to pass), in the field-pass workspace */
        for (int r = 0; r < n_passes; r++) {
            hipLaunchKernelGGL(k_stills_pass, gn, b64, 0, c->stream, n, d_state, sched[r]);
            rc = fieldpass_chunk(c, p, enc, 0, n, 7, lay, d_images, istride, d_out, ostride, d_state);
            if (rc) return rc;
        }
        HIPCHK(c, hipGetLastError());
        return CRTHIP_OK;
    }
    /* noise 0: the clean signal of every distinct entry once, slot[r] = where pass r's signal is */
    int slot[CRTHIP_STILLS_MAX_PASSES], first_of[CRTHIP_STILLS_MAX_PASSES], n_distinct = 0;
    for (int r = 0; r < n_passes; r++) {
        int e = 0;
        while (e < n_distinct && !((sched[first_of[e]].field & 1) == (sched[r].field & 1) && (sched[first_of[e]].frame & 1) == (sched[r].frame & 1) &&
                                   sched[first_of[e]].aux == sched[r].aux)) e++;
        if (e == n_distinct) first_of[n_distinct++] = r;
        slot[r] = e;
    }
    rc = stills_workspace(c, (size_t) n * n_distinct, lay.fstride);
    if (rc) return rc;
    if (c->still_lay.pitch != lay.pitch || c->still_lay.shift != lay.shift || c->still_lay.fstride != lay.fstride) {
        /* another layout than the one the workspace last held (or none yet): the bytes a layout reads without ever writing them --
         * the slack behind a flat field, the pads beyond the copies, the line behind the tail -- are zero for every call */
        HIPCHK(c, hipMemsetAsync(c->d_still_sig, 0, c->still_cap, c->stream));
        c->still_lay = lay;
    }
    const size_t slot_bytes = lay.fstride * (size_t) n;
    for (int e = 0; e < n_distinct; e++) {
        hipLaunchKernelGGL(k_stills_pass, gn, b64, 0, c->stream, n, d_state, sched[first_of[e]]);
        rc = crt_run_encoder(c, p, n, d_images, istride, c->d_still_sig + (size_t) e * slot_bytes, d_state, true, 1, false, &lay);
        if (rc) return rc;
    }
    /* what crt_modulate leaves in the state is applied per pass: by the sync chain's own waves (preset_ccf), or -- VHS, which also
     * resets hsync there -- by k_encoder_state, exactly as a field-pass does */
    /* (hue records: the preset comes from every still's own burst table, k_encoder_state's HU instantiation, as in a field-pass) */
    const bool preset = c->system != CRTHIP_SYSTEM_NTSCVHS && !c->call.hues;
    const crthip_params q = sync_blob(c, p, true);
    unsigned char *out = (unsigned char *) d_out;
    for (int r = 0; r < n_passes; r++) {
        const signed char *sig = c->d_still_sig + (size_t) slot[r] * slot_bytes;
        hipLaunchKernelGGL(k_stills_pass, gn, b64, 0, c->stream, n, d_state, sched[r]);
        if (!preset) {
            rc = crt_run_encoder_state(c, p, n, d_state);
            if (rc) return rc;
        }
        rc = crt_run_sync(c, &q, n, sig, d_state, c->d_lines, 1, preset ? 1 : 0, &lay);
        if (rc) return rc;
        launch_phosphor_rows(c, p, n, c->d_lines, out, ostride);
        rc = crt_run_decode(c, p, n, sig, c->d_lines, out, ostride, lay.fstride);
        if (rc) return rc;
    }
    HIPCHK(c, hipGetLastError());
    return CRTHIP_OK;
}

int crthip_stills(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                  void *d_out, size_t ostride, crthip_state *d_state, int n_passes, const crthip_pass *sched)
{
    return with_records(c, p, n, 0, nullptr, nullptr, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return stills_body(c, q, n, d_images, istride, d_out, ostride, d_state, n_passes, sched); });
}

/* Record k is still k's look and / or size in every pass: every launch of the body reads the records the way a field-pass of the n
 * stills does.  With the call's largest noise 0 the clean signal of every distinct entry is encoded once WITH the blob of the records
 * (the SZ instantiations, with LV / HU where levels / hues are bound: a still's clean signal depends on its own size, levels and hue,
 * not on the pass). */
int crthip_stills_knobs(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                        void *d_out, size_t ostride, crthip_state *d_state, int n_passes, const crthip_pass *sched,
                        const crthip_knob_rec *d_recs, const crthip_knobs_env *env)
{
    return with_records(c, p, n, REC_KNOBS, d_recs, env, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return stills_body(c, q, n, d_images, istride, d_out, ostride, d_state, n_passes, sched); });
}

int crthip_stills_sizes(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, void *d_out, size_t ostride,
                        crthip_state *d_state, int n_passes, const crthip_pass *sched,
                        const crthip_size_rec *d_srecs, const crthip_sizes_env *senv)
{
    return with_records(c, p, n, REC_SIZES, nullptr, nullptr, d_images, d_srecs, senv, [&](const crthip_params *q) {
        return stills_body(c, q, n, d_images, 0, d_out, ostride, d_state, n_passes, sched); });
}

int crthip_stills_sizes_knobs(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, void *d_out, size_t ostride,
                              crthip_state *d_state, int n_passes, const crthip_pass *sched,
                              const crthip_size_rec *d_srecs, const crthip_sizes_env *senv,
                              const crthip_knob_rec *d_recs, const crthip_knobs_env *env)
{
    return with_records(c, p, n, REC_SIZES | REC_KNOBS, d_recs, env, d_images, d_srecs, senv, [&](const crthip_params *q) {
        return stills_body(c, q, n, d_images, 0, d_out, ostride, d_state, n_passes, sched); });
}

unsigned crthip_table_generation(const crthip_ctx *c) { return c ? c->table_gen : 0u; }

int crthip_set_signal_tile(crthip_ctx *c, int dwords)
{
    if (!c || (dwords != 0 && dwords != 16 && dwords != 32 && dwords != 64)) return CRTHIP_E_ARG;
    c->sig_tile_env = dwords;
    return CRTHIP_OK;
}

int crthip_signal_layout_query(const crthip_params *p, int n_fields, int shape, int layout[4], size_t *field_stride)
{
    if (!p || p->finalized != CRTHIP_PARAMS_MAGIC || n_fields <= 0 || shape < 0 || shape > 2) return CRTHIP_E_ARG;
    struct crt_sysdef sd;
    if (crt_sysdef_get(&sd, p->system, p->chroma_pattern) != CRTHIP_OK) return CRTHIP_E_ARG;
    sig_layout lay;
    const bool padded = layout_rule(p->system, p->chroma_pattern, sd, crthip_field_stride(p->system, p->chroma_pattern), p, n_fields, shape, 1, &lay);
    if (layout) { layout[0] = lay.pitch; layout[1] = lay.shift; layout[2] = lay.padv; layout[3] = lay.wrap; }
    if (field_stride) *field_stride = lay.fstride;
    return padded ? 1 : 0;
}

int crthip_float_stages_used(const crthip_ctx *c) { return c ? c->last_fstage : CRTHIP_E_ARG; }

int crthip_set_signal_layout(crthip_ctx *c, int padded)
{
    if (!c || (padded != 0 && padded != 1)) return CRTHIP_E_ARG;
    c->sig_pad = padded;
    return CRTHIP_OK;
}

int crthip_fieldpass_signal(crthip_ctx *c, int n, signed char *d_inp_flat, int *padded)
{
    if (!c || n <= 0 || !d_inp_flat) return CRTHIP_E_ARG;
    if (CHECK_WORD(c, d_inp_flat)) return CRTHIP_E_ARG;
    if (n > c->last_n || !c->d_inp) return set_err(c, CRTHIP_E_ARG, "crthip_fieldpass_signal: no field-pass of that many fields went through this context", hipSuccess);
    HIPCHK(c, hipSetDevice(c->device));
    if (padded) *padded = c->last_lay.pitch != c->sd.hres;
    const int rc = crt_run_unpad(c, n, &c->last_lay, c->d_inp, d_inp_flat);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    return CRTHIP_OK;
}

int crthip_set_wide_lpw(crthip_ctx *c, int lpw)
{
    if (!c || (lpw != 0 && lpw != 8 && lpw != 16)) return CRTHIP_E_ARG;
    c->wide_lpw_env = lpw;
    return CRTHIP_OK;
}

int crthip_set_pixel_tile(crthip_ctx *c, int px)
{
    if (!c || (px != 0 && px != 16 && px != 32)) return CRTHIP_E_ARG;
    c->px_tile = px;
    c->ac_tile = px;
    return CRTHIP_OK;
}

/* The scratch of sequence mode, carved from the lazily grown block c->d_seq: set_first[n_sets + 1], tab[n] (first field of my set, my
 * set), inc[n_sets] (incoming hsync, vsync, rn) -- crthip_sequence_sets only; the phase entry points carve with n_sets == 0, which
 * leaves the three empty --, then guess[n] (int2), the changed flag, owner[n][outh] (u8), latest[n][outh] (int).  Who may trust
 * guess[] (c->seq_guess_n = the number of fields it holds finals for):
 *   - a reallocation synchronises the stream first (work in flight may still use the old block) and clears seq_guess_n;
 *   - a sets call clears seq_guess_n: its guess[] lies elsewhere in the block and holds other fields' pairs;
 *   - phase calls with the same n carve the same offsets (none depends on outh before owner), so a second crthip_seq_sync, or one
 *     behind crthip_seq_weave, finds guess[] where the previous one left it: the warm start across shards. */
static int seq_carve(crthip_ctx *c, int n_sets, int n, int outh, SetsScratch *sc)
{
    const auto up = [](size_t v) { return (v + 255) & ~(size_t) 255; };
    const size_t o_tab = up(sizeof(int) * ((size_t) n_sets + 1)), o_inc = o_tab + up(sizeof(int2) * (size_t) (n_sets ? n : 0));
    const size_t o_guess = o_inc + up(sizeof(int4) * (size_t) n_sets), o_changed = o_guess + up(sizeof(int2) * (size_t) n);
    const size_t o_owner = o_changed + 256, o_latest = o_owner + up((size_t) n * outh);
    const size_t need = o_latest + up(sizeof(int) * (size_t) n * outh);
    if (need > c->seq_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->d_seq) hipFree(c->d_seq);
        c->d_seq = 0; c->seq_cap = 0; c->seq_guess_n = 0;
        if (hipMalloc((void **) &c->d_seq, need) != hipSuccess) return set_err(c, CRTHIP_E_NOMEM, "hipMalloc sequence scratch", hipSuccess);
        c->seq_cap = need;
    }
    if (n_sets) c->seq_guess_n = 0;
    sc->set_first = (int *) c->d_seq;
    sc->tab = (int2 *) (c->d_seq + o_tab);
    sc->inc = (int4 *) (c->d_seq + o_inc);
    sc->guess = (int2 *) (c->d_seq + o_guess);
    sc->changed = (int *) (c->d_seq + o_changed);
    sc->owner = c->d_seq + o_owner;
    sc->latest = (int *) (c->d_seq + o_latest);
    return CRTHIP_OK;
}

static int seq_check(crthip_ctx *c, const crthip_params *p, int n)
{
    int rc = check_params(c, p, n);
    if (rc) return rc;
    if (c->system == CRTHIP_SYSTEM_NTSCVHS && !(p->flags & CRTHIP_F_VHS_LCG_NOISE) && !c->d_vhs_hist)
        return set_err(c, CRTHIP_E_ARG, "VHS: no generator histories bound (crthip_vhs_bind_history)", hipSuccess);
    if (p->flags & CRTHIP_F_NO_VSYNC)
        return set_err(c, CRTHIP_E_ARG, "sequence mode is not available for the CRT_DO_VSYNC 0 variant (its sync search reads the clean field)", hipSuccess);
    if (p->blend && (unsigned) p->outh + p->v_fac < (unsigned) c->sd.lines)
        return set_err(c, CRTHIP_E_ARG, "sequence mode with blend needs outh + v_fac >= CRT_LINES (one line per output row)", hipSuccess);
    if (p->out_bpp == 0) return set_err(c, CRTHIP_E_ARG, "sequence mode: unknown output pixel format", hipSuccess);
    int enc = check_encoder(c, p);
    if (enc != 0) return enc < 0 ? enc : set_err(c, CRTHIP_E_ARG, "sequence mode: unknown input pixel format", hipSuccess);
    return CRTHIP_OK;
}

/* What the single-set phases and crthip_sequence_sets have in common, each piece once. */

/* every field's noisy signal into c->d_inp, the states' generators already set.  vhs (the stock VHS build, whose noise follows
 * rand()): clean encode into c->d_analog, then the rand() noise (which also leaves rn), as in crthip_fieldpass; otherwise one fused
 * encode (noise fused, ccf presets) */
static int seq_signal(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride, crthip_state *d_state, bool vhs)
{
    if (!vhs) return crt_run_encoder(c, p, n, d_images, istride, c->d_inp, d_state, true, 1, false);
    crthip_params clean = *p;
    clean.noise = 0;
    const int rc = crt_run_encoder(c, &clean, n, d_images, istride, c->d_analog, d_state, true, 1, false);
    if (rc) return rc;
    return crt_run_noise(c, p, n, c->d_analog, c->d_inp, d_state, false);
}

/* sequence mode keeps the reference's flat signal layout: recorded once the signal of all n fields is enqueued */
static void seq_record_layout(crthip_ctx *c, int n) { c->last_lay = flat_layout(c); c->last_n = n; }

/* The sync fixed point over n fields whose signal is in c->d_inp (see the comment at the top).  Per pass: `load` enqueues the
 * caller's kernel that gives every field its initial pair -- the previous field's pair of sc.guess, or the incoming pair of its
 * set --, then the ccf preset (crt_ntsc.c:325-329), the sync chain, and k_seq_compare (guess <- finals, one flag for all fields).
 * After pass j the first j fields of every set are final, so more than `limit` = longest set + 1 passes cannot happen; `stuck` is
 * what the caller says if it does (say so instead of returning a half-converged chain). */
extern "C++" template <class Load>
int seq_converge(crthip_ctx *c, const crthip_params *p, int n, crthip_state *d_state, const SetsScratch &sc, int limit,
                 const char *stuck, int *passes_out, Load &&load)
{
    const crthip_params q = sync_blob(c, p, true);
    const dim3 gn((n + 63) / 64), b64(64);
    for (int passes = 1;; passes++) {
        HIPCHK(c, hipMemsetAsync(sc.changed, 0, sizeof(int), c->stream));
        load();
        int rc = crt_run_encoder_state(c, p, n, d_state);
        if (rc) return rc;
        rc = crt_run_sync(c, &q, n, c->d_inp, d_state, c->d_lines, 0);
        if (rc) return rc;
        hipLaunchKernelGGL(k_seq_compare, gn, b64, 0, c->stream, n, d_state, sc.guess, sc.changed);
        int flag = 0;
        HIPCHK(c, hipMemcpyAsync(&flag, sc.changed, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!flag) {
            if (passes_out) *passes_out = passes;
            return CRTHIP_OK;
        }
        if (passes > limit) return set_err(c, CRTHIP_E_HIP, stuck, hipSuccess);
    }
}

/* the row tables of the last phase from c->d_lines, for the sets of sc.set_first or (n_sets == 0) the single range [0, n).  With
 * blend: sc.latest = rowsrc (k_seq_rowsrc, -1 where nobody wrote); without: sc.owner, then sc.latest = the latest writer per set */
static int seq_row_tables(crthip_ctx *c, const crthip_params *p, int n_sets, int n, const SetsScratch &sc)
{
    const int outh = p->outh;
    const dim3 gl((n * c->sd.lines + 255) / 256), b256(256);
    if (p->blend) {
        HIPCHK(c, hipMemsetAsync(sc.latest, 0xff, sizeof(int) * (size_t) n * outh, c->stream));       /* -1 everywhere */
        hipLaunchKernelGGL(k_seq_rowsrc, gl, b256, 0, c->stream, n, c->sd.lines, outh, c->d_lines, sc.latest);
        return CRTHIP_OK;
    }
    HIPCHK(c, hipMemsetAsync(sc.owner, 0, (size_t) n * outh, c->stream));
    hipLaunchKernelGGL(k_seq_rows, gl, b256, 0, c->stream, n, c->sd.lines, outh, c->d_lines, sc.owner);
    if (n_sets) hipLaunchKernelGGL(k_sets_latest, dim3((n_sets * outh + 63) / 64), dim3(64), 0, c->stream, n_sets, outh, sc.set_first, sc.owner, sc.latest);
    else hipLaunchKernelGGL(k_seq_latest, dim3((outh + 63) / 64), dim3(64), 0, c->stream, n, outh, sc.owner, sc.latest);
    return CRTHIP_OK;
}

/* The phases.  Each *_body runs with the blob it is given: the caller's p, or -- crthip_sequence_knobs, or a phase entry point with
 * bound records -- the blob of call_begin, whose KN kernels then read noise, monitor hue and saturation (and bloom's max_e) per field.  Nothing of sequence mode's own arithmetic changes with that: rn advances once per sample whatever
 * the gain (crt_core.c:358-366, so k_seq_rn's closed form holds), and the sync fixed point reads only the noisy signal. */
/* phase 1: the noise generator of every field in closed form, all fields encoded in parallel (noise fused) */
static int seq_encode_body(crthip_ctx *c, const crthip_params *p, int n, int first_index, int rn0,
                      const void *d_images, size_t istride, crthip_state *d_state)
{
    int rc = seq_check(c, p, n);
    if (rc) return rc;
    if (!d_images || !d_state || first_index < 0) return CRTHIP_E_ARG;
    if ((rc = check_images(c, p, d_images, istride)) || (rc = CHECK_WORD(c, d_state))) return rc;
    const bool vhs = c->system == CRTHIP_SYSTEM_NTSCVHS && !(p->flags & CRTHIP_F_VHS_LCG_NOISE);
    if (vhs && first_index != 0 && !c->vhs_prechained)
        return set_err(c, CRTHIP_E_ARG, "VHS: a video shares ONE rand() stream; its fields cannot start in the middle (first_index != 0)", hipSuccess);
    HIPCHK(c, hipSetDevice(c->device));
    c->seq_guess_n = 0;                                    /* a new video: no warm start for the sync chain */
    rc = encoder_ready(c, p, n, true);                     /* (the layout is recorded below, once the signal is enqueued) */
    if (rc) return rc;
    if (!vhs) {
        hipLaunchKernelGGL(k_seq_rn, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, d_state, c->whole_field,
                           (unsigned) first_index, (unsigned) rn0);
    } else if (!c->vhs_prechained) {
        /* the fields share one rand() stream: run the chain ahead (k_vhs_chain: hist[k] = generator at the start
         * of field k, aberration heights drawn in-stream if asked), after which every field is independent */
        rc = crt_run_vhs_chain(c, n, d_state, (p->flags & CRTHIP_F_VHS_DRAW_ABERRATION) != 0);
        if (rc) return rc;
    }
    rc = seq_signal(c, p, n, d_images, istride, d_state, vhs);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    seq_record_layout(c, n);
    return CRTHIP_OK;
}

/* phase 2: the sync chain.  Field k starts from field k-1's final (hsync, vsync), field 0 from (hsync_in, vsync_in);
 * solved as a fixed point over ALL fields in parallel (see the comment at the top).  Called again with another
 * incoming pair (a video cut over several shards: the predecessor's final state became known) it restarts from the
 * finals of the previous call, so only the fields whose state really depends on the incoming pair are recomputed
 * in more than one pass. */
static int seq_sync_body(crthip_ctx *c, const crthip_params *p, int n, crthip_state *d_state, int hsync_in, int vsync_in,
                         int *hsync_out, int *vsync_out, int *passes_out)
{
    int rc = seq_check(c, p, n);
    if (rc) return rc;
    if (!d_state || n > c->cap_fields) return CRTHIP_E_ARG;
    if ((rc = CHECK_WORD(c, d_state))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SetsScratch sc;
    rc = seq_carve(c, 0, n, p->outh, &sc);
    if (rc) return rc;
    if (c->seq_guess_n != n) {
        /* first guess: nobody's sync state moves */
        int2 *h = (int2 *) malloc(sizeof(int2) * (size_t) n);
        if (!h) return CRTHIP_E_NOMEM;
        for (int k = 0; k < n; k++) h[k] = make_int2(hsync_in, vsync_in);
        hipError_t e = hipMemcpyAsync(sc.guess, h, sizeof(int2) * (size_t) n, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        free(h);
        HIPCHK(c, e);
        c->seq_guess_n = n;
    }
    rc = seq_converge(c, p, n, d_state, sc, n + 1, "crthip_seq_sync: the sync chain over the fields did not converge", passes_out,
                      [&] {
        hipLaunchKernelGGL(k_seq_load, dim3((n + 63) / 64), dim3(64), 0, c->stream, n, d_state, sc.guess, make_int2(hsync_in, vsync_in));
    });
    if (rc) return rc;
    if (hsync_out || vsync_out) {
        int hv[2];
        HIPCHK(c, hipMemcpyAsync(hv, &d_state[n - 1].hsync, sizeof(hv), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (hsync_out) *hsync_out = hv[0];
        if (vsync_out) *vsync_out = hv[1];
    }
    return CRTHIP_OK;
}

/* phase 3: rn after each field, all fields decoded in parallel (without blend: phase 4 folds the fields) */
static int seq_decode_body(crthip_ctx *c, const crthip_params *p, int n, void *d_out, size_t ostride, crthip_state *d_state)
{
    int rc = seq_check(c, p, n);
    if (rc) return rc;
    if (!d_out || !d_state || n > c->cap_fields) return CRTHIP_E_ARG;
    if ((rc = check_out(c, p, d_out, ostride)) || (rc = CHECK_WORD(c, d_state))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->system != CRTHIP_SYSTEM_NTSCVHS || (p->flags & CRTHIP_F_VHS_LCG_NOISE)) crt_run_advance_rn(c, n, d_state);
    crthip_params pb = *p;
    pb.blend = 0;
    rc = crt_run_decode(c, &pb, n, c->d_inp, c->d_lines, d_out, ostride);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    return CRTHIP_OK;
}

/* phase 4: image k = the single output buffer as it stands after field k.  d_out_init = the buffer before the shard's
 * first field (NULL = zeros).  Without blend: rows a field does not write come from the latest earlier field that
 * wrote them, or from d_out_init; patch_only != 0 revisits only the latter (the images were woven before with a
 * placeholder init: a later shard of a video whose predecessor's last picture arrives late).  With blend: the
 * recurrence over the fields, one pass per field in order (patch_only is not available). */
int crthip_seq_weave(crthip_ctx *c, const crthip_params *p, int n, void *d_out, size_t ostride, const void *d_out_init,
                     int patch_only)
{
    int rc = seq_check(c, p, n);
    if (rc) return rc;
    if (!d_out || n > c->cap_fields || (p->blend && patch_only)) return CRTHIP_E_ARG;
    if ((rc = check_out(c, p, d_out, ostride, d_out_init, 0))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SetsScratch sc;
    rc = seq_carve(c, 0, n, p->outh, &sc);
    if (rc) return rc;
    if (!patch_only && (rc = seq_row_tables(c, p, 0, n, sc))) return rc;      /* (a revisit finds sc.latest as the first visit left it) */
    const int outh = p->outh;
    const size_t pitch = (size_t) p->outw * p->out_bpp;
    const unsigned alpha = out_alpha_mask(p);
    unsigned char *out = (unsigned char *) d_out;
    const unsigned char *init = (const unsigned char *) d_out_init;
    dispatch_phosphor(phosphor_mode(p), [&](auto ph) {
        constexpr int PH = decltype(ph)::value;
        if (p->blend) {
            for (int k = 0; k < n; k++)
                hipLaunchKernelGGL(k_seq_blend_step<PH>, dim3((unsigned) outh), dim3(256), 0, c->stream, k, outh, pitch, out, ostride, init, sc.latest, alpha);
        } else {
            hipLaunchKernelGGL(k_seq_weave<PH>, dim3((unsigned) n * (unsigned) outh), dim3(256), 0, c->stream, n, outh, pitch, out, ostride, init,
                               sc.latest, patch_only, alpha);
        }
    });
    HIPCHK(c, hipGetLastError());
    return CRTHIP_OK;
}

int crthip_vhs_chain(crthip_ctx *c, int n, crthip_state *d_state, int draw_aberration)
{
    if (!c || n <= 0 || !d_state || c->system != CRTHIP_SYSTEM_NTSCVHS) return CRTHIP_E_ARG;
    if (CHECK_WORD(c, d_state)) return CRTHIP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = crt_run_vhs_chain(c, n, d_state, draw_aberration);
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    return CRTHIP_OK;
}

int crthip_seq_vhs_prechained(crthip_ctx *c, int on)
{
    if (!c || c->system != CRTHIP_SYSTEM_NTSCVHS) return CRTHIP_E_ARG;
    c->vhs_prechained = on != 0;
    return CRTHIP_OK;
}

int crthip_seq_bind_knobs(crthip_ctx *c, const crthip_knob_rec *d_recs, const crthip_knobs_env *env)
{
    if (!c) return CRTHIP_E_ARG;
    if (!d_recs && !env) { c->seq_knob_recs = nullptr; return CRTHIP_OK; }
    if (!d_recs || !env) return set_err(c, CRTHIP_E_ARG, "crthip_seq_bind_knobs: records and env go together ((NULL, NULL) unbinds)", hipSuccess);
    if (CHECK_WORD(c, d_recs)) return CRTHIP_E_ARG;
    const int rc = knobs_env_check(c, env, 0);
    if (rc) return rc;
    c->seq_knob_recs = d_recs;
    c->seq_knob_env = *env;
    return CRTHIP_OK;
}

/* The encoder's level records for the knob entry points (crt_hip.h, LEVEL KNOBS): kept until unbound; checked against each call's n,
 * env and system by call_begin.  Nothing is copied or launched here. */
int crthip_bind_levels(crthip_ctx *c, const crthip_level_rec *d_levs, const crthip_levels_env *lenv)
{
    if (!c) return CRTHIP_E_ARG;
    if (!d_levs && !lenv) { c->lev_recs = nullptr; return CRTHIP_OK; }
    if (!d_levs || !lenv) return set_err(c, CRTHIP_E_ARG, "crthip_bind_levels: records and env go together ((NULL, NULL) unbinds)", hipSuccess);
    if (check_word(c, d_levs, "d_levs needs 4-byte alignment")) return CRTHIP_E_ARG;
    if (lenv->magic != CRTHIP_LEVELS_MAGIC) return set_err(c, CRTHIP_E_ARG, "levels: lenv does not come from crthip_knobs_prepare7", hipSuccess);
    if (lenv->n <= 0 || lenv->white_abs_max < 0 || lenv->ire_base_abs_max < 0) return set_err(c, CRTHIP_E_ARG, "levels: lenv bounds", hipSuccess);
    c->lev_recs = d_levs;
    c->lev_env = *lenv;
    return CRTHIP_OK;
}

/* The encoder's hue records for the knob entry points (crt_hip.h, HUE KNOB): as crthip_bind_levels. */
int crthip_bind_hues(crthip_ctx *c, const crthip_hue_rec *d_hues, const crthip_hues_env *henv)
{
    if (!c) return CRTHIP_E_ARG;
    if (!d_hues && !henv) { c->hue_recs = nullptr; return CRTHIP_OK; }
    if (!d_hues || !henv) return set_err(c, CRTHIP_E_ARG, "crthip_bind_hues: records and env go together ((NULL, NULL) unbinds)", hipSuccess);
    if (check_word(c, d_hues, "d_hues needs 4-byte alignment")) return CRTHIP_E_ARG;
    if (henv->magic != CRTHIP_HUES_MAGIC) return set_err(c, CRTHIP_E_ARG, "hues: henv does not come from crthip_knobs_prepare8", hipSuccess);
    if (henv->n <= 0) return set_err(c, CRTHIP_E_ARG, "hues: henv bounds", hipSuccess);
    c->hue_recs = d_hues;
    c->hue_env = *henv;
    return CRTHIP_OK;
}

/* The phase entry points run with the records crthip_seq_bind_knobs has bound (call_begin, REC_SEQ_BOUND); nothing bound: exactly the
 * uniform phase */
int crthip_seq_encode(crthip_ctx *c, const crthip_params *p, int n, int first_index, int rn0,
                      const void *d_images, size_t istride, crthip_state *d_state)
{
    return with_records(c, p, n, REC_SEQ_BOUND, nullptr, nullptr, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return seq_encode_body(c, q, n, first_index, rn0, d_images, istride, d_state); });
}

int crthip_seq_sync(crthip_ctx *c, const crthip_params *p, int n, crthip_state *d_state, int hsync_in, int vsync_in,
                    int *hsync_out, int *vsync_out, int *passes_out)
{
    return with_records(c, p, n, REC_SEQ_BOUND, nullptr, nullptr, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return seq_sync_body(c, q, n, d_state, hsync_in, vsync_in, hsync_out, vsync_out, passes_out); });
}

int crthip_seq_decode(crthip_ctx *c, const crthip_params *p, int n, void *d_out, size_t ostride, crthip_state *d_state)
{
    return with_records(c, p, n, REC_SEQ_BOUND, nullptr, nullptr, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return seq_decode_body(c, q, n, d_out, ostride, d_state); });
}

/* crthip_sequence and crthip_sequence_knobs, on the blob of the call's records (call_begin) */
static int sequence_body(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                         void *d_out, size_t ostride, const void *d_out_init, crthip_state *d_state, int *passes_out)
{
    int rc;
    if (!d_images || !d_out || !d_state) return CRTHIP_E_ARG;
    if ((rc = check_images(c, p, d_images, istride)) || (rc = check_out(c, p, d_out, ostride, d_out_init, 0)) || (rc = CHECK_WORD(c, d_state))) return rc;
    if (p->out_bpp == 0) return CRTHIP_OK;                /* unknown output format: like crt_demodulate, nothing happens (crt_core.c:312-315) */
    HIPCHK(c, hipSetDevice(c->device));
    crthip_state first;
    HIPCHK(c, hipMemcpyAsync(&first, d_state, sizeof(first), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rc = seq_encode_body(c, p, n, 0, first.rn, d_images, istride, d_state);
    if (rc) return rc;
    rc = seq_sync_body(c, p, n, d_state, first.hsync, first.vsync, nullptr, nullptr, passes_out);
    if (rc) return rc;
    rc = seq_decode_body(c, p, n, d_out, ostride, d_state);
    if (rc) return rc;
    return crthip_seq_weave(c, p, n, d_out, ostride, d_out_init, 0);
}

int crthip_sequence(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                    void *d_out, size_t ostride, const void *d_out_init, crthip_state *d_state, int *passes_out)
{
    return with_records(c, p, n, 0, nullptr, nullptr, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return sequence_body(c, q, n, d_images, istride, d_out, ostride, d_out_init, d_state, passes_out); });
}

int crthip_sequence_knobs(crthip_ctx *c, const crthip_params *p, int n, const void *d_images, size_t istride,
                          void *d_out, size_t ostride, const void *d_out_init, crthip_state *d_state,
                          const crthip_knob_rec *d_recs, const crthip_knobs_env *env, int *passes_out)
{
    return with_records(c, p, n, REC_KNOBS, d_recs, env, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return sequence_body(c, q, n, d_images, istride, d_out, ostride, d_out_init, d_state, passes_out); });
}

/* crthip_sequence_sets* behind its checks (sequence_sets_body), on the blob of the call's records: n fields in n_sets sets, the
 * longest of max_len fields; streams = CRTHIP_F_VHS_SET_STREAMS */
static int sequence_sets_run(crthip_ctx *c, const crthip_params *p, int n_sets, const int *set_first, int n, int max_len, bool streams,
                             const void *d_images, size_t istride, void *d_out, size_t ostride,
                             const void *d_out_init, size_t out_init_stride, crthip_state *d_state, int *passes_out)
{
    HIPCHK(c, hipSetDevice(c->device));
    SetsScratch sc;
    int rc = seq_carve(c, n_sets, n, p->outh, &sc);
    if (rc) return rc;
    /* the set table: built here, uploaded once (the host copy belongs to the context: it outlives the copy) */
    const size_t tab_ints = (size_t) n_sets + 1, host_ints = ((tab_ints + 63) & ~(size_t) 63) + 2 * (size_t) n;
    if (host_ints > c->seq_sets_host_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        free(c->seq_sets_host);
        c->seq_sets_host_cap = 0;
        c->seq_sets_host = (int *) malloc(sizeof(int) * host_ints);
        if (!c->seq_sets_host) return set_err(c, CRTHIP_E_NOMEM, "crthip_sequence_sets: set table", hipSuccess);
        c->seq_sets_host_cap = host_ints;
    }
    int *h_first = c->seq_sets_host, *h_tab = c->seq_sets_host + ((tab_ints + 63) & ~(size_t) 63);
    for (int s = 0; s <= n_sets; s++) h_first[s] = set_first[s];
    for (int s = 0; s < n_sets; s++)
        for (int k = set_first[s]; k < set_first[s + 1]; k++) { h_tab[2 * k] = set_first[s]; h_tab[2 * k + 1] = s; }
    HIPCHK(c, hipMemcpyAsync(sc.set_first, h_first, sizeof(int) * tab_ints, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(sc.tab, h_tab, sizeof(int2) * (size_t) n, hipMemcpyHostToDevice, c->stream));
    /* as crthip_seq_encode: the workspace, the encoder's tables, and the flat signal layout (recorded once the whole call is enqueued) */
    rc = encoder_ready(c, p, n, true);
    if (rc) return rc;
    const dim3 gn((n + 63) / 64), gs((n_sets + 63) / 64), b64(64);
    hipLaunchKernelGGL(k_sets_incoming, gs, b64, 0, c->stream, n_sets, sc.set_first, d_state, sc.inc);
    if (streams) {
        /* every set's chain ahead of everything else (k_vhs_chain<SETS>: one wave per set, hist[k] = the generator at the start of
         * field k, the aberration heights drawn in-stream if asked; the rand() noise then leaves rn and the histories after every field) */
        hipLaunchKernelGGL(k_sets_guess, gn, b64, 0, c->stream, n, sc.tab, sc.inc, sc.guess);
        rc = crt_run_vhs_chain(c, n, d_state, (p->flags & CRTHIP_F_VHS_DRAW_ABERRATION) != 0, n_sets, sc.set_first);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(k_sets_rn, gn, b64, 0, c->stream, n, d_state, sc.tab, sc.inc, sc.guess, c->whole_field);
    }
    rc = seq_signal(c, p, n, d_images, istride, d_state, streams);
    if (rc) return rc;
    /* the joint fixed point: one flag for all sets */
    rc = seq_converge(c, p, n, d_state, sc, max_len + 1, "crthip_sequence_sets: the sync chain over the fields did not converge", passes_out,
                      [&] {
        hipLaunchKernelGGL(k_sets_load, gn, b64, 0, c->stream, n, d_state, sc.tab, sc.inc, sc.guess);
    });
    if (rc) return rc;
    if (!streams) crt_run_advance_rn(c, n, d_state);
    crthip_params pb = *p;
    pb.blend = 0;
    rc = crt_run_decode(c, &pb, n, c->d_inp, c->d_lines, d_out, ostride);
    if (rc) return rc;
    rc = seq_row_tables(c, p, n_sets, n, sc);
    if (rc) return rc;
    dispatch_phosphor(phosphor_mode(p), [&](auto ph) {
        launch_sets_weave<decltype(ph)::value>(c, p, n_sets, n, max_len, (unsigned char *) d_out, ostride, (const unsigned char *) d_out_init,
                                               out_init_stride, sc);
    });
    HIPCHK(c, hipGetLastError());
    seq_record_layout(c, n);
    return CRTHIP_OK;
}

/* crthip_sequence_sets, and (kinds = REC_KNOBS) crthip_sequence_sets_knobs: what a sets call checks of its own, then the run with the
 * call's records (call_begin over all n fields: record k belongs to field k of the batch, whatever its set) */
static int sequence_sets_body(crthip_ctx *c, const crthip_params *p, int n_sets, const int *set_first,
                              const void *d_images, size_t istride, void *d_out, size_t ostride,
                              const void *d_out_init, size_t out_init_stride, crthip_state *d_state, int *passes_out,
                              int kinds, const crthip_knob_rec *d_recs, const crthip_knobs_env *env)
{
    if (!c || !p) return CRTHIP_E_ARG;
    if (n_sets <= 0 || !set_first) return set_err(c, CRTHIP_E_ARG, "crthip_sequence_sets: no sets", hipSuccess);
    if (set_first[0] != 0) return set_err(c, CRTHIP_E_ARG, "crthip_sequence_sets: set_first[0] must be 0", hipSuccess);
    int max_len = 0;
    for (int s = 0; s < n_sets; s++) {
        if (set_first[s + 1] <= set_first[s])
            return set_err(c, CRTHIP_E_ARG, "crthip_sequence_sets: set_first must be strictly ascending (every set has at least one field)", hipSuccess);
        if (set_first[s + 1] - set_first[s] > max_len) max_len = set_first[s + 1] - set_first[s];
    }
    const int n = set_first[n_sets];
    int rc = check_params(c, p, n);
    if (rc) return rc;
    if (!d_images || !d_out || !d_state) return CRTHIP_E_ARG;
    if ((rc = check_images(c, p, d_images, istride)) || (rc = check_out(c, p, d_out, ostride, d_out_init, out_init_stride)) || (rc = CHECK_WORD(c, d_state)) || (rc = CHECK_WORD(c, d_recs))) return rc;
    if (p->out_bpp == 0) return CRTHIP_OK;                /* as crthip_sequence */
    /* CRTHIP_F_VHS_SET_STREAMS: every set owns one rand() stream (hist[set_first[s]] = its generator before its first field) */
    const bool streams = (p->flags & CRTHIP_F_VHS_SET_STREAMS) != 0;
    if (streams && (c->system != CRTHIP_SYSTEM_NTSCVHS || (p->flags & CRTHIP_F_VHS_LCG_NOISE)))
        return set_err(c, CRTHIP_E_ARG, "crthip_sequence_sets: CRTHIP_F_VHS_SET_STREAMS is for the VHS build with rand() noise "
                                        "(CRTHIP_SYSTEM_NTSCVHS without CRTHIP_F_VHS_LCG_NOISE)", hipSuccess);
    if (!streams && c->system == CRTHIP_SYSTEM_NTSCVHS && !(p->flags & CRTHIP_F_VHS_LCG_NOISE))
        return set_err(c, CRTHIP_E_ARG, "crthip_sequence_sets: the VHS build with rand() noise is not available (every set would own a rand() stream); "
                                        "use CRTHIP_F_VHS_LCG_NOISE or crthip_sequence per set", hipSuccess);
    if (!streams && c->system == CRTHIP_SYSTEM_NTSCVHS && (p->flags & CRTHIP_F_VHS_DRAW_ABERRATION))
        return set_err(c, CRTHIP_E_ARG, "crthip_sequence_sets: CRTHIP_F_VHS_DRAW_ABERRATION draws from the rand() stream; give the heights in d_state[k].aux", hipSuccess);
    rc = seq_check(c, p, n);                              /* (streams: also that a history array is bound) */
    if (rc) return rc;
    return with_records(c, p, n, kinds, d_recs, env, nullptr, nullptr, nullptr, [&](const crthip_params *q) {
        return sequence_sets_run(c, q, n_sets, set_first, n, max_len, streams, d_images, istride, d_out, ostride, d_out_init, out_init_stride,
                                 d_state, passes_out); });
}

int crthip_sequence_sets(crthip_ctx *c, const crthip_params *p, int n_sets, const int *set_first,
                         const void *d_images, size_t istride, void *d_out, size_t ostride,
                         const void *d_out_init, size_t out_init_stride, crthip_state *d_state, int *passes_out)
{
    return sequence_sets_body(c, p, n_sets, set_first, d_images, istride, d_out, ostride, d_out_init, out_init_stride, d_state, passes_out,
                              0, nullptr, nullptr);
}

int crthip_sequence_sets_knobs(crthip_ctx *c, const crthip_params *p, int n_sets, const int *set_first,
                               const void *d_images, size_t istride, void *d_out, size_t ostride,
                               const void *d_out_init, size_t out_init_stride, crthip_state *d_state,
                               const crthip_knob_rec *d_recs, const crthip_knobs_env *env, int *passes_out)
{
    if (!c || !p) return CRTHIP_E_ARG;
    if (!d_recs || !env) return set_err(c, CRTHIP_E_ARG, "crthip_sequence_sets_knobs: no records / env", hipSuccess);
    return sequence_sets_body(c, p, n_sets, set_first, d_images, istride, d_out, ostride, d_out_init, out_init_stride, d_state, passes_out,
                              REC_KNOBS, d_recs, env);
}

int crthip_set_shape(crthip_ctx *c, int shape)
{
    if (!c || shape < 0 || shape > 2) return CRTHIP_E_ARG;
    c->shape = shape;
    return CRTHIP_OK;
}

int crthip_set_overlap(crthip_ctx *c, int chunks)
{
    if (!c || chunks < 0 || chunks > CRTHIP_MAX_CHUNKS) return CRTHIP_E_ARG;
    c->overlap_chunks = chunks;
    return CRTHIP_OK;
}

int crthip_vhs_bind_history(crthip_ctx *c, unsigned *d_hist)
{
    if (!c || c->system != CRTHIP_SYSTEM_NTSCVHS) return CRTHIP_E_ARG;
    if (CHECK_WORD(c, d_hist)) return CRTHIP_E_ARG;
    c->d_vhs_hist = d_hist;
    return CRTHIP_OK;
}

int crthip_set_exact(crthip_ctx *c, int on)
{
    if (!c) return CRTHIP_E_ARG;
    c->force_exact = on == 1;
    c->no_tier0 = on == 2;      /* 2: allow the 24-bit tier but not the 64-bit-mad ones */
    c->no_loskip = on == 3;     /* 3: allow the 64-bit-mad tier but keep the I/Q low cascades */
    return CRTHIP_OK;
}

int crthip_profile_enable(crthip_ctx *c, int on)
{
    if (!c) return CRTHIP_E_ARG;
    c->prof = on != 0;
    return CRTHIP_OK;
}

int crthip_profile_read(crthip_ctx *c, double total_ms[CRTHIP_K_COUNT], int launches[CRTHIP_K_COUNT])
{
    if (!c) return CRTHIP_E_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < c->npend; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->pend[i].a, c->pend[i].b) == hipSuccess) {
            c->prof_ms[c->pend[i].k] += ms;
            c->prof_n[c->pend[i].k]++;
        }
        hipEventDestroy(c->pend[i].a);
        hipEventDestroy(c->pend[i].b);
    }
    c->npend = 0;
    for (int k = 0; k < CRTHIP_K_COUNT; k++) {
        if (total_ms) total_ms[k] = c->prof_ms[k];
        if (launches) launches[k] = c->prof_n[k];
        c->prof_ms[k] = 0.0;
        c->prof_n[k] = 0;
    }
    return CRTHIP_OK;
}

void *crthip_malloc(crthip_ctx *c, size_t bytes)
{
    void *p = 0;
    if (!c || hipSetDevice(c->device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) return 0;
    return p;
}

void crthip_free(crthip_ctx *c, void *d)
{
    if (c && d) { hipSetDevice(c->device); hipStreamSynchronize(c->stream); hipFree(d); }
}

int crthip_upload(crthip_ctx *c, void *d, const void *h, size_t bytes)
{
    if (!c) return CRTHIP_E_ARG;
    HIPCHK(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CRTHIP_OK;
}

int crthip_download(crthip_ctx *c, void *h, const void *d, size_t bytes)
{
    if (!c) return CRTHIP_E_ARG;
    HIPCHK(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return CRTHIP_OK;
}

int crthip_host_register(crthip_ctx *c, void *h, size_t bytes)
{
    if (!c || !h || !bytes) return CRTHIP_E_ARG;
    if (hipHostRegister(h, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void) hipGetLastError();
        return CRTHIP_E_HIP;
    }
    return CRTHIP_OK;
}

int crthip_host_unregister(crthip_ctx *c, void *h)
{
    if (!c || !h) return CRTHIP_E_ARG;
    if (hipHostUnregister(h) != hipSuccess) {
        (void) hipGetLastError();
        return CRTHIP_E_HIP;
    }
    return CRTHIP_OK;
}

int crthip_memset(crthip_ctx *c, void *d, int value, size_t bytes)
{
    if (!c) return CRTHIP_E_ARG;
    HIPCHK(c, hipMemsetAsync(d, value, bytes, c->stream));
    return CRTHIP_OK;
}

}  /* extern "C" */

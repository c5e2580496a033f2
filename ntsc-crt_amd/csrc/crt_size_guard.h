/*
 * The address guard of a sizes call (crthip_fieldpass_sizes / crthip_stills_sizes; k_active's SZ instantiations, crt_encode.hip).
 * Plain C++ without a HIP header, so that the very code the kernels run is also compiled for the host and run over hostile
 * records there (tests/test_sizes_cpu.py): a guard's failure on the device would be a fault, which no test may look for.
 */
#ifndef CRT_SIZE_GUARD_H
#define CRT_SIZE_GUARD_H

#include "crt_hip.h"

#if defined(__HIPCC__)
#define CRT_GUARD_FN __host__ __device__ __forceinline__
#else
#define CRT_GUARD_FN static inline
#endif

/* What a wavefront does with its field's record before it forms an address from it (wave-uniform throughout).  The host has seen the
 * env, never the records: they are the caller's device memory and may be rewritten between two replays of a graph.  A record whose
 * image does not lie inside [images, images + extent), or that the instantiation cannot walk (the cooperative tiles move 16-byte
 * pieces of dword pixels: w >= 4, offset a multiple of 4), is replaced by the smallest image such a kernel reads, at offset 0 --
 * which the host has checked the extent for (call_begin, crt_host.hip).  The samples are then unspecified; the accesses are not.
 * col_step is NOT checked here: whatever it holds, every column it produces goes through size_col_clamped. */
struct size_view { int w, h; unsigned long long off, cstep; };
CRT_GUARD_FN size_view size_rec_checked(const crthip_size_rec &r, int in_bpp, bool spare_row, bool tiles, unsigned long long extent)
{
    size_view v;
    v.w = r.w; v.h = r.h;
    v.off = ((unsigned long long) r.off_hi << 32) | r.off_lo;
    v.cstep = ((unsigned long long) r.col_step_hi << 32) | r.col_step_lo;
    const int w_least = tiles ? 4 : 1;
    bool ok = v.w >= w_least && v.h >= 1 && v.off <= extent && !(tiles && ((v.off & 3) || v.w >= (1 << 29)));   /* (tiles: w * 4 is an int) */
    if (ok) {
        /* (h + 1) * w * bpp can pass 2^64 (2^31 * 2^31 * 4): the multiplication says so */
        const unsigned long long row_bytes = (unsigned long long) (unsigned) v.w * (unsigned) in_bpp;
        const unsigned long long rows = (unsigned long long) (unsigned) v.h + (spare_row ? 1u : 0u);
        unsigned long long bytes;
        ok = !__builtin_mul_overflow(rows, row_bytes, &bytes) && bytes <= extent - v.off;
    }
    if (!ok) { v.w = w_least; v.h = 1; v.off = 0; v.cstep = 0; }
    return v;
}

/* The source column of a sample, (cpos >> 32) with cpos = x * col_step in wrapping 64-bit arithmetic: ANY 32-bit pattern when the
 * record's col_step is not the one crthip_sizes_prepare made -- negative as an int from col_step_hi = 0x80000000 on, or after a few
 * hundred samples from a few millions on.  One unsigned compare bounds it on both sides: a column in [0, w) stays, everything else
 * (too large OR negative) becomes w - 1.  A no-op for the records of crthip_sizes_prepare ((x * col_step) >> 32 == x * w / destw < w
 * for x < destw; the up to three samples behind the line end that the tile path computes and never stores read column w - 1). */
CRT_GUARD_FN int size_col_clamped(int col, int w)
{
    return (unsigned) col < (unsigned) w ? col : w - 1;
}

#endif

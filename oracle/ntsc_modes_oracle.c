/*
 * ntsc_modes_oracle.c -- TEST INFRASTRUCTURE ONLY (see ntsc_modes_oracle.h).
 *
 * The chain of ntsc_oracle.c as one body (ntsc_modes_body.h) compiled for double and for float planes; the four
 * flavours are that body with a run-time choice of what the quantising operations and the poles do.
 * MUST be compiled with -ffp-contract=off.
 */
#include "ntsc_modes_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#define NTSC_RATE ((315000000.00 * 4) / 88)

enum { MODES_POLE_ORACLE = 0,   /* s*a + (p - p*a): the reference's LowpassFilter                 */
       MODES_POLE_DIFF = 1,     /* p + a*(s - p), two roundings                                   */
       MODES_POLE_FMA = 2 };    /* fma(a, s - p, p): what the float kernels execute               */

typedef struct modes_cfg {
    int keep_int;       /* 1: the q_*() operations quantise as the oracle does; 0: they do not    */
    int pole;
    double luma_bias;
} modes_cfg;

static unsigned scanline_phase(const ntscsim_params *p, unsigned y, uint64_t fieldno)
{
    unsigned off = (unsigned)p->video_scanline_phase_shift_offset;
    if (p->video_scanline_phase_shift == 90)
        return (unsigned)((fieldno + off + (y >> 1)) & 3);
    if (p->video_scanline_phase_shift == 180)
        return (unsigned)((((fieldno + y) & 2) + off) & 3);
    if (p->video_scanline_phase_shift == 270)
        return (unsigned)((fieldno + off - (y >> 1)) & 3);
    return off & 3;
}

#define REAL double
#define SFX(n) n##_d
#define RFMA(a, b, c) fma((a), (b), (c))
#include "ntsc_modes_body.h"
#undef REAL
#undef SFX
#undef RFMA

#define REAL float
#define SFX(n) n##_f
#define RFMA(a, b, c) fmaf((a), (b), (c))
#include "ntsc_modes_body.h"
#undef REAL
#undef SFX
#undef RFMA

int ntsc_modes_exact64(const ntscsim_params *p, ntsc_oracle_rng *g,
                       const uint8_t *src, int src_linesize, int src_interlaced, int src_tff,
                       uint8_t *dst, int dst_linesize, int W, int H, unsigned field, uint64_t fieldno,
                       const ntsc_oracle_taps *taps)
{
    const modes_cfg m = { 1, MODES_POLE_ORACLE, 0.0 };
    return modes_field_d(&m, p, g, src, src_linesize, src_interlaced, src_tff, dst, dst_linesize, W, H, field, fieldno,
                         taps, NULL);
}

int ntsc_modes_fast32(const ntscsim_params *p, ntsc_oracle_rng *g,
                      const uint8_t *src, int src_linesize, int src_interlaced, int src_tff,
                      uint8_t *dst, int dst_linesize, int W, int H, unsigned field, uint64_t fieldno,
                      const ntsc_oracle_taps *taps)
{
    const modes_cfg m = { 1, MODES_POLE_FMA, 0.0 };
    return modes_field_f(&m, p, g, src, src_linesize, src_interlaced, src_tff, dst, dst_linesize, W, H, field, fieldno,
                         taps, NULL);
}

int ntsc_modes_real64(const ntscsim_params *p, ntsc_oracle_rng *g,
                      const uint8_t *src, int src_linesize, int src_interlaced, int src_tff,
                      uint8_t *dst, int dst_linesize, int W, int H, unsigned field, uint64_t fieldno,
                      double luma_bias, const ntsc_modes_planes *out)
{
    const modes_cfg m = { 0, MODES_POLE_DIFF, luma_bias };
    return modes_field_d(&m, p, g, src, src_linesize, src_interlaced, src_tff, dst, dst_linesize, W, H, field, fieldno,
                         NULL, out);
}

int ntsc_modes_real32(const ntscsim_params *p, ntsc_oracle_rng *g,
                      const uint8_t *src, int src_linesize, int src_interlaced, int src_tff,
                      uint8_t *dst, int dst_linesize, int W, int H, unsigned field, uint64_t fieldno,
                      double luma_bias, const ntsc_modes_planes *out)
{
    const modes_cfg m = { 0, MODES_POLE_FMA, luma_bias };
    return modes_field_f(&m, p, g, src, src_linesize, src_interlaced, src_tff, dst, dst_linesize, W, H, field, fieldno,
                         NULL, out);
}

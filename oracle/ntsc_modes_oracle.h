/*
 * ntsc_modes_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * ONE model of the per-field chain (ntsc_oracle_field(), restated stage for stage in ntsc_modes_body.h with planes of a
 * compile-time type and every quantisation of the signal behind a named, switchable operation), in four flavours:
 *
 *   exact64  double planes, quantisations kept, the oracle's poles s*a + (p - p*a)
 *            == ntsc_oracle_field() bit for bit (tests/test_modes_oracle.py): the self-check that ties the model's
 *            structure -- delays, raw tails, zero fill, head-switch remap, field parity, draws -- to the pinned oracle;
 *   fast32   float where the kernels say RT (filters, colour matrices, rotation), quantisations kept, poles
 *            fmaf(a, s - p, p): the bit-exact statement of NTSCSIM_MODE_FAST32;
 *   real64   double planes, NO quantisation of the signal, poles p + a*(s - p), one luma constant in front of the final
 *            truncation: the DEFINITION of NTSCSIM_MODE_FLOAT;
 *   real32   the same in float with fmaf poles: CPU only, measures how far an fp32 evaluation is from real64
 *            (tools/float_model_err.py), which is where the GPU tests' tolerances come from.
 *
 * Compiled with -ffp-contract=off like the oracle: every fused operation is an explicit fma()/fmaf().
 */
#ifndef NTSC_MODES_ORACLE_H
#define NTSC_MODES_ORACLE_H

#include "ntsc_oracle.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Outputs of the real flavours: each NULL or a buffer of the flavour's type (double for real64, float for real32),
 * rows of this field only (row k = frame row field+2k). */
typedef struct ntsc_modes_planes {
    void *composite;                  /* L*W: Y at the oracle's composite_y tap                                   */
    void *final_y, *final_i, *final_q;/* L*W each: the planes in front of YIQ -> RGB (luma WITHOUT the constant)   */
    void *v;                          /* L*W*3: r, g, b of every pixel before truncation and clamp, in output LSB  */
} ntsc_modes_planes;

/* Same contract as ntsc_oracle_field(): 0 or -1, `g` advanced by the draws made, int32 taps. */
int ntsc_modes_exact64(const ntscsim_params *p, ntsc_oracle_rng *g,
                       const uint8_t *src_bgra, int src_linesize, int src_interlaced, int src_tff,
                       uint8_t *dst_bgra, int dst_linesize,
                       int width, int height, unsigned field, uint64_t fieldno,
                       const ntsc_oracle_taps *taps);
int ntsc_modes_fast32(const ntscsim_params *p, ntsc_oracle_rng *g,
                      const uint8_t *src_bgra, int src_linesize, int src_interlaced, int src_tff,
                      uint8_t *dst_bgra, int dst_linesize,
                      int width, int height, unsigned field, uint64_t fieldno,
                      const ntsc_oracle_taps *taps);

/* luma_bias: the constant added to Y (units of the 256-scaled signal) in front of the final truncation.
 * dst receives clamp(trunc(v)) per channel, alpha 0. */
int ntsc_modes_real64(const ntscsim_params *p, ntsc_oracle_rng *g,
                      const uint8_t *src_bgra, int src_linesize, int src_interlaced, int src_tff,
                      uint8_t *dst_bgra, int dst_linesize,
                      int width, int height, unsigned field, uint64_t fieldno,
                      double luma_bias, const ntsc_modes_planes *out);
int ntsc_modes_real32(const ntscsim_params *p, ntsc_oracle_rng *g,
                      const uint8_t *src_bgra, int src_linesize, int src_interlaced, int src_tff,
                      uint8_t *dst_bgra, int dst_linesize,
                      int width, int height, unsigned field, uint64_t fieldno,
                      double luma_bias, const ntsc_modes_planes *out);

#ifdef __cplusplus
}
#endif
#endif

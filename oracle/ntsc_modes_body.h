/*
 * ntsc_modes_body.h -- TEST INFRASTRUCTURE ONLY.  The body of ntsc_modes_oracle.c, included once per plane type.
 *
 * The includer defines   REAL  the plane / filter type (double or float),
 *                        SFX(n) a name suffix,
 *                        RFMA(a, b, c) the fused multiply-add of that type.
 *
 * This is ntsc_oracle_field() (ntsc_oracle.c) stage for stage -- same switches, taps, delays, raw tails, zero fill,
 * head-switch remap and rand() stream -- with planes of type REAL.  Every place where the exact oracle quantises the
 * SIGNAL goes through one of the q_*() operations below; m->keep_int selects what they do:
 *   keep_int = 1   what the oracle does (C truncation, integer `/`, arithmetic `>>`): the planes then hold integers,
 *                  exactly representable in either type (|v| < 2^24), and the model is the oracle;
 *   keep_int = 0   nothing: the operation is its real-valued statement (x, s * 0.25, (a + b) * 0.5, ...).
 * The integer noise recurrences, the head-switch geometry and every draw are the oracle's text, unchanged.
 */

/* ------------------------------------------------------------------ the quantising operations ---- */

/* `(int32_t)` of a floating-point value: stores of RGB -> YIQ and of every filter */
static REAL SFX(q_store)(const modes_cfg *m, REAL v)
{
    return m->keep_int ? (REAL)(int32_t)v : v;
}

/* the separators' 4-tap box: integer `sum / 4` */
static REAL SFX(q_box4)(const modes_cfg *m, REAL sum)
{
    return m->keep_int ? (REAL)((int32_t)sum / 4) : sum * (REAL)0.25;
}

/* chroma_into_luma: `(c * amp) / 50`, the sign applied by the caller (integer division is symmetric) */
static REAL SFX(q_modulate)(const modes_cfg *m, REAL c, int amp)
{
    return m->keep_int ? (REAL)(((int32_t)c * amp) / 50) : c * ((REAL)amp / 50);
}

/* chroma_from_luma: `(c * 50) / amp` */
static REAL SFX(q_demodulate)(const modes_cfg *m, REAL c, int amp)
{
    return m->keep_int ? (REAL)(((int32_t)c * 50) / amp) : c * ((REAL)50 / (REAL)amp);
}

/* chroma_from_luma's fill of the odd samples: `(a + b) >> 1` */
static REAL SFX(q_half)(const modes_cfg *m, REAL a, REAL b)
{
    return m->keep_int ? (REAL)(((int32_t)a + (int32_t)b) >> 1) : (a + b) * (REAL)0.5;
}

/* the vertical chroma blend: `(above + cur + 1) >> 1`; as a real operation the mean (the +1 is a rounding device) */
static REAL SFX(q_blend)(const modes_cfg *m, REAL above, REAL cur)
{
    return m->keep_int ? (REAL)(((int32_t)above + (int32_t)cur + 1) >> 1) : (above + cur) * (REAL)0.5;
}

/* EXTENSION (ghosting): `acc / 256` */
static REAL SFX(q_ghost)(const modes_cfg *m, REAL acc)
{
    return m->keep_int ? (REAL)((int32_t)acc / 256) : acc / 256;
}

static int SFX(clamp255)(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

/* the final `(int)(x / 256)`, clamped: the byte of a channel value in output LSB */
static int SFX(q_out)(REAL v)
{
    if (v >= 256) return 255;
    if (!(v > -1)) return 0;
    return SFX(clamp255)((int)v);
}

/* ------------------------------------------------------------------------- one-pole IIR ---- */

typedef struct { REAL alpha, prev; } SFX(onepole);

static void SFX(onepole_set)(SFX(onepole) *f, double rate, double hz, double reset)
{
    double timeInterval = 1.0 / rate;
    double tau = 1 / (hz * 2 * M_PI);
    f->alpha = (REAL)(timeInterval / (tau + timeInterval));      /* the kernels: (RT)P.a_* of the same double */
    f->prev = (REAL)reset;
}

static REAL SFX(onepole_lp)(const modes_cfg *m, SFX(onepole) *f, REAL sample)
{
    if (m->pole == MODES_POLE_ORACLE) {
        REAL stage1 = sample * f->alpha;
        REAL stage2 = f->prev - (f->prev * f->alpha);
        f->prev = stage1 + stage2;
    } else if (m->pole == MODES_POLE_DIFF) {
        f->prev = f->prev + f->alpha * (sample - f->prev);
    } else {
        f->prev = RFMA(f->alpha, sample - f->prev, f->prev);
    }
    return f->prev;
}

static REAL SFX(onepole_hp)(const modes_cfg *m, SFX(onepole) *f, REAL sample)
{
    return sample - SFX(onepole_lp)(m, f, sample);
}

static void SFX(row_lp3_delayed)(const modes_cfg *m, REAL *P, int W, double cutoff, double reset, int delay)
{
    SFX(onepole) lp[3];
    int x, f;
    for (f = 0; f < 3; f++) SFX(onepole_set)(&lp[f], NTSC_RATE, cutoff, reset);
    for (x = 0; x < W; x++) {
        REAL s = P[x];
        for (f = 0; f < 3; f++) s = SFX(onepole_lp)(m, &lp[f], s);
        if (x >= delay) P[x - delay] = SFX(q_store)(m, s);
    }
}

/* ------------------------------------------------------------- subcarrier mod / demod ------ */

static void SFX(row_chroma_into_luma)(const modes_cfg *m, REAL *Y, REAL *I, REAL *Q, int W, unsigned xi, int amp)
{
    int x;
    for (x = 0; x < W; x++) {
        unsigned s = (xi + (unsigned)x) & 3;
        REAL chroma = SFX(q_modulate)(m, (s & 1u) ? Q[x] : I[x], amp);
        if (s & 2u) chroma = -chroma;
        Y[x] += chroma;
        I[x] = 0;
        Q[x] = 0;
    }
}

static void SFX(row_chroma_from_luma)(const modes_cfg *m, REAL *Y, REAL *I, REAL *Q, REAL *chroma, int W,
                                      unsigned xi, int amp)
{
    REAL d0 = 0, d1 = 0, d2, d3, c;
    int x;

    /* 4-tap box, pre-charged with the first two samples.  The oracle keeps a running sum; here the four samples are
     * summed afresh (the same integer where the planes hold integers, no drift where they do not). */
    d2 = Y[0];
    d3 = Y[1];
    for (x = 0; x < W; x++) {
        c = (x + 2 < W) ? Y[x + 2] : 0;
        d0 = d1; d1 = d2; d2 = d3; d3 = c;
        Y[x] = SFX(q_box4)(m, ((d0 + d1) + d2) + d3);
        chroma[x] = c - Y[x];
    }

    for (x = (int)((4 - xi) & 3); x + 3 < W; x += 4) {
        chroma[x + 2] = -chroma[x + 2];
        chroma[x + 3] = -chroma[x + 3];
    }
    for (x = 0; x < W; x++) chroma[x] = SFX(q_demodulate)(m, chroma[x], amp);

    for (x = 0; x + (int)xi + 1 < W; x += 2) {
        I[x] = -chroma[x + xi + 0];
        Q[x] = -chroma[x + xi + 1];
    }
    for (; x < W; x += 2) { I[x] = 0; Q[x] = 0; }
    for (x = 0; x + 2 < W; x += 2) {
        I[x + 1] = SFX(q_half)(m, I[x], I[x + 2]);
        Q[x + 1] = SFX(q_half)(m, Q[x], Q[x + 2]);
    }
    for (; x < W; x++) { I[x] = 0; Q[x] = 0; }
}

/* ------------------------------------------------------------------------------- taps ------ */

static void SFX(tap)(int32_t *dst, const REAL *src, size_t n)
{
    size_t i;
    if (dst) for (i = 0; i < n; i++) dst[i] = (int32_t)src[i];
}

static void SFX(rtap)(void *dst, const REAL *src, size_t n)
{
    if (dst) memcpy(dst, src, n * sizeof(REAL));
}

/* ------------------------------------------------------------------------- the field ------- */

static int SFX(modes_field)(const modes_cfg *m, const ntscsim_params *p, ntsc_oracle_rng *g,
                            const uint8_t *src, int src_linesize, int src_interlaced, int src_tff,
                            uint8_t *dst, int dst_linesize,
                            int W, int H, unsigned field, uint64_t fieldno,
                            const ntsc_oracle_taps *taps, const ntsc_modes_planes *out)
{
    static const ntsc_oracle_taps no_taps;
    static const ntsc_modes_planes no_out;
    const int output_ntsc = (p->tv_standard == NTSCSIM_TV_NTSC);
    unsigned opposite;
    REAL *fY, *fI, *fQ, *chroma;
    int L, k, x;
    size_t n;

    if (!src || !dst) return -1;
    if (dst_linesize < W * 4 || src_linesize < W * 4) return -1;
    if (W <= 0 || H <= 0 || field > 1) return -1;
    if (!taps) taps = &no_taps;
    if (!out) out = &no_out;

    opposite = src_interlaced ? (src_tff ? 1u : 0u) : 0u;
    L = ((unsigned)H > field) ? (int)((H - (int)field + 1) / 2) : 0;
    n = (size_t)L * (size_t)W;

    fY = (REAL *)calloc(n + 1, sizeof(REAL));
    fI = (REAL *)calloc(n + 1, sizeof(REAL));
    fQ = (REAL *)calloc(n + 1, sizeof(REAL));
    chroma = (REAL *)calloc((size_t)W + 1, sizeof(REAL));
    if (!fY || !fI || !fQ || !chroma) { free(fY); free(fI); free(fQ); free(chroma); return -1; }

#define ROWY(k) (fY + (size_t)(k) * W)
#define ROWI(k) (fI + (size_t)(k) * W)
#define ROWQ(k) (fQ + (size_t)(k) * W)
#define FRAME_Y(k) ((unsigned)(field + 2u * (unsigned)(k)))

    /* RGB -> YIQ */
    for (k = 0; k < L; k++) {
        unsigned y = FRAME_Y(k), sy = y + opposite;
        const uint8_t *srow;
        if (sy > (unsigned)H - 1u) sy = (unsigned)H - 1u;
        srow = src + (size_t)src_linesize * sy;
        for (x = 0; x < W; x++) {
            uint32_t px;
            int r, gg, b;
            REAL dY;
            memcpy(&px, srow + 4 * (size_t)x, 4);
            r = (int)((px >> 16) & 0xFF); gg = (int)((px >> 8) & 0xFF); b = (int)(px & 0xFF);
            dY = ((REAL)0.30 * r) + ((REAL)0.59 * gg) + ((REAL)0.11 * b);
            ROWY(k)[x] = SFX(q_store)(m, 256 * dY);
            ROWI(k)[x] = SFX(q_store)(m, 256 * (((REAL)-0.27 * (b - dY)) + ((REAL)0.74 * (r - dY))));
            ROWQ(k)[x] = SFX(q_store)(m, 256 * (((REAL)0.41 * (b - dY)) + ((REAL)0.48 * (r - dY))));
        }
    }

    /* input chroma low-pass */
    if (p->composite_in_chroma_lowpass) {
        for (k = 0; k < L; k++) SFX(row_lp3_delayed)(m, ROWI(k), W, 1300000, 0, 2);
        for (k = 0; k < L; k++) SFX(row_lp3_delayed)(m, ROWQ(k), W, 600000, 0, 4);
    }

    /* modulate */
    for (k = 0; k < L; k++)
        SFX(row_chroma_into_luma)(m, ROWY(k), ROWI(k), ROWQ(k), W,
                                  scanline_phase(p, FRAME_Y(k), fieldno), p->subcarrier_amplitude);

    /* composite pre-emphasis */
    if (p->composite_preemphasis != 0 && p->composite_preemphasis_cut > 0) {
        for (k = 0; k < L; k++) {
            REAL *Y = ROWY(k);
            SFX(onepole) pre;
            SFX(onepole_set)(&pre, NTSC_RATE, p->composite_preemphasis_cut, 16);
            for (x = 0; x < W; x++) {
                REAL s = Y[x];
                s += SFX(onepole_hp)(m, &pre, s) * (REAL)p->composite_preemphasis;
                Y[x] = SFX(q_store)(m, s);
            }
        }
    }

    /* luma noise; the accumulator carries across rows */
    if (p->video_noise != 0) {
        int noise = 0;
        unsigned noise_mod = (unsigned)((p->video_noise * 2) + 1);
        for (k = 0; k < L; k++) {
            REAL *Y = ROWY(k);
            for (x = 0; x < W; x++) {
                Y[x] += (REAL)noise;
                noise += (int)(ntsc_oracle_rng_next(g) % noise_mod) - p->video_noise;
                noise /= 2;
            }
        }
    }
    SFX(tap)(taps->composite_y, fY, n);
    SFX(rtap)(out->composite, fY, n);

    /* EXTENSION: multipath ghosting */
    if (p->ghost_taps > 0) {
        REAL *raw = (REAL *)malloc(((size_t)W + 1) * sizeof(REAL));
        int gk;
        for (k = 0; k < L && raw; k++) {
            REAL *Y = ROWY(k);
            memcpy(raw, Y, (size_t)W * sizeof(REAL));
            for (x = 0; x < W; x++) {
                REAL acc = 0;
                for (gk = 0; gk < p->ghost_taps; gk++)
                    if (x - p->ghost_delay[gk] >= 0) acc += p->ghost_gain[gk] * raw[x - p->ghost_delay[gk]];
                Y[x] = raw[x] + SFX(q_ghost)(m, acc);
            }
        }
        free(raw);
    }

    /* VHS head switching: the oracle's geometry, samples moved as they are */
    if (p->vhs_head_switching) {
        unsigned twidth = (unsigned)W + ((unsigned)W / 10u);
        unsigned tx, hx, pp, x2, shy = 0;
        double noise = 0, t;
        int shif, ishif, y;
        REAL *tmp = (REAL *)malloc((size_t)twidth * sizeof(REAL));

        if (p->vhs_head_switching_phase_noise != 0) {
            unsigned u = ntsc_oracle_rng_next(g);
            u *= ntsc_oracle_rng_next(g);
            u *= ntsc_oracle_rng_next(g);
            u *= ntsc_oracle_rng_next(g);
            u %= 2000000000U;
            noise = ((double)u / 1000000000U) - 1.0;
            noise *= p->vhs_head_switching_phase_noise;
        }

        t = output_ntsc ? twidth * 262.5 : twidth * 312.5;

        pp = (unsigned)(fmod(p->vhs_head_switching_point + noise, 1.0) * t);
        y = (int)((pp / twidth) * 2u) + (int)field;
        pp = (unsigned)(fmod(p->vhs_head_switching_phase + noise, 1.0) * t);
        hx = pp % twidth;

        y -= output_ntsc ? (262 - 240) * 2 : (312 - 288) * 2;

        tx = hx;
        ishif = (hx >= twidth / 2) ? (int)(hx - twidth) : (int)hx;

        shif = 0;
        while (y < H) {
            if (y >= 0 && shif != 0 && tmp) {
                REAL *Y = ROWY((y - (int)field) / 2);
                unsigned xx;
                x2 = (tx + twidth + (unsigned)shif) % twidth;
                memset(tmp, 0, (size_t)twidth * sizeof(REAL));
                memcpy(tmp, Y, (size_t)W * sizeof(REAL));
                for (xx = tx; xx < (unsigned)W; xx++) {
                    Y[xx] = tmp[x2];
                    if (++x2 == twidth) x2 = 0;
                }
            }
            shif = (shy == 0) ? ishif : (shif * 7) / 8;
            tx = 0;
            y += 2;
            shy++;
        }
        free(tmp);
    }
    SFX(tap)(taps->headswitch_y, fY, n);

    /* demodulate */
    if (!p->nocolor_subcarrier)
        for (k = 0; k < L; k++)
            SFX(row_chroma_from_luma)(m, ROWY(k), ROWI(k), ROWQ(k), chroma, W,
                                      scanline_phase(p, FRAME_Y(k), fieldno), p->subcarrier_amplitude_back);
    SFX(tap)(taps->demod_y, fY, n); SFX(tap)(taps->demod_i, fI, n); SFX(tap)(taps->demod_q, fQ, n);

    /* chroma noise */
    if (p->video_chroma_noise != 0) {
        int noiseU = 0, noiseV = 0;
        unsigned mm = (unsigned)((p->video_chroma_noise * 2) + 1);
        for (k = 0; k < L; k++) {
            REAL *U = ROWI(k), *V = ROWQ(k);
            for (x = 0; x < W; x++) {
                U[x] += (REAL)noiseU;
                V[x] += (REAL)noiseV;
                noiseU += (int)(ntsc_oracle_rng_next(g) % mm) - p->video_chroma_noise;
                noiseU /= 2;
                noiseV += (int)(ntsc_oracle_rng_next(g) % mm) - p->video_chroma_noise;
                noiseV /= 2;
            }
        }
    }
    /* chroma phase noise */
    if (p->video_chroma_phase_noise != 0) {
        int noise = 0;
        unsigned mm = (unsigned)((p->video_chroma_phase_noise * 2) + 1);
        for (k = 0; k < L; k++) {
            REAL *U = ROWI(k), *V = ROWQ(k);
            double pi;
            REAL sinpi, cospi;
            noise += (int)(ntsc_oracle_rng_next(g) % mm) - p->video_chroma_phase_noise;
            noise /= 2;
            pi = ((double)noise * M_PI) / 100;
            sinpi = (REAL)sin(pi);
            cospi = (REAL)cos(pi);
            for (x = 0; x < W; x++) {
                REAL u = U[x], v = V[x];
                REAL u_ = (u * cospi) - (v * sinpi);
                REAL v_ = (u * sinpi) + (v * cospi);
                U[x] = SFX(q_store)(m, u_);
                V[x] = SFX(q_store)(m, v_);
            }
        }
    }
    SFX(tap)(taps->noise_i, fI, n); SFX(tap)(taps->noise_q, fQ, n);

    /* VHS block */
    if (p->emulating_vhs) {
        double luma_cut, chroma_cut;
        int chroma_delay;
        switch (p->output_vhs_tape_speed) {
        case NTSCSIM_VHS_LP: luma_cut = 1900000; chroma_cut = 300000; chroma_delay = 12; break;
        case NTSCSIM_VHS_EP: luma_cut = 1400000; chroma_cut = 280000; chroma_delay = 14; break;
        default:             luma_cut = 2400000; chroma_cut = 320000; chroma_delay = 9;  break;
        }

        /* luma low-pass + emphasis */
        for (k = 0; k < L; k++) {
            REAL *Y = ROWY(k);
            SFX(onepole) lp[3], pre;
            int f;
            for (f = 0; f < 3; f++) SFX(onepole_set)(&lp[f], NTSC_RATE, luma_cut, 16);
            SFX(onepole_set)(&pre, NTSC_RATE, luma_cut, 16);
            for (x = 0; x < W; x++) {
                REAL s = Y[x];
                for (f = 0; f < 3; f++) s = SFX(onepole_lp)(m, &lp[f], s);
                s += SFX(onepole_hp)(m, &pre, s) * (REAL)1.6;
                Y[x] = SFX(q_store)(m, s);
            }
        }

        /* chroma low-pass */
        for (k = 0; k < L; k++) {
            SFX(row_lp3_delayed)(m, ROWI(k), W, chroma_cut, 0, chroma_delay);
            SFX(row_lp3_delayed)(m, ROWQ(k), W, chroma_cut, 0, chroma_delay);
        }

        /* vertical chroma blend through a one-line delay */
        if (p->vhs_chroma_vert_blend && output_ntsc) {
            REAL *delayU = (REAL *)calloc((size_t)W, sizeof(REAL));
            REAL *delayV = (REAL *)calloc((size_t)W, sizeof(REAL));
            if (delayU && delayV) {
                for (k = 1; k < L; k++) {
                    REAL *U = ROWI(k), *V = ROWQ(k);
                    for (x = 0; x < W; x++) {
                        REAL cU = U[x], cV = V[x];
                        U[x] = SFX(q_blend)(m, delayU[x], cU);
                        V[x] = SFX(q_blend)(m, delayV[x], cV);
                        delayU[x] = cU;
                        delayV[x] = cV;
                    }
                }
            }
            free(delayU); free(delayV);
        }

        /* playback sharpening */
        for (k = 0; k < L; k++) {
            REAL *Y = ROWY(k);
            SFX(onepole) lp[3];
            int f;
            for (f = 0; f < 3; f++) SFX(onepole_set)(&lp[f], NTSC_RATE, luma_cut * 4, 0);
            for (x = 0; x < W; x++) {
                REAL s, ts;
                s = ts = Y[x];
                for (f = 0; f < 3; f++) ts = SFX(onepole_lp)(m, &lp[f], ts);
                Y[x] = SFX(q_store)(m, s + ((s - ts) * (REAL)p->vhs_out_sharpen * 2));
            }
        }

        /* composite out of the VCR */
        if (!p->vhs_svideo_out) {
            for (k = 0; k < L; k++) {
                unsigned xi = scanline_phase(p, FRAME_Y(k), fieldno);
                SFX(row_chroma_into_luma)(m, ROWY(k), ROWI(k), ROWQ(k), W, xi, p->subcarrier_amplitude);
                SFX(row_chroma_from_luma)(m, ROWY(k), ROWI(k), ROWQ(k), chroma, W, xi, p->subcarrier_amplitude);
            }
        }
    }
    SFX(tap)(taps->vhs_y, fY, n); SFX(tap)(taps->vhs_i, fI, n); SFX(tap)(taps->vhs_q, fQ, n);

    /* chroma dropout */
    if (p->video_chroma_loss != 0) {
        for (k = 0; k < L; k++) {
            if ((ntsc_oracle_rng_next(g) % 100000U) < (unsigned)p->video_chroma_loss) {
                for (x = 0; x < W; x++) { ROWI(k)[x] = 0; ROWQ(k)[x] = 0; }
            }
        }
    }

    /* output chroma low-pass */
    if (p->composite_out_chroma_lowpass) {
        if (p->composite_out_chroma_lowpass_lite) {
            for (k = 0; k < L; k++) SFX(row_lp3_delayed)(m, ROWI(k), W, 2600000, 0, 1);
            for (k = 0; k < L; k++) SFX(row_lp3_delayed)(m, ROWQ(k), W, 2600000, 0, 1);
        } else {
            for (k = 0; k < L; k++) SFX(row_lp3_delayed)(m, ROWI(k), W, 1300000, 0, 2);
            for (k = 0; k < L; k++) SFX(row_lp3_delayed)(m, ROWQ(k), W, 600000, 0, 4);
        }
    }
    SFX(tap)(taps->final_y, fY, n); SFX(tap)(taps->final_i, fI, n); SFX(tap)(taps->final_q, fQ, n);
    SFX(rtap)(out->final_y, fY, n); SFX(rtap)(out->final_i, fI, n); SFX(rtap)(out->final_q, fQ, n);

    /* YIQ -> RGB into the rows of this field only; the luma constant of the real flavours sits in front of the
     * truncation (m->luma_bias, in units of the 256-scaled signal; 0 where the planes hold integers) */
    for (k = 0; k < L; k++) {
        uint8_t *drow = dst + (size_t)dst_linesize * FRAME_Y(k);
        for (x = 0; x < W; x++) {
            const REAL Yv = ROWY(k)[x] + (REAL)m->luma_bias, Iv = ROWI(k)[x], Qv = ROWQ(k)[x];
            const REAL r = ((((REAL)1.000 * Yv) + ((REAL)0.956 * Iv)) + ((REAL)0.621 * Qv)) / 256;
            const REAL gg = ((((REAL)1.000 * Yv) + ((REAL)-0.272 * Iv)) + ((REAL)-0.647 * Qv)) / 256;
            const REAL b = ((((REAL)1.000 * Yv) + ((REAL)-1.106 * Iv)) + ((REAL)1.703 * Qv)) / 256;
            uint32_t px = ((uint32_t)SFX(q_out)(r) << 16) + ((uint32_t)SFX(q_out)(gg) << 8) + (uint32_t)SFX(q_out)(b);
            memcpy(drow + 4 * (size_t)x, &px, 4);
            if (out->v) {
                REAL *v = (REAL *)out->v + 3 * ((size_t)k * W + x);
                v[0] = r; v[1] = gg; v[2] = b;
            }
        }
    }

#undef ROWY
#undef ROWI
#undef ROWQ
#undef FRAME_Y
    free(fY); free(fI); free(fQ); free(chroma);
    return 0;
}

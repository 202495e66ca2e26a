// lane_rand.hpp -- device pieces of glibc's rand() that more than one translation unit uses: the per-lane generator
// with its window in LDS, and the jump-ahead product.  Included inside namespace ntscsim by ntsc_kernels.hip (the
// simulator) and ntsc_key.hip (the colorkey stage's draw kernel).
#pragma once
#include <stdint.h>

#ifndef DEV
#define DEV __device__ __forceinline__
#endif

// ------------------------------------------------------------------------------ rand() in LDS
// Per-lane glibc TYPE_3 generator: the 31-word window lives in LDS as ring[slot][lane]
// (conflict-free: bank = lane), the three newest words in registers.
struct LaneRand {
    uint32_t p3, p2, p1;   // s[i-3], s[i-2], s[i-1]
    int slot;              // wave-uniform
    DEV void init(uint32_t *ring, const uint32_t *state, int stride, int lane)
    {
        for (int j = 0; j < 31; j++) ring[j * 64 + lane] = state[(size_t)j * stride];
        p3 = ring[28 * 64 + lane];
        p2 = ring[29 * 64 + lane];
        p1 = ring[30 * 64 + lane];
        slot = 0;
    }
    DEV uint32_t next(uint32_t *ring, int lane)
    {
#ifdef NTSC_AB_NORAND      // timing-only A/B build (WRONG pixels): no LDS ring
        (void)ring; (void)lane;
        p3 = p3 * 1664525u + 1013904223u;
        return p3 >> 1;
#endif
        const uint32_t v = ring[slot * 64 + lane] + p3;   // s[i-31] + s[i-3]
        ring[slot * 64 + lane] = v;
        p3 = p2; p2 = p1; p1 = v;
        slot = (slot == 30) ? 0 : slot + 1;
        return v >> 1;
    }
};

// Jump-ahead: state advanced by the polynomial c (x^n mod x^31 - x^28 - 1) given the 61-word
// extension w of the starting window:  out[j] = sum_k c[k] * w[j+k].  Fully unrolled so that
// everything stays in registers (private arrays with dynamic indices would live in scratch).
// Each product and its add are ONE v_mad_u64_u32 whose low word is kept (the sums are taken modulo 2^32): 961
// instructions where v_mul_lo_u32 and the adds the compiler pairs into v_add3_u32 were 1,423, and k_row_states, which is
// little else, 34.4 us where that form took 38.3 (profiles/r09_rowstates_ab.txt; -DNTSC_JUMP61_MUL_ADD: that form, A/B).
DEV void jump61(const uint32_t *__restrict__ c, const uint32_t *__restrict__ w, uint32_t (&o)[31])
{
    uint32_t cc[31], ww[61];
#pragma unroll
    for (int k = 0; k < 31; k++) cc[k] = c[k];
#pragma unroll
    for (int i = 0; i < 61; i++) ww[i] = w[i];
#pragma unroll
    for (int j = 0; j < 31; j++) {
#ifndef NTSC_JUMP61_MUL_ADD
        unsigned long long acc = 0, carry;
#pragma unroll
        for (int k = 0; k < 31; k++)
            asm("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(acc), "=s"(carry) : "v"(cc[k]), "v"(ww[j + k]));
        o[j] = (uint32_t)acc;
#else
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < 31; k++) acc += cc[k] * ww[j + k];
        o[j] = acc;
#endif
    }
}

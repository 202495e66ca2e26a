// ntsc_pack.hpp -- the last step of YIQ_to_RGB (ffmpeg_ntsc.cpp:1385-1396): three channel values, each 256 x the channel
// and already through the saturating unsigned conversion (v_cvt_u32_f64 / _f32: negative -> 0, too large -> 2^32 - 1),
// become one BGRA pixel.  Plain integer code, so the same text runs on the host: tests/pack_check.cpp and
// tests/pack_sat_check.cpp sweep it with g++ (there v_perm_b32 and v_cvt_pk_u16_u32 are the models below).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define NTSC_PACK_FN __host__ __device__ __forceinline__
#else
#define NTSC_PACK_FN static inline
#endif

namespace ntscsim {

// v_perm_b32: byte i of the result is byte sel[i] of the eight bytes {hi: 7..4, lo: 3..0}; selector 0x0c is constant 0
// (the only selectors >= 8 the callers use)
NTSC_PACK_FN uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t d = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t s = (sel >> (8 * i)) & 0xFFu;
        const uint32_t byte = s < 8 ? (uint32_t)(src >> (8 * s)) & 0xFFu : 0u;
        d |= byte << (8 * i);
    }
    return d;
#endif
}

// the round-4 form: shift, clamp, shift / or -- 3 + 3 + 2 VALU (v_lshrrev, v_min_u32, v_lshl_or / v_or3)
NTSC_PACK_FN uint32_t pack_bgra_shift(uint32_t r, uint32_t g, uint32_t b)
{
    r = r >> 8; g = g >> 8; b = b >> 8;
    r = r < 255u ? r : 255u; g = g < 255u ? g : 255u; b = b < 255u ? b : 255u;
    return ((r << 16) | b) | (g << 8);
}

// Clamp first, then pick: for every 32-bit x, min(x, 0xFFFF) >> 8 == min(x >> 8, 255) (x <= 0xFFFF: both are x >> 8;
// otherwise both are 255), and after the clamp the channel is byte 1 of its word -- so two v_perm_b32 gather the
// three bytes: 3 + 2 VALU, three issue slots fewer per pixel.  Alpha stays 0 (selector 0x0c).
NTSC_PACK_FN uint32_t pack_bgra_perm(uint32_t r, uint32_t g, uint32_t b)
{
    r = r < 0xFFFFu ? r : 0xFFFFu; g = g < 0xFFFFu ? g : 0xFFFFu; b = b < 0xFFFFu ? b : 0xFFFFu;
    const uint32_t gb = perm_b32(g, b, 0x0c0c0501u);          // byte 0 = b[1], byte 1 = g[1]
    return perm_b32(r, gb, 0x0c050100u);                      // byte 2 = r[1]
}

// v_cvt_pk_u16_u32: each 32-bit unsigned source saturates to 16 bits, a in the low half, b in the high half
NTSC_PACK_FN uint32_t cvt_pk_u16(uint32_t a, uint32_t b)
{
#ifdef __HIP_DEVICE_COMPILE__
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    union { u16x2 v; uint32_t u; } c;
    c.v = __builtin_amdgcn_cvt_pk_u16(a, b);
    return c.u;
#else
    a = a < 0xFFFFu ? a : 0xFFFFu; b = b < 0xFFFFu ? b : 0xFFFFu;
    return a | (b << 16);
#endif
}

// The round-10 form: the saturating pack is the clamp of two channels at once, so R and G go through one
// v_cvt_pk_u16_u32 (bytes r[0] r[1] g[0] g[1]), B through one v_min_u32, and a single v_perm_b32 gathers
// b[1], g[1] (byte 3 of the pair), r[1] (byte 1 of the pair): 3 VALU per pixel.  Alpha stays 0.
NTSC_PACK_FN uint32_t pack_bgra_sat(uint32_t r, uint32_t g, uint32_t b)
{
    const uint32_t rg = cvt_pk_u16(r, g);
    b = b < 0xFFFFu ? b : 0xFFFFu;
    return perm_b32(rg, b, 0x0c050701u);
}

NTSC_PACK_FN uint32_t pack_bgra(uint32_t r, uint32_t g, uint32_t b)
{
#if defined(NTSC_PACK_SHIFT)    /* A/B: the round-4 pack */
    return pack_bgra_shift(r, g, b);
#elif defined(NTSC_PACK_PERM)   /* A/B: the round-7 pack */
    return pack_bgra_perm(r, g, b);
#else
    return pack_bgra_sat(r, g, b);
#endif
}

} // namespace ntscsim

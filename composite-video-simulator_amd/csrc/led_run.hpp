// led_run.hpp -- what the vhsled stage (include/ntscsim.h: ntscsim_led_*) decides on plain integers: where the ninth
// non-blackish pixel of a run lies in a 64-pixel chunk of a row, and the nine-row mean and rounding that turn the
// rows' edges into shifts.  No HIP in this file: the kernel (csrc/ntsc_led.hip) runs it on wave-uniform values, and
// tests/led_run_check.cpp sweeps it with plain g++ against a bit-by-bit loop.  Line numbers refer to
// ffmpeg_vhsled.cpp of the reference.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LED_HOST_DEVICE __host__ __device__ inline
#else
#define LED_HOST_DEVICE inline
#endif

namespace ntscsim {

constexpr int LED_RUN = 9;               // the ninth non-blackish pixel in a row ends the scan :878
constexpr int LED_CHUNK = 64;            // pixels per mask: one per lane of a wavefront

// blackish() :682-692 negated: p is a pixel, blue the low byte of the row's first pixel -- the tool never shifts r,
// so B, G and R of the pixel are all compared with that one byte.  A darker channel (negative difference) is blackish.
LED_HOST_DEVICE bool led_not_blackish(uint32_t p, uint32_t blue)
{
    const int r = (int)(blue & 0xFFu);
    return (int)(p & 0xFFu) - r >= 16 || (int)((p >> 8) & 0xFFu) - r >= 16 || (int)((p >> 16) & 0xFFu) - r >= 16;
}

// trailing / leading zeros of a 64-bit word that is not 0
LED_HOST_DEVICE int led_ctz64(uint64_t v) { return __builtin_ctzll(v); }
LED_HOST_DEVICE int led_clz64(uint64_t v) { return __builtin_clzll(v); }

struct LedRunStep {
    int hit;                             // bit of the chunk that holds the NINTH pixel of the first run of nine, or -1
    int carry;                           // hit < 0: length (0 .. 8) of the run of ones that ends the chunk
};

// One chunk of the row walk :876-895.  Bit i of `mask` says pixel base + i is not blackish (bits behind the row's end
// are 0); `carry` (0 .. 8) is the run of non-blackish pixels that ended the chunk before.  A run that began in the
// earlier chunk is found here: hit is then 8 - carry, and the run's first pixel, base + hit - 8, lies below base.
LED_HOST_DEVICE LedRunStep led_run_step(uint64_t mask, int carry)
{
    // the run that comes in: it needs the 9 - carry lowest pixels of this chunk
    if (carry > 0) {
        const uint64_t need = (1ull << (LED_RUN - carry)) - 1ull;
        if ((mask & need) == need) return LedRunStep{LED_RUN - 1 - carry, 0};
    }
    // runs inside the chunk: bit s of t says bits s .. s + 8 are all set
    uint64_t t = mask & (mask >> 1);     // 2
    t &= t >> 2;                         // 4
    t &= t >> 4;                         // 8
    t &= mask >> 8;                      // 9
    if (t) return LedRunStep{led_ctz64(t) + LED_RUN - 1, 0};
    // no run of nine, so the ones at the top are 8 at the most (and ~mask is not 0)
    return LedRunStep{-1, led_clz64(~mask)};
}

// adj2[y] :903-906 for 4 <= y < h - 4: a[0 .. 8] are adj[y - 4 .. y + 4], each e << 16 with e <= 3640, so the sum
// plus 5 fits an int32 (9 * 3640 * 65536 + 5 = 2146959365).  The division truncates; the sum is never negative.
LED_HOST_DEVICE int32_t led_smooth(const int32_t a[9])
{
    int32_t s = 5;
    for (int i = 0; i < 9; i++) s += a[i];
    return s / 9;
}

// x :913 and the clamp :920
LED_HOST_DEVICE int32_t led_shift_of(int32_t adj2)
{
    const int32_t x = (adj2 + 0x8000) >> 16;
    return x < 0 ? 0 : x;
}

// :921 -- a row moves only when its shift is below half the width (unsigned division in the tool, w > 0)
LED_HOST_DEVICE bool led_row_moves(int32_t x, int32_t w) { return x < w / 2; }

constexpr int LED_MAX_WIDTH = 3640;      // 9 * w * 65536 + 5 <= INT32_MAX
constexpr int LED_MIN_SIZE = 16;         // :717
constexpr int LED_MAX_HEIGHT = 65536;

} // namespace ntscsim

// Host check of csrc/ntsc_pack.hpp (built and run by tests/test_pack_host.py with plain g++): the clamp-then-pick pixel
// pack against the reference's per-channel clamp((int)(v / 256), 0, 255), for every channel value up to 0x1FFFF and the
// two ends of the conversion's saturated range, in each of the three channel positions.
//
// x is the channel after the saturating unsigned conversion; the reference converts the same real v to int, which
// saturates at INT_MAX where the unsigned conversion gives x >= 2^31.  So the reference value of x is
// clamp(X >> 8, 0, 255) with X = x taken as a 64-bit integer: for x < 2^31 that is clamp((int)x >> 8, 0, 255) literally,
// for x >= 2^31 it is 255 (the clamp of INT_MAX >> 8).
#include <cstdint>
#include <cstdio>

#include "ntsc_pack.hpp"

static uint32_t ref_channel(uint32_t x)
{
    const int64_t v = (int64_t)x >> 8;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

static int bad = 0;

static void check(uint32_t r, uint32_t g, uint32_t b)
{
    const uint32_t want = (ref_channel(r) << 16) | (ref_channel(g) << 8) | ref_channel(b);      // B G R A bytes, A = 0
    const uint32_t got = ntscsim::pack_bgra_perm(r, g, b), old = ntscsim::pack_bgra_shift(r, g, b);
    if (got != want || old != want) {
        if (bad++ < 10) std::printf("r=%08x g=%08x b=%08x: perm %08x shift %08x want %08x\n", r, g, b, got, old, want);
    }
}

int main()
{
    // the other two channels hold values whose every byte differs from the one under test's, so a selector that
    // picks the wrong word or the wrong byte shows
    const uint32_t others[][2] = {{0x00001234u, 0x0000ABCDu}, {0xFFFFFFFFu, 0u}, {0x00010000u, 0x0000FF00u}};
    uint32_t n = 0;
    for (uint64_t i = 0; i <= 0x1FFFFu + 2u; i++) {
        const uint32_t x = i <= 0x1FFFFu ? (uint32_t)i : (i == 0x20000u ? 0x80000000u : 0xFFFFFFFFu);
        for (const auto &o : others) {
            check(x, o[0], o[1]);
            check(o[0], x, o[1]);
            check(o[0], o[1], x);
            n += 3;
        }
        check(x, x, x);
        n++;
    }
    // the selector model itself, on the two selectors the product's other user relies on (csrc/ntsc_encode_fast.hip)
    if (ntscsim::perm_b32(0u, 0xAABBCCDDu, 0x0c0c020cu) != 0x0000BB00u) { std::printf("perm model: R pick\n"); bad++; }
    if (ntscsim::perm_b32(0u, 0xAABBCCDDu, 0x0c0c000cu) != 0x0000DD00u) { std::printf("perm model: B pick\n"); bad++; }
    std::printf("%u packs checked, %d bad\n", n, bad);
    return bad ? 1 : 0;
}

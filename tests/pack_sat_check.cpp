// Host check of the saturating pixel pack of csrc/ntsc_pack.hpp (built and run by tests/test_pack_sat_host.py with plain
// g++, once as it is and once under -fsanitize=address,undefined): pack_bgra_sat -- R and G through the model of
// v_cvt_pk_u16_u32 (min(x, 0xFFFF) per half), B through one clamp, one byte gather -- against pack_bgra_shift, the
// per-channel shift / clamp / or of round 4, which tests/pack_check.cpp holds to the reference's clamp.  The sweep: every
// channel value 0 ... 0x1FFFF, every power of two with its two neighbours up to 2^32 - 1, each in all three channel
// positions beside values whose every byte differs from the one under test's.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ntsc_pack.hpp"

static int bad = 0;

static void check(uint32_t r, uint32_t g, uint32_t b)
{
    const uint32_t want = ntscsim::pack_bgra_shift(r, g, b), got = ntscsim::pack_bgra_sat(r, g, b);
    if (got != want || ntscsim::pack_bgra(r, g, b) != want) {
        if (bad++ < 10) std::printf("r=%08x g=%08x b=%08x: sat %08x shift %08x\n", r, g, b, got, want);
    }
}

int main()
{
    std::vector<uint32_t> xs;
    for (uint32_t x = 0; x <= 0x1FFFFu; x++) xs.push_back(x);
    for (int k = 0; k < 32; k++) {
        const uint32_t p = 1u << k;
        xs.push_back(p - 1u); xs.push_back(p); xs.push_back(p + 1u);
    }
    xs.push_back(0xFFFFFFFEu); xs.push_back(0xFFFFFFFFu);
    const uint32_t others[][2] = {{0x00001234u, 0x0000ABCDu}, {0xFFFFFFFFu, 0u}, {0x00010000u, 0x0000FF00u}};
    unsigned long n = 0;
    for (const uint32_t x : xs) {
        for (const auto &o : others) {
            check(x, o[0], o[1]);
            check(o[0], x, o[1]);
            check(o[0], o[1], x);
            n += 3;
        }
        check(x, x, x);
        n++;
    }
    // the pack model itself: low half = first source, high half = second, each saturated
    if (ntscsim::cvt_pk_u16(0x00012345u, 0x0000BEEFu) != 0xBEEFFFFFu) { std::printf("cvt_pk_u16 model\n"); bad++; }
    if (ntscsim::cvt_pk_u16(0x00000102u, 0xFFFFFFFFu) != 0xFFFF0102u) { std::printf("cvt_pk_u16 model\n"); bad++; }
    std::printf("%lu packs checked, %d bad\n", n, bad);
    return bad ? 1 : 0;
}

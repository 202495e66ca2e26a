// led_run_check -- csrc/led_run.hpp against a bit-by-bit loop in the shape of the tool's row walk
// (ffmpeg_vhsled.cpp:876-895) and against 64-bit arithmetic for the smoothing step.  Stand-alone: plain g++, no HIP.
#include <cstdint>
#include <cstdio>
#include <random>

#include "led_run.hpp"

using namespace ntscsim;

static long checks = 0, bad = 0;

// the tool's walk over one chunk: bc is the run so far
static LedRunStep walk(uint64_t mask, int carry)
{
    int bc = carry;
    for (int i = 0; i < 64; i++) {
        if ((mask >> i) & 1) {
            if (bc >= 8) return LedRunStep{i, 0};
            bc++;
        } else
            bc = 0;
    }
    return LedRunStep{-1, bc};
}

static void check(uint64_t mask, int carry)
{
    const LedRunStep a = led_run_step(mask, carry), b = walk(mask, carry);
    checks++;
    if (a.hit != b.hit || (b.hit < 0 && a.carry != b.carry)) {
        if (bad++ < 10) std::printf("mask %016llx carry %d: hit %d carry %d, want %d %d\n", (unsigned long long)mask, carry, a.hit, a.carry, b.hit, b.carry);
    }
}

// a row of two chunks walked as the kernel walks it: e, or 128 when there is no run
static int row_edge(uint64_t m0, uint64_t m1)
{
    LedRunStep s = led_run_step(m0, 0);
    if (s.hit >= 0) return s.hit - 8;
    s = led_run_step(m1, s.carry);
    return s.hit >= 0 ? 64 + s.hit - 8 : 128;
}

int main()
{
    // every 16-bit pattern at bit offsets 0, 47 and 48 (the last one touches the chunk's end), every carry
    const int offs[3] = {0, 47, 48};
    for (int o = 0; o < 3; o++)
        for (uint32_t pat = 0; pat < 65536; pat++)
            for (int carry = 0; carry <= 8; carry++) check((uint64_t)pat << offs[o], carry);
    std::mt19937_64 rng(20261019);
    for (int i = 0; i < 100000; i++) {
        uint64_t m = rng();
        if (i & 1) m |= rng();                                                   // denser masks: longer runs
        if ((i & 3) == 3) m |= rng();
        check(m, (int)(rng() % 9));
    }
    check(0, 0); check(~0ull, 0); check(~0ull, 8); check(0xFFull, 1); check(0x1FFull << 55, 0); check(0xFFull << 56, 0);
    // two-chunk rows: a run of nine that starts at each of bits 55 .. 63 of the first chunk, alone and behind a run of
    // eight that a blackish pixel ends
    for (int start = 55; start <= 63; start++) {
        unsigned __int128 row = (unsigned __int128)0x1FF << start;
        for (int pre = 0; pre < 2; pre++) {
            if (pre) row |= (unsigned __int128)0xFF << (start - 9);
            const uint64_t m0 = (uint64_t)row, m1 = (uint64_t)(row >> 64);
            checks++;
            if (row_edge(m0, m1) != start) { if (bad++ < 10) std::printf("two chunks, start %d pre %d: %d\n", start, pre, row_edge(m0, m1)); }
        }
        // eight only: not found
        const unsigned __int128 row8 = (unsigned __int128)0xFF << start;
        checks++;
        if (row_edge((uint64_t)row8, (uint64_t)(row8 >> 64)) != 128) { if (bad++ < 10) std::printf("two chunks, eight at %d found\n", start); }
    }
    // smoothing: sums of every residue modulo 9, at small edges and at the widest frame
    for (int w : {16, 17, 720, 3639, LED_MAX_WIDTH})
        for (int k = 0; k < 9 * 9; k++) {
            int32_t a[9];
            for (int i = 0; i < 9; i++) a[i] = (int32_t)(w - (i < k % 9 ? 1 : 0) - (k / 9 > i ? 1 : 0)) << 16;
            int64_t s = 5;
            for (int i = 0; i < 9; i++) s += a[i];
            checks++;
            if (s > INT32_MAX || led_smooth(a) != (int32_t)(s / 9)) { if (bad++ < 10) std::printf("smooth w %d k %d\n", w, k); }
            const int32_t x = led_shift_of(led_smooth(a));
            checks++;
            if (x != (int32_t)(((s / 9) + 0x8000) >> 16) || x < w - 2 || x > w) { if (bad++ < 10) std::printf("shift w %d k %d: %d\n", w, k, x); }
        }
    {   // the residues themselves: nine edges 0 .. 8 apart give sums (e << 16) whose remainders modulo 9 differ
        bool seen[9] = {};
        for (int e = 0; e < 9; e++) {
            int32_t a[9] = {};
            a[0] = e << 16;
            seen[((int64_t)a[0] + 5) % 9] = true;
            checks++;
            if (led_smooth(a) != (int32_t)(((int64_t)a[0] + 5) / 9)) bad++;
        }
        for (int i = 0; i < 9; i++) { checks++; if (!seen[i]) { bad++; std::printf("residue %d not reached\n", i); } }
    }
    checks += 4;
    if (led_row_moves(8, 16) || !led_row_moves(7, 16) || led_row_moves(8, 17) || !led_row_moves(7, 17)) { bad++; std::printf("row_moves\n"); }
    if (!led_not_blackish(0x00000010u, 0) || led_not_blackish(0xFF00000Fu, 0) || !led_not_blackish(0x00100000u, 0xFFFFFF00u) ||
        led_not_blackish(0x00FFFFFFu, 0xFFu)) { bad++; std::printf("not_blackish\n"); }
    std::printf("%ld checks, %ld bad\n", checks, bad);
    return bad ? 1 : 0;
}

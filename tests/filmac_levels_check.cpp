// filmac_levels_check -- csrc/filmac_levels.hpp against a plain transcription of the tool's loops (filmac.cpp:886-951,
// :986 / :1000): the block grid of every width from 16 to 1100, the frame levels of random frames through block
// records, the recurrence, and the byte table of 10^4 random (final_minv, final_maxv) pairs.  Stand-alone: plain g++,
// no HIP.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "filmac_levels.hpp"

using namespace ntscsim;

static long checks = 0, bad = 0;
#define EXPECT(cond, ...)                                        \
    do {                                                         \
        checks++;                                                \
        if (!(cond)) {                                           \
            if (bad++ < 10) { std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                        \
    } while (0)

static uint16_t dec_tab[256];
static uint8_t enc_tab[8193];

// the tool's loops over one frame of L values (three per pixel) :887-925
static FilmacLevels tool_levels(const std::vector<long> &L, unsigned W, unsigned H, long scaleto)
{
    long minv = (scaleto * 6l) / 10l, maxv = (scaleto * 4l) / 10l;
    const unsigned minx = (W * 15) / 100, maxx = (W * 90) / 100, blw = 128, blh = 128;
    for (unsigned y = 0; y < H; y += blh)
        for (unsigned x = minx; x < maxx; x += blw) {
            long long grmin = 0, grmax = 0, grd = 0;
            for (unsigned sy = 0; sy < blh; sy++)
                for (unsigned sx = 0; sx < blw; sx++) {
                    if ((x + sx) >= W || (y + sy) >= H) continue;
                    const long *p = &L[((size_t)(y + sy) * W + (x + sx)) * 3];
                    grd++;
                    grmin += std::min(std::min(p[0], p[1]), p[2]);
                    grmax = std::max(std::max(p[0], p[1]), p[2]);
                    if (maxv < grmax) maxv = grmax;
                }
            grmin += grd / 2l;
            grmin /= grd;
            if (minv > grmin) minv = grmin;
        }
    if (minv == maxv) maxv++;
    return FilmacLevels{minv, maxv};
}

// the tool's stretch and pack of one value :949-951, :986 / :1000; den: final_maxv - final_minv, not 0
static int tool_byte(long Lv, long final_minv, long long den, long scaleto, bool gamma)
{
    long long v = (((long long)(Lv - final_minv)) * (long long)scaleto) / den;
    if (v < -0x7FFFFFFFl) v = -0x7FFFFFFFl;
    if (v > 0x7FFFFFFFl) v = 0x7FFFFFFFl;
    const long t = std::max(0l, (long)v >> 16l);
    int o = gamma ? (int)enc_tab[t > 8192 ? 8192 : t] : (int)std::min(t, 100000l);
    return o > 255 ? 255 : o < 0 ? 0 : o;
}

int main()
{
    for (unsigned i = 0; i < 256; i++) dec_tab[i] = (uint16_t)(unsigned long)(std::pow(i / 255.0, 2.2) * 8192);
    for (unsigned i = 0; i <= 8192; i++) enc_tab[i] = (uint8_t)(unsigned long)(std::pow(i / 8192.0, 1.0 / 2.2) * 255);
    for (unsigned i = 1; i < 256; i++) EXPECT(dec_tab[i] >= dec_tab[i - 1], "decode table decreases at %u", i);
    std::mt19937_64 rng(20261019);

    // ---- the block grid: every width, heights below, at and above a multiple of 128
    for (int W = 16; W <= 1100; W++)
        for (int H : {16, 128, 129, 300}) {
            const FilmacGrid g = filmac_grid(W, H);
            int b = 0;
            const unsigned minx = ((unsigned)W * 15) / 100, maxx = ((unsigned)W * 90) / 100;
            for (unsigned y = 0; y < (unsigned)H; y += 128)
                for (unsigned x = minx; x < maxx; x += 128, b++) {
                    const FilmacBox o = b < g.nbx * g.nby ? filmac_box(g, W, H, b) : FilmacBox{-1, -1, -1, -1};
                    const int w = std::min(128u, (unsigned)W - x), h = std::min(128u, (unsigned)H - y);
                    EXPECT(o.x == (int)x && o.y == (int)y && o.w == w && o.h == h && o.w > 0 && o.h > 0, "grid %dx%d block %d: %d %d %d %d", W, H, b, o.x, o.y, o.w, o.h);
                }
            EXPECT(b == g.nbx * g.nby && b > 0, "grid %dx%d: %d blocks, %d x %d", W, H, b, g.nbx, g.nby);
        }
    for (int W : {16384}) {
        const FilmacGrid g = filmac_grid(W, W);
        EXPECT(g.nbx == 96 && g.nby == 128, "grid of the largest frame: %d x %d", g.nbx, g.nby);
    }

    // ---- frame levels through block records, with and without gamma; few distinct values so that minv == maxv,
    // untouched start values and rounding at every remainder occur
    for (int gamma = 0; gamma < 2; gamma++) {
        const uint16_t *dec = gamma ? dec_tab : nullptr;
        const long scaleto = (long)filmac_scale(gamma != 0);
        EXPECT(scaleto == (gamma ? 0x10000l * 8192l : 0x10000l * 256l), "scale");
        for (int W = 16; W <= 1100; W += 7)
            for (int H : {16, 130}) {
                const int lo = (int)(rng() % 256), span = (int)(rng() % 4 == 0 ? 1 : 1 + rng() % (256 - lo));
                std::vector<uint8_t> px((size_t)W * H * 3);
                for (auto &v : px) v = (uint8_t)(lo + rng() % span);
                if (rng() % 2) px[(size_t)(rng() % ((size_t)W * H)) * 3 + rng() % 3] = (uint8_t)(rng() % 256);   // one outlier, anywhere
                std::vector<long> L(px.size());
                for (size_t i = 0; i < px.size(); i++) L[i] = (long)(gamma ? dec_tab[px[i]] : px[i]) << 16;
                const FilmacLevels want = tool_levels(L, (unsigned)W, (unsigned)H, scaleto);
                const FilmacGrid g = filmac_grid(W, H);
                std::vector<FilmacBlockRec> recs((size_t)(g.nbx * g.nby));
                for (int b = 0; b < g.nbx * g.nby; b++) {
                    const FilmacBox o = filmac_box(g, W, H, b);
                    FilmacBlockRec r{0, 0, 0, 0};
                    for (int y = o.y; y < o.y + o.h; y++)
                        for (int x = o.x; x < o.x + o.w; x++) {
                            const uint8_t *p = &px[((size_t)y * W + x) * 3];
                            const uint8_t mn = std::min(std::min(p[0], p[1]), p[2]), mx = std::max(std::max(p[0], p[1]), p[2]);
                            r.sum += gamma ? dec_tab[mn] : mn;
                            r.count++;
                            r.top = std::max<uint32_t>(r.top, mx);
                        }
                    recs[(size_t)b] = r;
                }
                const FilmacLevels got = filmac_levels(recs.data(), (int)recs.size(), scaleto, dec);
                EXPECT(got.minv == want.minv && got.maxv == want.maxv, "levels %dx%d gamma %d: %lld %lld, want %lld %lld", W, H, gamma,
                       (long long)got.minv, (long long)got.maxv, (long long)want.minv, (long long)want.maxv);
                // the same joined from two halves, as lanes of a wavefront join theirs
                FilmacLevels a = filmac_levels_start(scaleto), c = a;
                for (size_t b = 0; b < recs.size(); b++) (b & 1 ? a : c) = filmac_levels_add(b & 1 ? a : c, recs[b], dec);
                const FilmacLevels j = filmac_levels_end(filmac_levels_join(a, c));
                EXPECT(j.minv == want.minv && j.maxv == want.maxv, "joined levels %dx%d gamma %d", W, H, gamma);
            }
        // the largest block sum stays inside 32 bits
        EXPECT(filmac_block_mean(128u * 128u * (gamma ? 8192u : 255u), 128u * 128u) == (int64_t)(gamma ? 8192 : 255) << 16, "full block mean");
    }
    for (uint32_t count : {1u, 2u, 3u, 127u, 128u, 16384u})                      // rounding: every remainder class near a half
        for (uint32_t sum = 0; sum < 40; sum++) {
            long long grmin = (long long)sum << 16;
            grmin += count / 2l;
            grmin /= count;
            EXPECT(filmac_block_mean(sum, count) == grmin, "mean %u / %u", sum, count);
        }

    // ---- the recurrence :927-942 on random levels; the range stays open
    for (int run = 0; run < 2000; run++) {
        const long S = (long)filmac_scale(run & 1);
        long final_minv = -1, final_maxv = -1;
        bool final_init = false;
        FilmacRun s{0, 0, 0};
        for (int f = 0; f < 40; f++) {
            long minv = (long)(rng() % (uint64_t)(S * 6 / 10 + 1)), maxv = S * 4 / 10 + (long)(rng() % (uint64_t)(S * 6 / 10 + 1));
            if (minv >= maxv) maxv = minv + 1;
            if (!final_init) { final_init = true; final_minv = minv; final_maxv = maxv; }
            else {
                if (final_maxv < maxv) final_maxv = ((final_maxv * 1l) + maxv) / 2l;
                else final_maxv = ((final_maxv * 4l) + maxv) / 5l;
                if (final_minv > minv) final_minv = ((final_minv * 1l) + minv) / 2l;
                else final_minv = ((final_minv * 4l) + minv) / 5l;
            }
            s = filmac_step(s, FilmacLevels{minv, maxv});
            EXPECT(s.init == 1 && s.final_minv == final_minv && s.final_maxv == final_maxv, "step run %d frame %d", run, f);
            EXPECT(s.final_maxv > s.final_minv, "range closed: run %d frame %d", run, f);
        }
    }

    // ---- the table: 10^4 random pairs, a denominator of 1, minima above every pixel, maxima below; every byte
    for (int i = 0; i < 10000; i++) {
        const bool gamma = (i & 1) != 0;
        const long S = (long)filmac_scale(gamma);
        long fmin = (long)(rng() % (uint64_t)(S + 1)), fmax;
        switch (i % 5) {
        case 0: fmax = fmin + 1; break;                                           // denominator 1: everything runs into the clamp
        case 1: fmin = S + (long)(rng() % 65536); fmax = fmin + 1 + (long)(rng() % (uint64_t)S); break;   // above every pixel
        case 2: fmax = fmin + 1 + (long)(rng() % 70000); break;                   // narrow
        default: fmax = fmin + 1 + (long)(rng() % (uint64_t)S); break;
        }
        for (uint32_t b = 0; b < 256; b++) {
            const long Lv = (long)(gamma ? dec_tab[b] : b) << 16;
            const int want = tool_byte(Lv, fmin, (long long)(fmax - fmin), S, gamma);
            const int got = filmac_map(b, fmin, fmax, gamma ? dec_tab : nullptr, gamma ? enc_tab : nullptr);
            EXPECT(got == want, "map byte %u of (%ld, %ld) gamma %d: %d, want %d", b, fmin, fmax, (int)gamma, got, want);
        }
    }
    // what only set_state() can bring about: a denominator of 0 counts as 1, a negative one divides as C does; the
    // widest state that is accepted stays inside 64 bits (the sanitized build would say otherwise)
    for (int gamma = 0; gamma < 2; gamma++) {
        const long S = (long)filmac_scale(gamma != 0);
        const uint16_t *dec = gamma ? dec_tab : nullptr;
        const uint8_t *enc = gamma ? enc_tab : nullptr;
        for (uint32_t b = 0; b < 256; b++) {
            const long Lv = (long)(gamma ? dec_tab[b] : b) << 16;
            EXPECT(filmac_map(b, 5 << 16, 5 << 16, dec, enc) == tool_byte(Lv, 5 << 16, 1, S, gamma != 0), "zero denominator, byte %u", b);
            EXPECT(filmac_map(b, 9 << 16, 3 << 16, dec, enc) == tool_byte(Lv, 9 << 16, -(6 << 16), S, gamma != 0), "negative denominator, byte %u", b);
            for (int64_t lo : {-FILMAC_STATE_LIMIT, (int64_t)0, FILMAC_STATE_LIMIT})
                for (int64_t hi : {-FILMAC_STATE_LIMIT, (int64_t)1, FILMAC_STATE_LIMIT})
                    EXPECT(filmac_map(b, lo, hi, dec, enc) == tool_byte(Lv, (long)lo, hi - lo ? (long long)(hi - lo) : 1, S, gamma != 0), "limits, byte %u", b);
        }
    }
    std::printf("%ld checks, %ld bad\n", checks, bad);
    return bad ? 1 : 0;
}

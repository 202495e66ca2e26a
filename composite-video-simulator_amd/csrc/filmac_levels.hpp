// filmac_levels.hpp -- the arithmetic of the filmac stage (include/ntscsim.h: ntscsim_filmac_*) on plain integers: which
// 128 x 128 blocks of a frame are measured, the rounded mean of a block, the levels of a frame from its block records,
// one step of the frame-to-frame recurrence, and the byte table that is the stretch of one frame.  No HIP in this
// file: the kernels (csrc/ntsc_filmac.hip) call these functions, and tests/filmac_levels_check.cpp sweeps them with
// plain g++ against the tool's loops.  Line numbers refer to filmac.cpp of the reference.  
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FILMAC_HOST_DEVICE __host__ __device__ inline
#else
#define FILMAC_HOST_DEVICE inline
#endif

namespace ntscsim {

constexpr int FILMAC_BLOCK = 128;        // blw, blh :895
constexpr int FILMAC_MIN_SIZE = 16;      // :705
constexpr int FILMAC_MAX_SIZE = 16384;   // a block record's sum: 128 * 128 * 8192 = 2^27; blocks of a frame: 96 * 128
constexpr int64_t FILMAC_STATE_LIMIT = (int64_t)1 << 32;   // |final_minv|, |final_maxv| that set_state() accepts

// scaleto :886
FILMAC_HOST_DEVICE int64_t filmac_scale(bool gamma) { return gamma ? (int64_t)0x10000 * 8192 : (int64_t)0x10000 * 256; }

struct FilmacGrid {                      // the blocks of a frame :891-898
    int x0;                              // minx = W * 15 / 100
    int nbx, nby;                        // blocks in a row of blocks: x0, x0 + 128, ... < W * 90 / 100; rows of blocks
};
struct FilmacBox { int x, y, w, h; };    // one block, clipped by the frame alone :904

FILMAC_HOST_DEVICE FilmacGrid filmac_grid(int W, int H)
{
    const unsigned minx = ((unsigned)W * 15u) / 100u, maxx = ((unsigned)W * 90u) / 100u;
    FilmacGrid g;
    g.x0 = (int)minx;
    g.nbx = maxx > minx ? (int)((maxx - minx + (unsigned)FILMAC_BLOCK - 1u) / (unsigned)FILMAC_BLOCK) : 0;
    g.nby = (H + FILMAC_BLOCK - 1) / FILMAC_BLOCK;
    return g;
}

// block b of g.nbx * g.nby, row of blocks by row of blocks.  The last block of a row runs past W * 90 / 100 up to W.
FILMAC_HOST_DEVICE FilmacBox filmac_box(const FilmacGrid &g, int W, int H, int b)
{
    const int by = b / g.nbx, bx = b - by * g.nbx;
    FilmacBox o;
    o.x = g.x0 + bx * FILMAC_BLOCK;
    o.y = by * FILMAC_BLOCK;
    o.w = W - o.x < FILMAC_BLOCK ? W - o.x : FILMAC_BLOCK;
    o.h = H - o.y < FILMAC_BLOCK ? H - o.y : FILMAC_BLOCK;
    return o;
}

// What a workgroup leaves of one block.  sum: of min(B, G, R) per pixel, as the byte without gamma and as
// gamma_dec16 of the byte with it -- the decode table does not decrease, so the smallest of three decoded values is
// the decoded smallest byte, and the tool's << 16 is applied once to the sum.  top: the largest byte of B, G, R.
struct FilmacBlockRec { uint32_t sum, count, top, _pad; };

// grmin :914-915: (sum of L + grd / 2) / grd with L = value << 16
FILMAC_HOST_DEVICE int64_t filmac_block_mean(uint32_t sum, uint32_t count)
{
    return (((int64_t)sum << 16) + (int64_t)(count / 2u)) / (int64_t)count;
}

// L of one byte :866 / :879; dec: gamma_dec16_table, or NULL without gamma
FILMAC_HOST_DEVICE int64_t filmac_widen(uint32_t byte, const uint16_t *dec) { return (int64_t)(dec ? dec[byte] : byte) << 16; }

struct FilmacLevels { int64_t minv, maxv; };

// the start values :887-888, and what one block does to them :910, :919-920
FILMAC_HOST_DEVICE FilmacLevels filmac_levels_start(int64_t scale) { return FilmacLevels{(scale * 6) / 10, (scale * 4) / 10}; }
FILMAC_HOST_DEVICE FilmacLevels filmac_levels_add(FilmacLevels l, const FilmacBlockRec &r, const uint16_t *dec)
{
    const int64_t mean = filmac_block_mean(r.sum, r.count), top = filmac_widen(r.top, dec);
    if (l.minv > mean) l.minv = mean;
    if (l.maxv < top) l.maxv = top;
    return l;
}
// two partial results of one frame (the kernel reduces lanes; min and max commute), and the end :925
FILMAC_HOST_DEVICE FilmacLevels filmac_levels_join(FilmacLevels a, FilmacLevels b)
{
    return FilmacLevels{a.minv < b.minv ? a.minv : b.minv, a.maxv > b.maxv ? a.maxv : b.maxv};
}
FILMAC_HOST_DEVICE FilmacLevels filmac_levels_end(FilmacLevels l)
{
    if (l.minv == l.maxv) l.maxv++;
    return l;
}

// the frame levels :887-925 from the records of all of a frame's blocks
FILMAC_HOST_DEVICE FilmacLevels filmac_levels(const FilmacBlockRec *recs, int n, int64_t scale, const uint16_t *dec)
{
    FilmacLevels l = filmac_levels_start(scale);
    for (int i = 0; i < n; i++) l = filmac_levels_add(l, recs[i], dec);
    return filmac_levels_end(l);
}

struct FilmacRun { int64_t init, final_minv, final_maxv; };   // final_init, final_minv, final_maxv :828-829

// :927-942
FILMAC_HOST_DEVICE FilmacRun filmac_step(FilmacRun s, FilmacLevels l)
{
    if (!s.init) return FilmacRun{1, l.minv, l.maxv};
    s.final_maxv = s.final_maxv < l.maxv ? (s.final_maxv + l.maxv) / 2 : (s.final_maxv * 4 + l.maxv) / 5;
    s.final_minv = s.final_minv > l.minv ? (s.final_minv + l.minv) / 2 : (s.final_minv * 4 + l.minv) / 5;
    return s;
}

// The output byte of input byte `byte` :949-951 and :986 / :1000: the stretch depends on the byte and on the frame's
// (final_minv, final_maxv) alone, so a frame's stretch is 256 of these.  dec / enc: the gamma tables, both NULL
// without gamma.  The levels of real frames keep final_maxv above final_minv; set_state() can
// put anything there, so a denominator of 0, at which the tool would stop with a division fault, counts as 1, and a
// negative one divides as the tool's signed division does.  |final_*| <= 2^32 keeps the product inside 64 bits.
FILMAC_HOST_DEVICE uint8_t filmac_map(uint32_t byte, int64_t final_minv, int64_t final_maxv, const uint16_t *dec, const uint8_t *enc)
{
    const int64_t scale = filmac_scale(dec != nullptr);
    int64_t den = final_maxv - final_minv;
    if (den == 0) den = 1;
    int64_t v = ((filmac_widen(byte, dec) - final_minv) * scale) / den;         // truncates toward zero
    if (v < -0x7FFFFFFFll) v = -0x7FFFFFFFll;
    if (v > 0x7FFFFFFFll) v = 0x7FFFFFFFll;
    int64_t t = v >> 16;                                                        // arithmetic
    if (t < 0) t = 0;
    if (enc) return enc[t > 8192 ? 8192 : t];                                   // gamma_enc16 :664-670; at most 255
    return (uint8_t)(t > 255 ? 255 : t);
}

} // namespace ntscsim

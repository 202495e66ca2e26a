// key_host.hpp -- host pieces the two halves of the colorkey stage share (csrc/key_params.cpp, csrc/ntsc_key.hip):
// how the rand() draws of one noisy layer of one frame are dealt to the lanes of k_key_draw.
#pragma once
#include <cstdint>
#include <vector>

#include "glibc_rand.hpp"

namespace ntscsim {

// One lane of k_key_draw owns KEY_RUN_PIXELS consecutive pixels (raster order) of one noisy (frame, layer): 3 draws
// per pixel, 8 whole words of the hit bitmap.  Lane j starts 3 * KEY_RUN_PIXELS * j draws behind the layer's first.
constexpr int KEY_RUN_PIXELS = 256;
constexpr int KEY_RUN_WORDS = KEY_RUN_PIXELS / 32;
constexpr uint64_t KEY_RUN_DRAWS = 3ull * KEY_RUN_PIXELS;

inline uint32_t key_lanes_per_job(int W, int H)
{
    return (uint32_t)(((uint64_t)W * (uint64_t)H + KEY_RUN_PIXELS - 1) / KEY_RUN_PIXELS);
}

// x^(KEY_RUN_DRAWS * j) for j = 0 .. lanes-1, coefficient-major: out[k * lanes + j] (lanes of a wave read
// consecutive words)
void key_lane_polys(uint32_t lanes, std::vector<uint32_t> &out);

// the window a lane starts from: what jump61 computes on the device (out[i] = sum_k c[k] * w[i + k] over the
// 61-word extension of the job's window), on the host
RandState key_lane_state(const uint32_t *polys, uint32_t lanes, uint32_t lane, const RandState &job);

} // namespace ntscsim

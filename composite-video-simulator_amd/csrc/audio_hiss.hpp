// audio_hiss.hpp -- the hiss draws of the audio stages (csrc/ntsc_audio.hip, csrc/ntsc_cass.hip): k_audio_hiss makes
// the numerators of a call's channel-samples ahead of the chain, by jump-ahead from each block's own rand() position.
// The kernel lives in ntsc_audio.hip; this is what a second translation unit needs to call it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glibc_rand.hpp"
#include "ntsc_stage.hpp"

namespace ntscsim {

constexpr int HISS_ROUNDS = 16;
constexpr int HISS_CHUNK = 31 * HISS_ROUNDS;   // draws of one lane of k_audio_hiss
constexpr int HISS_POLYS = 26;           // x^(HISS_CHUNK * 2^j): 2^33 draws of a block are 2^25 chunks at the most

struct AudioHissBlock {                  // rand() window at the block's position; first: its first channel-sample in the call
    uint32_t w[31];
    int32_t level;                       // the hiss level of the block's stream: the blocks of one launch may differ in it
    uint64_t first, items;
};

// The window of a block whose first draw is at position p.  seq / seq_pos: a generator the caller keeps across the
// blocks of a call (seq_pos UINT64_MAX: it stands nowhere) -- small blocks that follow each other (the tool's packets)
// step it instead of jumping.
inline void audio_hiss_window(AudioHissBlock &h, RandSeq &seq, uint64_t &seq_pos, uint64_t p, uint64_t first, uint64_t items, int level)
{
    if (seq_pos == UINT64_MAX || p < seq_pos || p - seq_pos > 65536) {
        seq = RandSeq(rand_state_at(p));
        seq_pos = p;
    }
    for (; seq_pos < p; seq_pos++) (void)seq.next();
    for (int j = 0; j < 31; j++) h.w[j] = seq.r[(seq.i + j) % 31];
    h.level = level;
    h.first = first;
    h.items = items;
}

// HISS_POLYS polynomials in device memory (the caller frees them)
int audio_hiss_polys(const CtxStageView &v, uint32_t **polys);
// k_audio_hiss over m blocks (device records) whose longest has max_items draws: out[first + i] = numerator of draw i
// at the block's level
void audio_hiss_launch(const AudioHissBlock *blocks, int m, uint64_t max_items, const uint32_t *polys, int32_t *out, hipStream_t st);

} // namespace ntscsim

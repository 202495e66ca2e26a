// ntsc_stage.hpp -- the host scaffold of the device stages that are translation units of their own (frameblend:
// csrc/ntsc_blend.hip, colorkey: csrc/ntsc_key.hip, average_delay: csrc/ntsc_avg.hip, scanimate: csrc/ntsc_scan.hip, vhsled: csrc/ntsc_led.hip, filmac: csrc/ntsc_filmac.hip, posterize and colormap: csrc/ntsc_pixmap.hip, the audio chain: csrc/ntsc_audio.hip, the cassette chain: csrc/ntsc_cass.hip): what they see of an ntscsim_ctx,
// whose definition stays private to ntscsim_hip.hip, the pinned record slots their launches go up through, and the
// arena their *_frames_host() calls copy host frames through.  The host logic without HIP in it: ntsc_frames.hpp (every
// stage's); what only the two layer stages share: ntsc_layer.hpp (no HIP in it either) and ntsc_layer_frames.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "ntscsim.h"

struct ntscsim_ctx;

namespace ntscsim {

struct BlendState;                       // ntsc_blend.hip: bound params, tables, record slots, host-frame arena
struct KeyState;                         // ntsc_key.hip: bound params, record slots, noise bits, host-frame arena
struct AvgState;                         // ntsc_avg.hip: bound params, record slots, host-frame arena
struct ScanState;                        // ntsc_scan.hip: bound params, record slots, accumulator planes, sine tables, host-frame arena
struct LedState;                         // ntsc_led.hip: bound params, record slots, edges plane of the debug tap, host-frame arena
struct FilmacState;                      // ntsc_filmac.hip: bound params, gamma tables, level state, record slots, scratch, host-frame arena
struct PostState;                        // ntsc_pixmap.hip: bound size, the inputs' masks, record slots, host-frame arena
struct CmapState;                        // ntsc_pixmap.hip: bound size, the colour table, record slots, host-frame arena
struct AudioStageState;                  // ntsc_audio.hip: bound params, carried chain state, draw polynomials, scratch, record slots, staging
struct CassStageState;                   // ntsc_cass.hip: bound params, carried chain state and history, scratch planes, tilt staging, record slots

struct CtxStageView {
    int device;
    hipStream_t stream;                  // the ctx's own stream
    std::string *err;                    // ntscsim_last_error
    std::string *kernels;                // ntscsim_debug_last_kernels
    BlendState **blend;                  // owned by the ctx, freed by ntscsim_destroy() through the *_state_destroy()
    KeyState **key;
    AvgState **avg;
    ScanState **scan;
    LedState **led;
    FilmacState **filmac;
    PostState **post;
    CmapState **cmap;
    AudioStageState **audio;
    CassStageState **cass;
};
CtxStageView ctx_stage_view(ntscsim_ctx *c);     // ntscsim_hip.hip
void blend_state_destroy(BlendState *b);         // ntsc_blend.hip
void key_state_destroy(KeyState *k);             // ntsc_key.hip
void avg_state_destroy(AvgState *k);             // ntsc_avg.hip
void scan_state_destroy(ScanState *k);           // ntsc_scan.hip
void led_state_destroy(LedState *k);             // ntsc_led.hip
void filmac_state_destroy(FilmacState *k);       // ntsc_filmac.hip
void post_state_destroy(PostState *k);           // ntsc_pixmap.hip
void cmap_state_destroy(CmapState *k);           // ntsc_pixmap.hip
void audio_state_destroy(AudioStageState *k);    // ntsc_audio.hip
void cass_state_destroy(CassStageState *k);      // ntsc_cass.hip
// ntscsim_debug_last_kernels(): "k_scan_splat" becomes "k_scan_splat+spill" if a workgroup of the last call spilled
void scan_kernels_tap(ScanState *k, int device, std::string &kernels);   // ntsc_scan.hip

#define STAGECHK(view, call)                                                           \
    do {                                                                               \
        hipError_t e__ = (call);                                                       \
        if (e__ != hipSuccess) {                                                       \
            *(view).err = std::string(#call) + ": " + hipGetErrorString(e__);          \
            return NTSCSIM_E_HIP;                                                      \
        }                                                                              \
    } while (0)

struct RecordSlot {                      // records of one launch: pinned host copy, device copy, "launch finished"
    unsigned char *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool used = false;
};

// Four slots taken in turn, so that a call returns while its records are still being read.  Slot: RecordSlot, or a
// struct derived from it that keeps more per launch (free that before release()).
template <class Slot = RecordSlot>
struct RecordSlots {
    Slot slot[4];
    int idx = 0;

    // the next slot, free (its last launch has finished) and holding `bytes` at the least
    int acquire(const CtxStageView &v, size_t bytes, Slot *&out)
    {
        Slot &s = slot[idx];
        idx = (idx + 1) & 3;
        if (!s.done) STAGECHK(v, hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        if (s.used) STAGECHK(v, hipEventSynchronize(s.done));
        if (bytes > s.cap) {
            if (s.host) { (void)hipHostFree(s.host); s.host = nullptr; }
            if (s.dev) { (void)hipFree(s.dev); s.dev = nullptr; }
            s.cap = 0;
            const size_t want = bytes + bytes / 4 + 4096;
            STAGECHK(v, hipHostMalloc((void **)&s.host, want, hipHostMallocPortable));
            STAGECHK(v, hipMalloc((void **)&s.dev, want));
            s.cap = want;
        }
        out = &s;
        return NTSCSIM_OK;
    }

    // *_bind(): launches in flight read what bind replaces
    int wait_all(const CtxStageView &v)
    {
        for (Slot &s : slot)
            if (s.used) STAGECHK(v, hipEventSynchronize(s.done));
        return NTSCSIM_OK;
    }

    void release()
    {
        for (Slot &s : slot) {
            if (s.host) (void)hipHostFree(s.host);
            if (s.dev) (void)hipFree(s.dev);
            if (s.done) (void)hipEventDestroy(s.done);
        }
    }
};

// The tail of a *_launch(): the kernels just enqueued on st have been accepted, slot s (NULL: the kernels are not the
// last that read it) is busy until they finish, and `name` joins ntscsim_debug_last_kernels().  A failure leaves no name.
inline int stage_launched(const CtxStageView &v, RecordSlot *s, hipStream_t st, const std::string &name)
{
    STAGECHK(v, hipGetLastError());
    if (s) {
        STAGECHK(v, hipEventRecord(s->done, st));
        s->used = true;
    }
    if (!v.kernels->empty()) *v.kernels += ';';
    *v.kernels += name;
    return NTSCSIM_OK;
}

struct FrameArena {                      // *_frames_host(): the call's frames in device memory, and pinned staging
    unsigned char *arena = nullptr, *staging = nullptr;
    size_t arena_cap = 0, staging_cap = 0;

    int reserve(const CtxStageView &v, size_t arena_bytes, size_t staging_bytes)
    {
        if (arena_bytes > arena_cap) {
            if (arena) { (void)hipFree(arena); arena = nullptr; arena_cap = 0; }
            STAGECHK(v, hipMalloc((void **)&arena, arena_bytes));
            arena_cap = arena_bytes;
        }
        if (staging_bytes > staging_cap) {
            if (staging) { (void)hipHostFree(staging); staging = nullptr; staging_cap = 0; }
            STAGECHK(v, hipHostMalloc((void **)&staging, staging_bytes, hipHostMallocPortable));
            staging_cap = staging_bytes;
        }
        return NTSCSIM_OK;
    }

    void release()
    {
        if (arena) (void)hipFree(arena);
        if (staging) (void)hipHostFree(staging);
    }
};

} // namespace ntscsim

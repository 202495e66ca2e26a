// ntsc_blend.hpp -- what csrc/ntsc_blend.hip (the frameblend stage, a translation unit of its own) sees of an
// ntscsim_ctx, whose definition stays private to ntscsim_hip.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

struct ntscsim_ctx;

namespace ntscsim {

struct BlendState;                       // ntsc_blend.hip: bound params, tables, record slots, host-frame arenas

struct CtxBlendView {
    int device;
    hipStream_t stream;                  // the ctx's own stream
    std::string *err;                    // ntscsim_last_error
    std::string *kernels;                // ntscsim_debug_last_kernels
    BlendState **blend;                  // owned by the ctx, freed by ntscsim_destroy() through blend_state_destroy()
};
CtxBlendView ctx_blend_view(ntscsim_ctx *c);     // ntscsim_hip.hip
void blend_state_destroy(BlendState *b);         // ntsc_blend.hip

} // namespace ntscsim

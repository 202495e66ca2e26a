// ntsc_key.hpp -- what csrc/ntsc_key.hip (the colorkey stage, a translation unit of its own) sees of an
// ntscsim_ctx, whose definition stays private to ntscsim_hip.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

struct ntscsim_ctx;

namespace ntscsim {

struct KeyState;                         // ntsc_key.hip: bound params, record slots, noise bits, host-frame arenas

struct CtxKeyView {
    int device;
    hipStream_t stream;                  // the ctx's own stream
    std::string *err;                    // ntscsim_last_error
    std::string *kernels;                // ntscsim_debug_last_kernels
    KeyState **key;                      // owned by the ctx, freed by ntscsim_destroy() through key_state_destroy()
};
CtxKeyView ctx_key_view(ntscsim_ctx *c);         // ntscsim_hip.hip
void key_state_destroy(KeyState *k);             // ntsc_key.hip

} // namespace ntscsim

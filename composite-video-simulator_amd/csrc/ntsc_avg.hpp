// ntsc_avg.hpp -- what csrc/ntsc_avg.hip (the average_delay stage, a translation unit of its own) sees of an
// ntscsim_ctx, whose definition stays private to ntscsim_hip.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

struct ntscsim_ctx;

namespace ntscsim {

struct AvgState;                         // ntsc_avg.hip: bound params, record slots, host-frame arenas

struct CtxAvgView {
    int device;
    hipStream_t stream;                  // the ctx's own stream
    std::string *err;                    // ntscsim_last_error
    std::string *kernels;                // ntscsim_debug_last_kernels
    AvgState **avg;                      // owned by the ctx, freed by ntscsim_destroy() through avg_state_destroy()
};
CtxAvgView ctx_avg_view(ntscsim_ctx *c);         // ntscsim_hip.hip
void avg_state_destroy(AvgState *k);             // ntsc_avg.hip

} // namespace ntscsim

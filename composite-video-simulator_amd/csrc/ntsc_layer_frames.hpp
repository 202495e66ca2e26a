// ntsc_layer_frames.hpp -- *_frames_host() of the layer stages (colorkey: csrc/ntsc_key.hip, average_delay:
// csrc/ntsc_avg.hip): the plan of ntsc_layer.hpp carried out through the stage's FrameArena.
#pragma once
#include <vector>

#include "ntsc_layer.hpp"
#include "ntsc_stage.hpp"

namespace ntscsim {

// *_frames_host() of a layer stage: every distinct frame of the call up once, packed to 16-byte pitched rows,
// frames_device(descriptors, n, stream) on the copies, the destinations down.  Synchronous.
template <class Desc, class FramesDevice>
int layer_frames_host(const CtxStageView &v, FrameArena &a, const LayerGeom &g, const Desc *descs, int n, FramesDevice &&frames_device)
{
    STAGECHK(v, hipSetDevice(v.device));
    HostFrames p;
    int rc = host_frames_plan(g, descs, n, p);
    if (rc != NTSCSIM_OK || n == 0) return rc;
    rc = a.reserve(v, p.order.size() * p.fb, p.fb);
    if (rc != NTSCSIM_OK) return rc;
    const size_t row = (size_t)g.W * 4;
    hipStream_t st = v.stream;
    for (const HostFrame &f : p.order) {
        copy_rows(a.staging, p.pitch, f.first, (size_t)f.second, row, g.H);
        STAGECHK(v, hipMemcpyAsync(a.arena + p.where[f], a.staging, p.fb, hipMemcpyHostToDevice, st));
        STAGECHK(v, hipStreamSynchronize(st));
    }
    std::vector<Desc> dd;
    std::vector<LayerSrcOf<Desc>> ll;
    host_frames_rebase(p, a.arena, descs, n, dd, ll);
    rc = frames_device(dd.data(), n, st);
    if (rc != NTSCSIM_OK) return rc;
    for (const HostFrame &f : p.dsts) {
        STAGECHK(v, hipMemcpyAsync(a.staging, a.arena + p.where[f], p.fb, hipMemcpyDeviceToHost, st));
        STAGECHK(v, hipStreamSynchronize(st));
        copy_rows(const_cast<void *>(f.first), (size_t)f.second, a.staging, p.pitch, row, g.H);
    }
    return NTSCSIM_OK;
}

} // namespace ntscsim

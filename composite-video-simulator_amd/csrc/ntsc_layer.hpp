// ntsc_layer.hpp -- the host logic only the layer stages share (colorkey: csrc/ntsc_key.hip, average_delay:
// csrc/ntsc_avg.hip): what a descriptor of bound layers must satisfy, a clip call's frames as descriptors, which host
// frames are one frame.  Spans, the plane check, the in-order launch planner and the writes of a call are every stage's:
// ntsc_frames.hpp.  Templates over the stage's descriptor type: ntscsim_key_desc / ntscsim_avg_desc (and their _src)
// have the same fields up to the last uint64_t, which nothing here touches.  No HIP in it: plain C++, so that it can be
// driven without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

#include "ntscsim.h"
#include "ntsc_frames.hpp"

namespace ntscsim {

struct LayerGeom { int W, H, nl; };      // what the bound params fix for every descriptor

template <class Desc> using LayerSrcOf = typename std::remove_cv<typename std::remove_pointer<decltype(Desc::layers)>::type>::type;

template <class Desc>
int check_desc(const LayerGeom &g, const Desc &d)
{
    const int W = g.W, H = g.H;
    if (!d.dst_dev || (d.n_layers > 0 && !d.layers)) return NTSCSIM_E_ARG;
    if (d.width != W || d.height != H || d.n_layers != g.nl) return NTSCSIM_E_SIZE;
    if (plane_check(d.dst_dev, d.dst_linesize, W, true)) return NTSCSIM_E_SIZE;
    const Span ds = span_of(d.dst_dev, d.dst_linesize, H);
    for (int l = 0; l < d.n_layers; l++) {
        const auto &s = d.layers[l];
        if (!s.src_dev) continue;
        if (plane_check(s.src_dev, s.src_linesize, W, true)) return NTSCSIM_E_SIZE;
        if (overlaps(ds, span_of(s.src_dev, s.src_linesize, H))) return NTSCSIM_E_ARG;
    }
    return NTSCSIM_OK;
}

// *_frames_device(): every descriptor checked, then launch(first descriptor, count) for runs of at most `cap`
// descriptors, cut where descriptors depend on each other (frames_in_order()).  An absent layer reads nothing.
template <class Desc, class Launch>
int layer_frames_in_order(const LayerGeom &g, const Desc *descs, int n, int cap, Launch &&launch)
{
    for (int i = 0; i < n; i++) {
        const int rc = check_desc(g, descs[i]);
        if (rc != NTSCSIM_OK) return rc;
    }
    return frames_in_order(n, cap, [&](int i, std::vector<Span> &rd) {
        const Desc &d = descs[i];
        for (int l = 0; l < d.n_layers; l++)
            if (d.layers[l].src_dev) rd.push_back(span_of(d.layers[l].src_dev, d.layers[l].src_linesize, g.H));
        return span_of(d.dst_dev, d.dst_linesize, g.H);
    }, [&](int first, int m) { return launch(descs + first, m); });
}

// *_clip_device(): what the call writes (ring, outputs) must be disjoint from itself and from every source; then the
// clip's frames as descriptors (descs[t].layers points into lays; the last uint64_t is left 0 for the stage).
// every_linesize: src_linesize[l] is checked for every layer up front, one that is absent in every frame included;
// otherwise only on a frame where the layer is present.
template <class Desc>
int layer_clip_descs(const LayerGeom &g, int delay, void *const *ring_dev, int ring_linesize, const void *const *src_dev,
                     const int32_t *src_linesize, void *const *out_dev, int out_linesize, int T, bool every_linesize,
                     std::vector<Desc> &descs, std::vector<LayerSrcOf<Desc>> &lays)
{
    const int W = g.W, H = g.H, nl = g.nl;
    if (plane_check(nullptr, ring_linesize, W, true) || plane_check(nullptr, out_linesize, W, true)) return NTSCSIM_E_SIZE;
    CallWrites wr;
    for (int i = 0; i < delay; i++) {
        if (!ring_dev[i]) return NTSCSIM_E_ARG;
        if (plane_check(ring_dev[i], ring_linesize, W, true)) return NTSCSIM_E_SIZE;
        wr.add(span_of(ring_dev[i], ring_linesize, H));
    }
    for (int t = 0; t < T; t++) {
        if (!out_dev[t]) return NTSCSIM_E_ARG;
        if (plane_check(out_dev[t], out_linesize, W, true)) return NTSCSIM_E_SIZE;
        wr.add(span_of(out_dev[t], out_linesize, H));
    }
    if (wr.sort() != NTSCSIM_OK) return NTSCSIM_E_ARG;
    if (every_linesize)
        for (int l = 0; l < nl; l++)
            if (plane_check(nullptr, src_linesize[l], W, true)) return NTSCSIM_E_SIZE;
    descs.assign((size_t)T, Desc());
    lays.assign((size_t)T * (size_t)nl, LayerSrcOf<Desc>());
    for (int t = 0; t < T; t++) {
        Desc &d = descs[(size_t)t];
        d.dst_dev = out_dev[t]; d.dst_linesize = out_linesize; d.width = W; d.height = H; d.n_layers = nl;
        d.layers = lays.data() + (size_t)t * (size_t)nl;
        for (int l = 0; l < nl; l++) {
            auto &s = lays[(size_t)t * (size_t)nl + (size_t)l];
            s.src_dev = src_dev[(size_t)l * (size_t)T + (size_t)t];
            s.src_linesize = src_linesize[l];
            s._pad = 0;
            if (!s.src_dev) continue;
            // (with every_linesize the linesize has passed already: only the pointer can fail here)
            if (plane_check(s.src_dev, s.src_linesize, W, true)) return NTSCSIM_E_SIZE;
            if (wr.hits(span_of(s.src_dev, s.src_linesize, H))) return NTSCSIM_E_ARG;
        }
    }
    return NTSCSIM_OK;
}

// *_frames_host(): the distinct frames of the call, (pointer, linesize) -> offset in a device arena of frames with
// 16-byte pitched rows, and the frames the call writes.
typedef std::pair<const void *, int> HostFrame;
struct HostFrames {
    size_t pitch = 0, fb = 0;            // bytes of a row and of a frame in the arena
    std::map<HostFrame, size_t> where;
    std::vector<HostFrame> order, dsts;
};

template <class Desc>
int host_frames_plan(const LayerGeom &g, const Desc *descs, int n, HostFrames &p)
{
    const int W = g.W, H = g.H;
    p.pitch = ((size_t)W * 4 + 15) & ~(size_t)15;
    p.fb = p.pitch * (size_t)H;
    for (int i = 0; i < n; i++) {
        const Desc &d = descs[i];
        if (!d.dst_dev || (d.n_layers > 0 && !d.layers)) return NTSCSIM_E_ARG;
        if (d.width != W || d.height != H || d.n_layers != g.nl || plane_check(d.dst_dev, d.dst_linesize, W, false)) return NTSCSIM_E_SIZE;
        const HostFrame dk(d.dst_dev, d.dst_linesize);
        if (p.where.emplace(dk, p.order.size() * p.fb).second) p.order.push_back(dk);
        if (std::find(p.dsts.begin(), p.dsts.end(), dk) == p.dsts.end()) p.dsts.push_back(dk);
        for (int l = 0; l < d.n_layers; l++) {
            const auto &s = d.layers[l];
            if (!s.src_dev) continue;
            if (plane_check(s.src_dev, s.src_linesize, W, false)) return NTSCSIM_E_SIZE;
            const HostFrame sk(s.src_dev, s.src_linesize);
            if (p.where.emplace(sk, p.order.size() * p.fb).second) p.order.push_back(sk);
        }
    }
    // a frame that is written must be disjoint from every other frame of the call: two host frames that overlap without
    // being the same (pointer, linesize) would become two device frames, and the result would not be the tool's
    for (const HostFrame &dk : p.dsts)
        for (const HostFrame &ok : p.order)
            if (ok != dk && overlaps(span_of(dk.first, dk.second, H), span_of(ok.first, ok.second, H))) return NTSCSIM_E_ARG;
    return NTSCSIM_OK;
}

// the call's descriptors with every frame replaced by its copy in the arena
template <class Desc>
void host_frames_rebase(const HostFrames &p, unsigned char *arena, const Desc *descs, int n, std::vector<Desc> &dd,
                        std::vector<LayerSrcOf<Desc>> &ll)
{
    dd.assign(descs, descs + n);
    size_t nsrc = 0;
    for (int i = 0; i < n; i++) nsrc += (size_t)descs[i].n_layers;
    ll.assign(nsrc, LayerSrcOf<Desc>());
    LayerSrcOf<Desc> *first = ll.data();
    for (int i = 0; i < n; i++) {
        Desc &d = dd[(size_t)i];
        d.dst_dev = arena + p.where.at(HostFrame(descs[i].dst_dev, descs[i].dst_linesize));
        d.dst_linesize = (int)p.pitch;
        for (int l = 0; l < d.n_layers; l++) {
            const auto &s = descs[i].layers[l];
            first[l].src_dev = s.src_dev ? arena + p.where.at(HostFrame(s.src_dev, s.src_linesize)) : nullptr;
            first[l].src_linesize = (int)p.pitch;
            first[l]._pad = 0;
        }
        d.layers = first;
        first += d.n_layers;
    }
}

} // namespace ntscsim

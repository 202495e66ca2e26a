// ntsc_layer.hpp -- the host logic the layer stages share (colorkey: csrc/ntsc_key.hip, average_delay: csrc/ntsc_avg.hip):
// what a call may alias, where a run of descriptors has to be cut into launches, which host frames are one frame.
// Templates over the stage's descriptor type: ntscsim_key_desc / ntscsim_avg_desc (and their _src) have the same fields
// up to the last uint64_t, which nothing here touches.  No HIP in it: plain C++, so that it can be driven without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

#include "ntscsim.h"

namespace ntscsim {

struct Span { uintptr_t a, b; };
inline bool overlaps(const Span &x, const Span &y) { return x.a < y.b && y.a < x.b; }
inline Span span_of(const void *p, int ls, int H) { return Span{(uintptr_t)p, (uintptr_t)p + (size_t)ls * (size_t)H}; }

struct LayerGeom { int W, H, nl; };      // what the bound params fix for every descriptor

template <class Desc> using LayerSrcOf = typename std::remove_cv<typename std::remove_pointer<decltype(Desc::layers)>::type>::type;

template <class Desc>
int check_desc(const LayerGeom &g, const Desc &d)
{
    const int W = g.W, H = g.H;
    if (!d.dst_dev || (d.n_layers > 0 && !d.layers)) return NTSCSIM_E_ARG;
    if (d.width != W || d.height != H || d.n_layers != g.nl) return NTSCSIM_E_SIZE;
    if (d.dst_linesize < 4 * W || (d.dst_linesize & 3) || ((uintptr_t)d.dst_dev & 3)) return NTSCSIM_E_SIZE;
    const Span ds = span_of(d.dst_dev, d.dst_linesize, H);
    for (int l = 0; l < d.n_layers; l++) {
        const auto &s = d.layers[l];
        if (!s.src_dev) continue;
        if (s.src_linesize < 4 * W || (s.src_linesize & 3) || ((uintptr_t)s.src_dev & 3)) return NTSCSIM_E_SIZE;
        if (overlaps(ds, span_of(s.src_dev, s.src_linesize, H))) return NTSCSIM_E_ARG;
    }
    return NTSCSIM_OK;
}

// *_frames_device(): every descriptor checked, then launch(first descriptor, count) for runs of at most `cap`
// descriptors.  Descriptors take effect in order: a launch ends in front of the first descriptor that writes what the
// launch reads or writes, or reads what it writes.
template <class Desc, class Launch>
int layer_frames_in_order(const LayerGeom &g, const Desc *descs, int n, int cap, Launch &&launch)
{
    for (int i = 0; i < n; i++) {
        const int rc = check_desc(g, descs[i]);
        if (rc != NTSCSIM_OK) return rc;
    }
    const int H = g.H;
    std::vector<Span> wr, rd;
    int first = 0;
    for (int i = 0; i <= n; i++) {
        bool cut = i == n || i - first >= cap;
        if (!cut) {
            const Desc &d = descs[i];
            const Span ds = span_of(d.dst_dev, d.dst_linesize, H);
            for (const Span &w : wr) if (overlaps(ds, w)) { cut = true; break; }
            for (size_t j = 0; !cut && j < rd.size(); j++) cut = overlaps(ds, rd[j]);
            for (int l = 0; !cut && l < d.n_layers; l++) {
                if (!d.layers[l].src_dev) continue;
                const Span ss = span_of(d.layers[l].src_dev, d.layers[l].src_linesize, H);
                for (const Span &w : wr) if (overlaps(ss, w)) { cut = true; break; }
            }
        }
        if (cut && i > first) {
            const int rc = launch(descs + first, i - first);
            if (rc != NTSCSIM_OK) return rc;
            first = i;
            wr.clear(); rd.clear();
        }
        if (i < n) {
            const Desc &d = descs[i];
            wr.push_back(span_of(d.dst_dev, d.dst_linesize, H));
            for (int l = 0; l < d.n_layers; l++)
                if (d.layers[l].src_dev) rd.push_back(span_of(d.layers[l].src_dev, d.layers[l].src_linesize, H));
        }
    }
    return NTSCSIM_OK;
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
    if (ring_linesize < 4 * W || (ring_linesize & 3) || out_linesize < 4 * W || (out_linesize & 3)) return NTSCSIM_E_SIZE;
    std::vector<Span> wr;
    for (int i = 0; i < delay; i++) {
        if (!ring_dev[i]) return NTSCSIM_E_ARG;
        if ((uintptr_t)ring_dev[i] & 3) return NTSCSIM_E_SIZE;
        wr.push_back(span_of(ring_dev[i], ring_linesize, H));
    }
    for (int t = 0; t < T; t++) {
        if (!out_dev[t]) return NTSCSIM_E_ARG;
        if ((uintptr_t)out_dev[t] & 3) return NTSCSIM_E_SIZE;
        wr.push_back(span_of(out_dev[t], out_linesize, H));
    }
    const auto by_start = [](const Span &x, const Span &y) { return x.a < y.a; };
    std::sort(wr.begin(), wr.end(), by_start);
    for (size_t i = 1; i < wr.size(); i++)
        if (wr[i].a < wr[i - 1].b) return NTSCSIM_E_ARG;
    if (every_linesize)
        for (int l = 0; l < nl; l++)
            if (src_linesize[l] < 4 * W || (src_linesize[l] & 3)) return NTSCSIM_E_SIZE;
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
            if (s.src_linesize < 4 * W || (s.src_linesize & 3) || ((uintptr_t)s.src_dev & 3)) return NTSCSIM_E_SIZE;
            const Span ss = span_of(s.src_dev, s.src_linesize, H);
            auto it = std::upper_bound(wr.begin(), wr.end(), ss, by_start);
            if (it != wr.end() && overlaps(ss, *it)) return NTSCSIM_E_ARG;
            if (it != wr.begin() && overlaps(ss, *(it - 1))) return NTSCSIM_E_ARG;
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
        if (d.width != W || d.height != H || d.n_layers != g.nl || d.dst_linesize < 4 * W) return NTSCSIM_E_SIZE;
        const HostFrame dk(d.dst_dev, d.dst_linesize);
        if (p.where.emplace(dk, p.order.size() * p.fb).second) p.order.push_back(dk);
        if (std::find(p.dsts.begin(), p.dsts.end(), dk) == p.dsts.end()) p.dsts.push_back(dk);
        for (int l = 0; l < d.n_layers; l++) {
            const auto &s = d.layers[l];
            if (!s.src_dev) continue;
            if (s.src_linesize < 4 * W) return NTSCSIM_E_SIZE;
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

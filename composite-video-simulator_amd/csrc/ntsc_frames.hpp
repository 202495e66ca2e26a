// ntsc_frames.hpp -- the host logic every device stage shares (frameblend: csrc/ntsc_blend.hip, colorkey: csrc/ntsc_key.hip,
// average_delay: csrc/ntsc_avg.hip, scanimate: csrc/ntsc_scan.hip, vhsled: csrc/ntsc_led.hip, filmac: csrc/ntsc_filmac.hip, posterize and colormap: csrc/ntsc_pixmap.hip): the bytes a frame covers,
// what a plane of pixels must satisfy, where a run of descriptors has to be cut into launches, what a call writes, and
// the copy between two row pitches.  No HIP in it: plain C++, so that it can be driven without a GPU
// (tests/frames_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ntscsim.h"

namespace ntscsim {

struct Span { uintptr_t a, b; };
inline bool overlaps(const Span &x, const Span &y) { return x.a < y.b && y.a < x.b; }
inline Span span_of(const void *p, int ls, int H) { return Span{(uintptr_t)p, (uintptr_t)p + (size_t)ls * (size_t)H}; }

// a plane whose rows hold w BGRA pixels.  aligned: a device call, whose kernels move dwords; the rows of a host frame
// are copied byte by byte and may lie anywhere
inline int plane_check(const void *p, int linesize, int w, bool aligned)
{
    if (linesize < 4 * w) return NTSCSIM_E_SIZE;
    if (aligned && ((linesize & 3) || ((uintptr_t)p & 3))) return NTSCSIM_E_SIZE;
    return NTSCSIM_OK;
}

// s overlaps one of the spans [p, end)
inline bool hits_any(Span s, const Span *p, const Span *end)
{
    for (; p != end; ++p)
        if (overlaps(s, *p)) return true;
    return false;
}

// Descriptors 0 .. n - 1 take effect in order: launch(first, count) for runs of at most `cap` descriptors, and a run
// ends in front of the first descriptor that writes what the run reads or writes, or reads what it writes.
// touch(i, rd) returns the span descriptor i writes and appends the spans it reads to rd.  A launch that does not
// return NTSCSIM_OK ends the call.
template <class Touch, class Launch>
int frames_in_order(int n, int cap, Touch &&touch, Launch &&launch)
{
    std::vector<Span> wr, rd;                                                   // what the run writes and reads
    int first = 0;
    for (int i = 0; i < n; i++) {
        const size_t r0 = rd.size();                                            // descriptor i's reads go behind the run's
        const Span w = touch(i, rd);
        const Span *const wr0 = wr.data(), *const wr1 = wr0 + wr.size();
        bool cut = i - first >= cap || hits_any(w, wr0, wr1) || hits_any(w, rd.data(), rd.data() + r0);
        for (size_t r = r0; !cut && r < rd.size(); r++) cut = hits_any(rd[r], wr0, wr1);
        if (cut && i > first) {
            const int rc = launch(first, i - first);
            if (rc != NTSCSIM_OK) return rc;
            first = i;
            wr.clear();
            rd.erase(rd.begin(), rd.begin() + (std::ptrdiff_t)r0);
        }
        wr.push_back(w);
    }
    return n > first ? launch(first, n - first) : NTSCSIM_OK;
}

// What a *_clip_device() call writes: add() every span, sort() once (NTSCSIM_E_ARG if two of them overlap), then
// hits(s): s overlaps one of them.
struct CallWrites {
    std::vector<Span> wr;

    static bool by_start(const Span &x, const Span &y) { return x.a < y.a; }
    void add(const Span &s) { wr.push_back(s); }
    int sort()
    {
        std::sort(wr.begin(), wr.end(), by_start);
        for (size_t i = 1; i < wr.size(); i++)
            if (wr[i].a < wr[i - 1].b) return NTSCSIM_E_ARG;
        return NTSCSIM_OK;
    }
    bool hits(const Span &s) const
    {
        const auto it = std::upper_bound(wr.begin(), wr.end(), s, by_start);
        return (it != wr.end() && overlaps(s, *it)) || (it != wr.begin() && overlaps(s, *(it - 1)));
    }
};

// `rows` rows of row_bytes bytes from one pitch to another; what lies between the rows of dst stays
inline void copy_rows(void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t row_bytes, int rows)
{
    for (int y = 0; y < rows; y++)
        std::memcpy(static_cast<uint8_t *>(dst) + (size_t)y * dst_pitch, static_cast<const uint8_t *>(src) + (size_t)y * src_pitch, row_bytes);
}

} // namespace ntscsim

// ntsc_px4.hpp -- how the kernels of the stages (csrc/ntsc_key.hip, csrc/ntsc_avg.hip, csrc/ntsc_led.hip,
// csrc/ntsc_filmac.hip, csrc/ntsc_pixmap.hip) reach their pixels: dwords
// and quads of BGRA pixels through the global address space.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ntscsim {

#define PX4_DEV __device__ __forceinline__

// device memory is reached through the global address space: a pointer that comes out of a record would otherwise be
// accessed with flat instructions, which count against the scalar-load counter too, so every record read would wait
// for the vector loads in flight
#define PX4_GLOBAL __attribute__((address_space(1)))
typedef uint32_t px4_u4 __attribute__((ext_vector_type(4)));
PX4_DEV uint32_t gld(const void *p) { return *(const PX4_GLOBAL uint32_t *)p; }
PX4_DEV px4_u4 gld4(const void *p) { return *(const PX4_GLOBAL px4_u4 *)p; }
// 16 bytes from an address that is only a multiple of 4
typedef px4_u4 px4_u4a __attribute__((aligned(4)));
PX4_DEV px4_u4 gld4a(const void *p) { return *(const PX4_GLOBAL px4_u4a *)p; }
PX4_DEV void gst(void *p, uint32_t v) { *(PX4_GLOBAL uint32_t *)p = v; }
PX4_DEV void gst4(void *p, px4_u4 v) { *(PX4_GLOBAL px4_u4 *)p = v; }

// a lane's quad: VEC one 16-byte access, otherwise the first npx pixels as dwords
template <bool VEC>
PX4_DEV void px4_load(uint32_t (&v)[4], const uint8_t *__restrict__ p, int npx)
{
    if (VEC) {
        const px4_u4 q = gld4(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < npx) v[k] = gld(p + 4 * k);
    }
}

template <bool VEC>
PX4_DEV void px4_store(uint8_t *__restrict__ p, const uint32_t (&v)[4], int npx)
{
    if (VEC) gst4(p, px4_u4{v[0], v[1], v[2], v[3]});
    else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < npx) gst(p + 4 * k, v[k]);
    }
}

} // namespace ntscsim

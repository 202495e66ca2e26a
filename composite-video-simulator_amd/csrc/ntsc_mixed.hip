// ntsc_mixed.hip -- the kernels of ntscsim_mixed_fields_device(): the generic chain of ntsc_kernels.hip over fields that
// name different parameter sets, ONE launch of each kernel however many sets a call holds (csrc/mixed_plan.hpp lays the
// call out).
//
// A call's fields are sorted into groups, one per set; a group owns a piece of the common scanline space that starts at
// a multiple of 64 rows, and its workgroups are counted within it.  A workgroup finds its group through a block table
// (block index of the launch -> group, block within the group), reads the group's record -- the DevParams and jump
// tables a single-set launch gets as kernel arguments -- and runs the SAME body as k_field_row_setup / k_encode /
// k_decode / k_bob on the group's slice of the records, with every row-indexed scratch pointer advanced by the group's
// first row.  The block index, hence the group and all of its record, is wave-uniform: the record arrives through
// scalar loads, and every switch branch and trip count of the bodies stays uniform as it is with kernel arguments.
// Rows between a group's last row and the next group's first belong to nobody: the bodies clamp against the group's
// own R (`rho < P.R`), as they do at the end of a single-set launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ntsc_device.hpp"

#pragma clang fp contract(off)

namespace ntscsim {

// one group of a mixed call (device memory, read-only for the kernels)
struct MixedGroup {
    DevParams P;          // the set's switches; nfields / R: the group's; W, H, Lslot, Rpad: the call's
    GeomDev G;            // jump tables of the set's draw layout, ptab of its phase-noise level
    int32_t base;         // first row of the group in the common scanline space (multiple of 64)
    int32_t field0;       // first record of the group
};
struct MixedBlock { int32_t group, block; };

// k_mixed_setup: blocks [0, 3 * nfields) are one (field, part) each -- head switch | phase-noise walk | dropout walk, as
// k_field_row_setup -- and the rest the row-start states, luma then chroma, over the encoder's block table.
__global__ __launch_bounds__(64) void k_mixed_setup(const MixedGroup *__restrict__ groups, const int32_t *__restrict__ group_of,
                                                    const MixedBlock *__restrict__ btab, const FieldDev *__restrict__ fields,
                                                    int *__restrict__ hs_shift, int *__restrict__ pn_noise,
                                                    int *__restrict__ dropout,
                                                    uint32_t *__restrict__ rs_luma, int *__restrict__ n0_luma,
                                                    uint32_t *__restrict__ rs_chroma,
                                                    int *__restrict__ n0_u, int *__restrict__ n0_v, int nfs, int nrs)
{
    __shared__ uint32_t ring[31 * 64];
    const int b = __builtin_amdgcn_readfirstlane((int)blockIdx.x);
    if (b < nfs) {
        const int f = b / 3;
        const MixedGroup &g = groups[group_of[f]];
        field_part_body(g.P, g.G, fields + g.field0, hs_shift + g.base, pn_noise + g.base, dropout + g.base, ring,
                        f - g.field0, b % 3);
        return;
    }
    const int q = b - nfs;
    const MixedBlock r = btab[q % nrs];
    const MixedGroup &g = groups[r.group];
    row_states_body(g.P, g.G, fields + g.field0, rs_luma + g.base, n0_luma + g.base, rs_chroma + g.base, n0_u + g.base,
                    n0_v + g.base, ring, r.block, q / nrs);
}

template <class RT>
__global__ __launch_bounds__(64) void k_mixed_encode(const MixedGroup *__restrict__ groups, const MixedBlock *__restrict__ btab,
                                                     const FieldDev *__restrict__ fields,
                                                     const uint32_t *__restrict__ rs_luma,
                                                     const int *__restrict__ n0_luma, int *__restrict__ comp)
{
    __shared__ uint32_t ring[31 * 64];
    const MixedBlock r = btab[__builtin_amdgcn_readfirstlane((int)blockIdx.x)];
    const MixedGroup &g = groups[r.group];
    const DevParams P = g.P;      // read once, here: a load left inside the row loop would wait with the LDS traffic
    encode_body<Opt<F_GENERIC>, RT>(P, r.block, fields + g.field0, rs_luma + g.base, n0_luma + g.base, comp + g.base, ring);
}

// One launch per decoder class present in the call, over the blocks of that class's groups (`btab` is the class's).
template <bool VHS, bool COMPOUT, class RT>
__global__ __launch_bounds__(64, (VHS && COMPOUT) ? NTSC_DEC_WAVES_VHS : NTSC_DEC_WAVES) void k_mixed_decode(
    const MixedGroup *__restrict__ groups, const MixedBlock *__restrict__ btab, const FieldDev *__restrict__ fields,
    const int *__restrict__ comp, const uint32_t *__restrict__ rs_chroma, const int *__restrict__ n0_u,
    const int *__restrict__ n0_v, const int *__restrict__ hs_shift, const int *__restrict__ pn_noise,
    const int *__restrict__ dropout, int *__restrict__ tails)
{
    __shared__ uint32_t ring[31 * 64];
#ifdef NTSC_DIRECT_STORE
    uint32_t *ostage = nullptr;
#else
    __shared__ __attribute__((aligned(16))) uint32_t ostage[64 * 20];
#endif
    const MixedBlock r = btab[__builtin_amdgcn_readfirstlane((int)blockIdx.x)];
    const MixedGroup &g = groups[r.group];
    const DevParams P = g.P;      // (as k_mixed_encode)
    const GeomDev G = g.G;
    decode_body<VHS, COMPOUT, Opt<F_GENERIC>, RT>(P, G, r.block, fields + g.field0, comp + g.base, rs_chroma + g.base,
                                                 n0_u + g.base, n0_v + g.base, hs_shift + g.base, pn_noise + g.base,
                                                 dropout + g.base, tails, blockIdx.x, gridDim.x, ring, ostage);
}

// bob reads W, H and the destinations' alignment only, which are the call's: any group's record holds them.
__global__ void k_mixed_bob(const MixedGroup *__restrict__ groups, const FieldDev *__restrict__ fields)
{
    bob_body(groups[0].P, fields, (int)blockIdx.y, (int)blockIdx.x);
}

} // namespace ntscsim

// ntsc422_mixed.hip -- the kernels of ntscsim_mixed_fields422_device(): the twelve-sweep chain of ntsc422_kernels.hip over
// fields that name different parameter sets, ONE launch of each kernel however many sets a call holds (csrc/mixed_plan.hpp
// lays the call out as it does for the BGRA tool, ntsc_mixed.hip; DESIGN.md 7, "settings per field").
//
// A group -- the fields of one set -- owns a piece of the common scanline space that starts at a multiple of 64 rows.  Its
// workgroups of 63 rows (+ the halo lane) are counted WITHIN it, so three things that a single-set launch reads off
// blockIdx.x come apart here:
//   - the rows of a workgroup, gidx = block * 63 + lane - 1, count from the block WITHIN THE GROUP;
//   - "has a row above" (halo_redirect) is a property of the block within the group: a group's first block has none, as
//     block 0 of a single-set launch has none -- the row above it in the scanline space belongs to another set or nobody;
//   - the scratch slot block * 64 + lane and the place of the halo copy are the LAUNCH's: two groups must not share them.
// Setup is k_mixed_setup (ntsc_mixed.hip) as it stands: its bodies branch on P.variant, and its row-state blocks of 64
// rows come from the plan's encoder table.
//
// Included by ntscsim_hip.hip after ntsc_mixed.hip and ntsc422_kernels.hip.
#pragma clang fp contract(off)

namespace ntscsim {

// one group of a mixed YUV422P call (device memory, read-only for the kernels)
struct Mixed422Group {
    DevParams P;          // the set's switches as prepare422() derives them (variant 1); nfields / R: the group's; W, H, Lslot,
                          // Rpad and the alignment flags: the call's
    GeomDev G;            // jump tables of the set's draw layout, ptab of its phase-noise level
    double a_hp_i, a_hp_q, a_sh_c, sharpen_c;     // what k422_process takes as scalar arguments
    int32_t yc_recombine, after_yc_sep;
    int32_t bkey_level;   // black_key_level_feedback (k422_bkey's argument)
    int32_t base;         // first row of the group in the common scanline space (multiple of 64)
    int32_t field0;       // first record of the group
    int32_t _pad;
};

// z = record in sorted order
__global__ void k422_mixed_render(const Mixed422Group *__restrict__ groups, const int32_t *__restrict__ group_of,
                                  const Field422Dev *__restrict__ fields)
{
    const int f = blockIdx.z;
    render422_body(groups[group_of[f]].P, fields[f]);
}

// (records whose set has no black-key feedback carry no flt pointers: the host leaves them out, as prepare422() does)
__global__ void k422_mixed_bkey(const Mixed422Group *__restrict__ groups, const int32_t *__restrict__ group_of,
                                const Field422Dev *__restrict__ fields)
{
    const int f = blockIdx.z;
    const Mixed422Group &g = groups[group_of[f]];
    bkey422_body(g.P, fields[f], g.bkey_level);
}

// One block per process block of the launch.  Block b of a group (b >= 1) copies the input of the group's row b * 63 - 1
// -- field and row taken within the group -- to the slot of its LAUNCH-wide block; a group's first block has no row above.
__global__ __launch_bounds__(256) void k422_mixed_halo(const Mixed422Group *__restrict__ groups,
                                                       const MixedBlock *__restrict__ btab,
                                                       const Field422Dev *__restrict__ fields, Scratch422 Sc)
{
    const MixedBlock r = btab[__builtin_amdgcn_readfirstlane((int)blockIdx.x)];
    if (r.block == 0) return;
    const Mixed422Group &g = groups[r.group];
    halo422_body(g.P, fields + g.field0, Sc, r.block, blockIdx.x);
}

__global__ __launch_bounds__(64) void k422_mixed_process(const Mixed422Group *__restrict__ groups,
                                                         const MixedBlock *__restrict__ btab,
                                                         const Field422Dev *__restrict__ fields, Scratch422 Sc,
                                                         const uint32_t *__restrict__ rs_luma,
                                                         const int *__restrict__ n0_luma,
                                                         const uint32_t *__restrict__ rs_chroma,
                                                         const int *__restrict__ n0_u, const int *__restrict__ n0_v,
                                                         const int *__restrict__ hs_shift,
                                                         const int *__restrict__ pn_noise,
                                                         const int *__restrict__ dropout)
{
    __shared__ uint32_t ring[31 * 64];
    const MixedBlock r = btab[__builtin_amdgcn_readfirstlane((int)blockIdx.x)];
    const Mixed422Group &g = groups[r.group];
    // read once, here (as k_mixed_encode): no load of a switch may sit inside the sweeps
    const DevParams P = g.P;
    const GeomDev G = g.G;
    const double a_hp_i = g.a_hp_i, a_hp_q = g.a_hp_q, a_sh_c = g.a_sh_c, sharpen_c = g.sharpen_c;
    const int yc_recombine = g.yc_recombine, after_yc_sep = g.after_yc_sep;
    const int base = g.base, field0 = g.field0;
    process422_body(P, G, fields + field0, Sc, rs_luma + base, n0_luma + base, rs_chroma + base, n0_u + base, n0_v + base,
                    hs_shift + base, pn_noise + base, dropout + base, a_hp_i, a_hp_q, a_sh_c, sharpen_c, yc_recombine,
                    after_yc_sep, ring, (unsigned)r.block, blockIdx.x);
}

} // namespace ntscsim

// ntsc_mixed_fast.hip -- the hand-tuned kernels (ntsc_encode_fast.hip, ntsc_decode_fast.hip) behind
// ntscsim_mixed_fields_device(), for the groups whose parameter set is of the default / -vhs preset families
// (ntscsim_set_mixed_forms(NTSCSIM_MIXED_TUNED); csrc/mixed_forms.hpp picks each group's form).
//
// As in ntsc_mixed.hip a workgroup finds its group through the block table of ITS kernel form, copies the group's record
// into locals once -- the block index is wave-uniform, so the record arrives by scalar loads and every branch of the body
// stays uniform as it is with kernel arguments -- and runs the SAME body as the single-set kernel of that form, with the
// block within the group and the group's first row where the single-set kernel passes blockIdx.x and 0.
// Every row-indexed scratch pointer is advanced by the group's first row, EXCEPT the composite plane: both bodies address
// it through a buffer descriptor over the whole plane (num_records = W * Rpad * 4) and the decoder needs that bounds
// check to read 0 outside a row, so there the first row goes into the lane's byte offset (see the bodies).
// Launch bounds are those of the single-set kernels.
#pragma clang fp contract(off)

namespace ntscsim {

template <class RT, bool PRE = false>
__global__ __launch_bounds__(64) void k_mixed_encode_fast(const MixedGroup *__restrict__ groups, const MixedBlock *__restrict__ btab,
                                                          const FieldDev *__restrict__ fields,
                                                          const uint32_t *__restrict__ rs_luma,
                                                          const int *__restrict__ n0_luma, int *__restrict__ comp)
{
    const MixedBlock r = btab[__builtin_amdgcn_readfirstlane((int)blockIdx.x)];
    const MixedGroup &g = groups[r.group];
    const DevParams P = g.P;      // (as k_mixed_encode)
    encode_fast_body<RT, PRE>(P, (unsigned)r.block, g.base, fields + g.field0, rs_luma + g.base, n0_luma + g.base, comp);
}

#define NTSC_MIXED_FAST_DECODE_ARGS                                                                                          \
    const MixedGroup *__restrict__ groups, const MixedBlock *__restrict__ btab, const FieldDev *__restrict__ fields,        \
    const int *__restrict__ comp, const uint32_t *__restrict__ rs_chroma, const int *__restrict__ n0_u,                      \
    const int *__restrict__ n0_v, const int *__restrict__ hs_shift, const int *__restrict__ pn_noise,                        \
    const int *__restrict__ dropout, int *__restrict__ tails
// (the dynamic LDS of the luma delay ring is the launch's: LUMA_RING_BYTES if any group of the launch runs it; the body
//  tests rowend::luma_ring with the group's own tape speed)
#define NTSC_MIXED_FAST_DECODE_BODY(...)                                                                                     \
    const MixedBlock r = btab[__builtin_amdgcn_readfirstlane((int)blockIdx.x)];                                              \
    const MixedGroup &g = groups[r.group];                                                                                   \
    const DevParams P = g.P;                                                                                                 \
    const GeomDev G = g.G;                                                                                                   \
    decode_fast_body<__VA_ARGS__>(P, G, (unsigned)r.block, g.base, fields + g.field0, comp, rs_chroma + g.base,              \
                                  n0_u + g.base, n0_v + g.base, hs_shift + g.base, pn_noise + g.base, dropout + g.base, tails)

template <bool VHS, class RT, bool WR = false>
__global__ __launch_bounds__(64, VHS ? FastWaves<RT>::n : 4) void k_mixed_decode_fast(NTSC_MIXED_FAST_DECODE_ARGS)
{
    NTSC_MIXED_FAST_DECODE_BODY(VHS, RT, WR, false);
}

template <bool VHS, class RT>
__global__ __launch_bounds__(64, VHS ? FastWaves<RT>::n : 4) void k_mixed_decode_fast_bk(NTSC_MIXED_FAST_DECODE_ARGS)
{
    NTSC_MIXED_FAST_DECODE_BODY(VHS, RT, VHS, true);
}

template <class RT>
__global__ __launch_bounds__(64, FastWaves<RT>::n) void k_mixed_decode_fast_sv(NTSC_MIXED_FAST_DECODE_ARGS)
{
    NTSC_MIXED_FAST_DECODE_BODY(true, RT, true, false, true);
}

#undef NTSC_MIXED_FAST_DECODE_BODY
#undef NTSC_MIXED_FAST_DECODE_ARGS

} // namespace ntscsim

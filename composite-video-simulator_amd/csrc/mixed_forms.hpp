// mixed_forms.hpp -- which kernel form every group of an ntscsim_mixed_fields_device() call runs when the call may use the
// hand-tuned kernels (ntscsim_set_mixed_forms(NTSCSIM_MIXED_TUNED)), and the block tables of those forms.  No HIP in it:
// plain code over PODs and std::vector, so tests/mixed_forms_check.cpp sweeps it with g++ (plain and with the sanitizers).
//
//   1. the rule   form_of(): the facts of one parameter set plus the facts of the call -> an encoder form and a decoder
//                 form, chosen independently.  A set takes the hand-tuned form that the single-set launcher
//                 (launch_records(), ntscsim_hip.hip) picks for it on a throughput-form context, under that form's
//                 preconditions taken for the CALL: the alignment of all descriptors and the call-wide Rpad.  Everything
//                 else -- odd scanline phases, the full output low-pass, nocolor, amp != 50, no luma noise, no input
//                 low-pass, partly switched-off chroma noise ... -- keeps the generic mixed kernel of its decoder class.
//   2. the tables make_form_tables(): one block table per encoder form and one per decoder form from the plan's groups,
//                 blocks counted within a group exactly as in mixed::Plan::enc_tab / dec_tab.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mixed_plan.hpp"

namespace ntscsim {
namespace mixed {

// encoder forms, in launch order
enum { ENC_GENERIC = 0,        // k_mixed_encode<RT>
       ENC_FAST = 1,           // k_mixed_encode_fast<RT>              (k_encode_fast)
       ENC_FAST_PRE = 2,       // k_mixed_encode_fast<RT,true>         (k_encode_fast_pre)
       N_ENC = 3 };
// decoder forms, in launch order.  The generic form of a decoder class has the class's own number (CLS_*).
enum { DEC_GENERIC_TV = CLS_TV, DEC_GENERIC_VCR_COMP = CLS_VCR_COMP, DEC_GENERIC_VCR_SVIDEO = CLS_VCR_SVIDEO,   // k_mixed_decode<..>
       DEC_FAST_TV = 3,        // k_mixed_decode_fast<false,RT>        (k_decode_fast<false>)
       DEC_FAST_VHS = 4,       // k_mixed_decode_fast<true,RT>         (k_decode_fast<true>)
       DEC_FAST_VHS_WR = 5,    // k_mixed_decode_fast<true,RT,true>    (wrap-around head switch)
       DEC_FAST_SV = 6,        // k_mixed_decode_fast_sv<RT>
       DEC_FAST_BK_TV = 7,     // k_mixed_decode_fast_bk<false,RT>
       DEC_FAST_BK_VHS = 8,    // k_mixed_decode_fast_bk<true,RT>
       N_DEC = 9 };

// The hand-tuned kernels address the transposed composite plane through a raw buffer descriptor with a 32-bit byte
// offset: offset = row*4 + (x + head-switch displacement) * Rpad*4, compared (unsigned) with num_records = W * Rpad*4, and
// out-of-range reads return the reference's fill value 0.  That only works while the displaced offset cannot wrap around
// 2^32 back INTO the plane: the displacement lies in [-W/10, +W/10] (hs_mode 1), so both x + shift >= W and x + shift < 0
// stay outside iff (W + W/10 + 1) * Rpad*4 fits in 32 bits.  When the displacement can wrap around the tw = 1.1 W window
// (hs_mode 2, |shift| up to tw/2: the WR forms) the offset is first formed for x + shift, which reaches from -tw/2 to
// W - 1 + tw/2, and then moved by -+ tw samples: (W + tw + 1) * Rpad*4 is required to fit, a margin that covers every
// intermediate value.  Larger planes take the generic kernels (64-bit addressing).  hs_mode 0: no head switching.
inline bool fast_plane_ok(size_t Rpad, int W, int hs_mode)
{
    const size_t tw = (size_t)W + (size_t)W / 10u;
    const size_t span = (size_t)W + (hs_mode == 0 ? 0u : (hs_mode == 1 ? (size_t)W / 10u + 1u : tw + 1u));
    return span * Rpad * 4u < 0xFFF00000ull;
}

// what the rule needs to know of one parameter set (the switches as the kernels' DevParams holds them)
struct SetFacts {
    bool in_lp;           // input chroma low-pass on
    bool pre_on;          // composite pre-emphasis on
    bool noise;           // video_noise != 0
    bool cnoise, pnoise;  // video_chroma_noise != 0, video_chroma_phase_noise != 0
    bool nocolor;
    bool even_phase;      // scanline phases 0 / 2 only
    bool vhs, svideo;
    bool hs;              // head switching on
    bool hs_small;        // ... and every displacement within W/10 samples (true without head switching)
    int amp, amp_back;    // subcarrier_amplitude, subcarrier_amplitude_back
    int out_lp;           // 0 off, 1 lite, 2 full
};

// ... and of the call
struct CallFacts {
    size_t Rpad;          // rows of the composite plane of the WHOLE call (mixed::Plan::Rpad)
    int W;
    bool src_al16, dst_al16;      // over all descriptors
    bool force_generic;           // ntscsim_debug_force_generic
    bool no_fast;                 // ntscsim_debug_no_fast_decode, bit 0
};

struct Forms { int enc, dec; };

inline int generic_dec_form(const SetFacts &s)
{
    return !s.vhs ? DEC_GENERIC_TV : (s.svideo ? DEC_GENERIC_VCR_SVIDEO : DEC_GENERIC_VCR_COMP);
}

inline Forms form_of(const SetFacts &s, const CallFacts &c)
{
    Forms f;
    f.enc = ENC_GENERIC;
    f.dec = generic_dec_form(s);
    if (c.force_generic || c.no_fast || !s.even_phase) return f;
    const int hs_mode = !s.hs ? 0 : (s.hs_small ? 1 : 2);
    const bool small_plane = fast_plane_ok(c.Rpad, c.W, hs_mode);
    const bool any_plane = fast_plane_ok(c.Rpad, c.W, s.hs ? 2 : 0);       // the forms with wrap-around loads
    // ---- encoder: the default / -vhs presets' input stage, with or without pre-emphasis
    if (s.in_lp && s.noise && s.amp == 50 && small_plane && c.src_al16) f.enc = s.pre_on ? ENC_FAST_PRE : ENC_FAST;
    // ---- decoder
    const bool back50 = s.amp_back == 50;
    const bool dec_fast = !s.nocolor && s.out_lp == 1 && s.amp == 50 && (back50 || s.amp_back >= 2) && c.dst_al16 && small_plane;
    if (!dec_fast) return f;
    const bool cn_all = s.cnoise && s.pnoise, cn_none = !s.cnoise && !s.pnoise;
    if (s.vhs && cn_all) {
        if (s.svideo) { if (back50 && any_plane) f.dec = DEC_FAST_SV; }
        else if (back50) f.dec = s.hs_small ? DEC_FAST_VHS : DEC_FAST_VHS_WR;
        else if (any_plane) f.dec = DEC_FAST_BK_VHS;
    } else if (!s.vhs && cn_none && s.hs_small) {
        f.dec = back50 ? DEC_FAST_TV : DEC_FAST_BK_TV;
    }
    return f;
}

struct FormTables {
    std::vector<BlockRef> enc[N_ENC];
    std::vector<BlockRef> dec[N_DEC];
    size_t dec_max = 0;           // blocks of the largest decoder table (the `tails` scratch is sized for it)
};

// enc_form_of_group[g] / dec_form_of_group[g]: the forms of plan.groups[g].  Returns false (tables empty) on a form out of
// range or a decoder form of another class than the group's.
inline bool make_form_tables(const Plan &plan, const int *enc_form_of_group, const int *dec_form_of_group, FormTables &out)
{
    out = FormTables();
    const size_t ng = plan.groups.size();
    if (ng && (!enc_form_of_group || !dec_form_of_group)) return false;
    size_t n_enc[N_ENC] = {0}, n_dec[N_DEC] = {0};
    for (size_t g = 0; g < ng; g++) {
        const Group &G = plan.groups[g];
        const int e = enc_form_of_group[g], d = dec_form_of_group[g];
        if (e < 0 || e >= N_ENC || d < 0 || d >= N_DEC) return false;
        if (d < N_CLS && d != G.cls) return false;
        n_enc[e] += (size_t)G.enc_blocks;
        n_dec[d] += (size_t)G.dec_blocks;
    }
    for (int e = 0; e < N_ENC; e++) out.enc[e].reserve(n_enc[e]);
    for (int d = 0; d < N_DEC; d++) out.dec[d].reserve(n_dec[d]);
    for (size_t g = 0; g < ng; g++) {
        const Group &G = plan.groups[g];
        std::vector<BlockRef> &et = out.enc[enc_form_of_group[g]], &dt = out.dec[dec_form_of_group[g]];
        for (int32_t b = 0; b < G.enc_blocks; b++) et.push_back(BlockRef{(int32_t)g, b});
        for (int32_t b = 0; b < G.dec_blocks; b++) dt.push_back(BlockRef{(int32_t)g, b});
    }
    for (int d = 0; d < N_DEC; d++) if (out.dec[d].size() > out.dec_max) out.dec_max = out.dec[d].size();
    return true;
}

} // namespace mixed
} // namespace ntscsim

"""The table of NTSCSIM_MODE_FAST32 kernel forms: every `RT = float` twin that launch_records() (csrc/ntscsim_hip.hip) can
pick -- hand-tuned, two-launch, template, generic and role kernels -- with a switch set and a geometry that reaches it and
the names ntscsim_debug_last_kernels() must report.  Shared by tests/test_fast32_forms_host.py (CPU: the model on every
row, the closure of the table over the launcher's names) and tests/test_fast32_forms_gpu.py (equality with the model, form
by form).  Test infrastructure only; no GPU import.

A batch row: (id, flags, ghost, w, h, n, kind, mode, names, il, tff, plane)
  ghost   tap list ((delay, gain), ...) of the ghosting extension, () for none
  kind    source kind of tests/_modes.py: sources()
  mode    how the form is reached:
            "hand-tuned"  the dispatcher's own choice
            "two-launch"  ntscsim_debug_no_fast_decode(2): VCR half and TV half as two launches
            "template"    ntscsim_debug_no_fast_decode(1): the template forms of the generic kernels
            "generic"     ntscsim_debug_force_generic(1): options read at run time
            "fold-off"    ntscsim_debug_no_fast_decode(8): ghosting as a pass of its own whatever the delays
  names   what last_kernels() must hold among its k_encode*, k_ghost, k_vcr*, k_decode* entries, in order
  plane   whether the int32 composite plane the product exposes (ntscsim_debug_read_composite: the plane the ENCODER
          wrote) is the model's composite_y tap.  The tap sits behind pre-emphasis and luma noise and in FRONT of the
          ghosting extension (oracle/ntsc_modes_body.h; tests/test_fast32_forms_host.py checks both on the host), so:
          pre-emphasis rows compare it; rows whose ghosting runs as k_ghost compare it (that pass writes a second plane,
          the exposed one stays raw); rows whose ghosting is folded into the encoder (k_encode_fast_gh) expose the GHOSTED
          plane, another point of the chain -- those compare bytes only.
"""
from collections import namedtuple

import cases

Row = namedtuple("Row", "id flags ghost w h n kind mode names il tff plane")
Role = namedtuple("Role", "id flags w h name")

HT, TWO, TPL, GEN, NOFOLD = "hand-tuned", "two-launch", "template", "generic", "fold-off"
DEBUG_BITS = {HT: 0, TWO: 2, TPL: 1, GEN: 0, NOFOLD: 8}       # ntscsim_debug_no_fast_decode; GEN: ntscsim_debug_force_generic

# ------------------------------------------------------------------------------------------------ the names
ENC, ENC_XI, ENC_PRE = "k_encode_fast<float>", "k_encode_fast_xi<float>", "k_encode_fast_pre<float>"
GH2, GH4, GHOST = "k_encode_fast_gh<float,2>", "k_encode_fast_gh<float,4>", "k_ghost"
ENC_T, ENC_G = "k_encode<8u,float>", "k_encode<1u,float>"               # F_LNOISE: the presets' template form; F_GENERIC
VCR = "k_vcr_front<float>"
DEC_TV, DEC_VHS, DEC_WR = "k_decode_fast<false,float>", "k_decode_fast<true,float>", "k_decode_fast<true,float,true>"
DEC_XI, DEC_FO, DEC_SV = "k_decode_fast_xi<float>", "k_decode_fast_fo<float>", "k_decode_fast_sv<float>"
BK_VHS, BK_TV = "k_decode_fast_bk<true,float>", "k_decode_fast_bk<false,float>"
T_VHS, T_TV, T_SV = "k_decode<true,true,6u,float>", "k_decode<false,false,0u,float>", "k_decode<true,false,1u,float>"
G_VHS, G_TV, G_SV = "k_decode<true,true,1u,float>", "k_decode<false,false,1u,float>", T_SV

# The names the launcher does not hold as one string literal: it assembles them from macro arguments (NTSC_LAUNCH_ENCODE,
# NTSC_LAUNCH_DECODE, NTSC_LAUNCH_FAST, NTSC_LAUNCH_FAST_BK, NTSC_LAUNCH_FAST_WR) or from pieces (k_encode_fast_gh).  The
# closure test derives the same set from the macro invocations in csrc/ntscsim_hip.hip and compares.
MACRO_NAMES = sorted({ENC_T, ENC_G, T_VHS, T_TV, T_SV, G_VHS, G_TV, DEC_TV, DEC_VHS, DEC_WR, BK_VHS, BK_TV, GH2, GH4})

ROLE_NAMES = ["k_field_pipe<float>", "k_field_pipe<float,true>", "k_field_pipe_sv<float>", "k_field_pipe_xi<float>",
              "k_field_pipe_catv<float>", "k_field_pipe_tv<float>", "k_field_pipe_tv_catv<float>"]

# ------------------------------------------------------------------------------------------------ switch sets
VHS = ["-vhs"]
LP = ["-vhs", "-vhs-speed", "lp"]
EP = ["-vhs", "-vhs-speed", "ep"]
PAL = ["-tvstd", "pal", "-vhs"]
SV = ["-vhs-svideo", "1"]
FO = ["-out-composite-lowpass-lite", "0"]
DROP = ["-chroma-dropout", "30000"]
SAT = ["-noise", "100"]
NOPN = ["-chroma-phase-noise", "0"]
# head switch inside a 96x32 frame, displaced beyond W/10 forwards (0.0012) and backwards (0.002): tests/cases.py hs_pos, hs_neg
HS_POS = ["-vhs-head-switching-point", "0.105", "-vhs-head-switching-phase", "0.0012"]
HS_NEG = ["-vhs-head-switching-point", "0.105", "-vhs-head-switching-phase", "0.002"]

# tests/test_gpu_parity.py: _GHOST_FUSED (the host test compares the two lists)
GHOST_FUSED = [((12, 64),), ((12, 64), (31, -32)), ((1, 256), (63, -256)), ((7, 64), (19, -32), (40, 12)),
               ((1, -256), (2, 256), (62, 100), (63, -7)), ((5, 90), (5, 90), (33, -120), (33, 17))]

# both sides of every steady loop (tests/test_fast32_model_gpu.py: SIZES), H = 10; 18/17-row fields with a partial last chunk
WIDTHS = (16, 28, 36, 40, 44, 68)
SMALL = [(w, 10, 4) for w in WIDTHS] + [(100, 35, 4)]
# 45 chunks per row, four 63-row workgroups per field
FULL = (720, 486, 2)


def _rows():
    out = []

    def add(name, flags, w, h, n, mode, names, kind="mixed", ghost=(), il=0, tff=0, plane=True):
        out.append(Row(name, list(flags), tuple(ghost), w, h, n, kind, mode, list(names), il, tff, plane))

    def family(tag, flags, mode, names, full=True, ghost=(), plane=True):
        """the widths, 100x35, one saturating row that hits both clamps, one decaying row and (per decoder family) 720x486"""
        for w, h, n in SMALL:
            add("%s_%dx%d" % (tag, w, h), flags, w, h, n, mode, names, ghost=ghost, plane=plane)
        add("%s_sat_68x10" % tag, flags + SAT, 68, 10, 2, mode, names, "saturating", ghost=ghost, plane=plane)
        add("%s_decay_720x16" % tag, flags, 720, 16, 2, mode, names, "decay", ghost=ghost, plane=plane)
        if full:
            add("%s_720x486" % tag, flags, FULL[0], FULL[1], FULL[2], mode, names, ghost=ghost, plane=plane)

    # ---- hand-tuned: the two presets
    family("def", [], HT, [ENC, DEC_TV])
    family("sp", VHS, HT, [ENC, DEC_VHS])
    family("lp", LP, HT, [ENC, DEC_VHS], full=False)
    family("ep", EP, HT, [ENC, DEC_VHS], full=False)
    # ---- the wrap-around head switch: displacements beyond W/10.  The geometry of the EXACT test
    # (test_every_decoder_path_agrees_with_the_oracle), for which the displacement is derived; PAL's default phase
    # (0.18 of the 1.1 W window) is beyond W/10 at every width, so the family's 720x486 launch is PAL's
    add("wr_pal_96x36", PAL, 96, 36, 4, HT, [ENC, DEC_WR])
    add("wr_pos_96x32", VHS + HS_POS, 96, 32, 4, HT, [ENC, DEC_WR])
    add("wr_neg_96x32", VHS + HS_NEG, 96, 32, 4, HT, [ENC, DEC_WR])
    add("wr_pal_sat_96x36", PAL + SAT, 96, 36, 2, HT, [ENC, DEC_WR], "saturating")
    add("wr_pal_decay_720x16", PAL, 720, 16, 2, HT, [ENC, DEC_WR], "decay")
    add("wr_pal_720x486", PAL, 720, 486, 2, HT, [ENC, DEC_WR])
    # ---- scanline phases of either parity
    family("xi_p90", VHS + ["-comp-phase", "90"], HT, [ENC_XI, DEC_XI])
    add("xi_p270_off3_100x35", VHS + ["-comp-phase", "270", "-comp-phase-offset", "3"], 100, 35, 4, HT, [ENC_XI, DEC_XI])
    add("xi_off1_96x32", VHS + ["-comp-phase-offset", "1"], 96, 32, 4, HT, [ENC_XI, DEC_XI])
    add("xi_pal_p90_drop_96x36", PAL + ["-comp-phase", "90"] + DROP, 96, 36, 4, HT, [ENC_XI, DEC_XI])
    # ---- the full output chroma low-pass
    family("fo_sp", VHS + FO, HT, [ENC, DEC_FO])
    family("fo_lp", LP + FO, HT, [ENC, DEC_FO], full=False)
    family("fo_ep_drop", EP + FO + DROP, HT, [ENC, DEC_FO], full=False)
    add("fo_pal_96x36", PAL + FO, 96, 36, 4, HT, [ENC, DEC_FO])
    # ---- the pre-emphasis presets: subcarrier_amplitude_back other than 50.  Without the VCR the hand-tuned decoder takes
    # them with chroma phase noise off only (the presets switch it on: their own decoder is then the generic one)
    family("bk_vhs_catv", VHS + ["-comp-catv"], HT, [ENC_PRE, BK_VHS])
    family("bk_tv_catv", ["-comp-catv"] + NOPN, HT, [ENC_PRE, BK_TV])
    for k in ("2", "3", "4"):
        add("bk_vhs_catv%s_96x32" % k, VHS + ["-comp-catv" + k], 96, 32, 4, HT, [ENC_PRE, BK_VHS])
        add("bk_tv_catv%s_96x32" % k, ["-comp-catv" + k] + NOPN, 96, 32, 4, HT, [ENC_PRE, BK_TV])
    add("bk_vhs_catv3_hs_neg_96x32", VHS + ["-comp-catv3"] + HS_NEG, 96, 32, 4, HT, [ENC_PRE, BK_VHS])
    add("pre_tv_catv_pnoise_96x32", ["-comp-catv"], 96, 32, 4, HT, [ENC_PRE, G_TV])
    family("bk_vhs_catv3", VHS + ["-comp-catv3"], HT, [ENC_PRE, BK_VHS], full=False)
    # (the 256x100 of tests/test_fast32_model_gpu.py for the three switch sets whose names that file does not assert)
    add("bk_vhs_catv3_256x100", VHS + ["-comp-catv3"], 256, 100, 2, HT, [ENC_PRE, BK_VHS])
    add("xi_p90_256x100", VHS + ["-comp-phase", "90"], 256, 100, 2, HT, [ENC_XI, DEC_XI])
    add("sv_sp_256x100", VHS + SV, 256, 100, 2, HT, [ENC, DEC_SV])
    # ---- S-Video out of the VCR
    family("sv_sp", VHS + SV, HT, [ENC, DEC_SV])
    family("sv_lp", LP + SV, HT, [ENC, DEC_SV], full=False)
    family("sv_ep", EP + SV, HT, [ENC, DEC_SV], full=False)
    add("sv_pal_96x36", PAL + SV, 96, 36, 4, HT, [ENC, DEC_SV])
    # ---- the two-launch form
    family("two_sp", VHS, TWO, [ENC, VCR, DEC_TV])
    family("two_ep", EP, TWO, [ENC, VCR, DEC_TV], full=False)
    # ---- ghosting folded into the encoder (the exposed plane is the ghosted one: bytes only) ...
    family("gh2_sp", VHS, HT, [GH2, DEC_VHS], ghost=GHOST_FUSED[1], plane=False)
    family("gh4_def", [], HT, [GH4, DEC_TV], ghost=GHOST_FUSED[3], plane=False)
    for i, taps in enumerate(GHOST_FUSED):
        gh = GH2 if len(taps) <= 2 else GH4
        add("gh_taps%d_def_112x40" % i, [], 112, 40, 4, HT, [gh, DEC_TV], ghost=taps, plane=False)
        add("gh_taps%d_sp_112x40" % i, VHS, 112, 40, 4, HT, [gh, DEC_VHS], ghost=taps, plane=False)
    # ---- ... and as a pass of its own: a delay of 64, and the fold switched off
    family("ghost_d64_sp", VHS, HT, [ENC, GHOST, DEC_VHS], full=False, ghost=((12, 64), (64, -32)))
    add("ghost_d64_def_96x32", [], 96, 32, 4, HT, [ENC, GHOST, DEC_TV], ghost=((12, 64), (64, -32)))
    family("ghost_nofold_sp", VHS, NOFOLD, [ENC, GHOST, DEC_VHS], full=False, ghost=GHOST_FUSED[4])
    add("ghost_nofold_def_112x40", [], 112, 40, 4, NOFOLD, [ENC, GHOST, DEC_TV], ghost=GHOST_FUSED[1])
    # ---- the template forms of the generic kernels
    family("tpl_sp", VHS, TPL, [ENC_T, T_VHS])
    family("tpl_ep", EP, TPL, [ENC_T, T_VHS], full=False)
    family("tpl_def", [], TPL, [ENC_T, T_TV])
    family("tpl_sv", VHS + SV, TPL, [ENC_T, T_SV])
    # ---- the generic forms: `vhs`, `default` and `vhs_svideo` forced ...
    family("gen_sp", VHS, GEN, [ENC_G, G_VHS])
    family("gen_def", [], GEN, [ENC_G, G_TV])
    family("gen_sv", VHS + SV, GEN, [ENC_G, G_SV])
    # ... and the rows of tests/cases.py outside the presets' switch sets, with their own geometry and descriptor flags:
    # forced generic (the pair), and as the dispatcher itself runs them -- the hand-tuned kernel of whichever HALF of the
    # chain still matches a preset, the generic kernel for the other
    own = {
        "noise0": [ENC_G, DEC_TV],                    # encoder: luma noise off; decoder: the default preset's
        "chroma_noise_only": [ENC_G, G_TV],
        "phase_noise20": [ENC, G_TV],
        "nocolor": [ENC, G_TV],                       # (the switch acts in the decoder only)
        "nocolor_vhs": [ENC, G_VHS],
        "amp30": [ENC_G, G_VHS],
        "amp1": [ENC_G, G_VHS],
        "no_outlp": [ENC, G_TV],
        "no_inlp": [ENC_G, DEC_TV],
        "vhs_lp_only": [ENC, DEC_VHS],                # -vhs-speed alone: the VCR without head switching, all else preset
        "hs_nonoise": [ENC, DEC_WR],                  # hs_neg without the jitter: still beyond W/10
        "interlaced_tff": [ENC, DEC_VHS],
        "interlaced_bff": [ENC, DEC_TV],
    }
    by_name = {c[0]: c for c in cases.CASES}
    for name, names in own.items():
        _, flags, w, h, n, _, il, tff = by_name[name]
        dec = G_TV if names[1] in (DEC_TV, G_TV) else G_VHS
        add("gen_%s" % name, flags, w, h, n, GEN, [ENC_G, dec], "noise", il=il, tff=tff)
        add("own_%s" % name, flags, w, h, n, HT, names, "noise", il=il, tff=tff)
    return out


ROWS = _rows()
assert len({r.id for r in ROWS}) == len(ROWS)
BY_ID = {r.id: r for r in ROWS}


def params(flags, ghost=()):
    """ntscsim_params of a row: the switches, then the taps of the ghosting extension (no switch sets them)"""
    import _libs as L
    p = L.make_params(flags)
    p.ghost_taps = len(ghost)
    for k, (d, g) in enumerate(ghost):
        p.ghost_delay[k], p.ghost_gain[k] = d, g
    return p


def float_forms_take(row, p):
    """launch_records()'s rule for NTSCSIM_MODE_FLOAT (`fp`), in terms of a row and its parameters p (ntscsim_params): the
    all-float kernels run the two presets with their standard switches, head-switch displacements up to W/10 and frames
    with 16-byte rows (every row of the table has them); anything else runs the FAST32 forms"""
    if row.mode != HT or row.ghost or DEC_WR in row.names:
        return False
    even_phase = p.video_scanline_phase_shift not in (90, 270) and not (p.video_scanline_phase_shift_offset & 1)
    enc_preset = (p.composite_in_chroma_lowpass and p.video_noise != 0 and p.subcarrier_amplitude == 50 and
                  not (p.composite_preemphasis != 0 and p.composite_preemphasis_cut > 0))
    if not (enc_preset and even_phase) or p.nocolor_subcarrier or p.subcarrier_amplitude_back != 50:
        return False
    if not (p.composite_out_chroma_lowpass and p.composite_out_chroma_lowpass_lite):
        return False
    if p.emulating_vhs:
        return bool(not p.vhs_svideo_out and p.video_chroma_noise and p.video_chroma_phase_noise)
    return not p.video_chroma_noise and not p.video_chroma_phase_noise


# the rows of the table that NTSCSIM_MODE_FLOAT runs on its own kernels (they belong to tests/test_float_model_gpu.py):
# the families def, sp, lp, ep (10 rows for def and sp, 9 for lp and ep) and own_vhs_lp_only, own_interlaced_tff / _bff
N_FLOAT_ROWS = 10 + 10 + 9 + 9 + 3


# ------------------------------------------------------------------------------------------------ the role kernels
# ntscsim_field() call after call; the switch sets of test_synchronous_call_takes_the_pipelined_form_and_equals_the_oracle
# (tests/test_gpu_parity.py), one per size
def _roles():
    out = []
    sets = {
        "k_field_pipe<float>": [VHS, LP, EP, VHS + DROP, VHS],
        "k_field_pipe<float,true>": [PAL, VHS + ["-vhs-head-switching-phase", "0.003"], PAL,
                                     VHS + ["-vhs-head-switching-phase", "0.001"], PAL],
        "k_field_pipe_sv<float>": [VHS + SV, VHS + SV, EP + SV + DROP, VHS + SV, PAL + SV],
        "k_field_pipe_xi<float>": [VHS + ["-comp-phase", "90"], VHS + ["-comp-phase", "90"], VHS + ["-comp-phase-offset", "1"],
                                   PAL + ["-comp-phase", "90"], VHS + ["-comp-phase", "270"]],
        "k_field_pipe_catv<float>": [VHS + ["-comp-catv"], VHS + ["-comp-catv"], VHS + ["-comp-catv4"],
                                     PAL + ["-comp-catv3"], VHS + ["-comp-catv2"]],
        "k_field_pipe_tv<float>": [[], [], ["-noise", "30", "-chroma-dropout", "20000"], ["-vhs-head-switching", "1"], []],
        "k_field_pipe_tv_catv<float>": [["-comp-catv"], ["-comp-catv", "-chroma-dropout", "20000", "-vhs-head-switching", "1"],
                                        ["-comp-catv4"] + NOPN, ["-comp-catv3"], ["-comp-catv2"]],
    }
    for name in ROLE_NAMES:
        odd = name not in ("k_field_pipe<float>", "k_field_pipe<float,true>", "k_field_pipe_sv<float>")
        sizes = [(16, 4), (21, 9) if odd else (20, 9), (36, 130), (256, 100), (720, 486)]
        for flags, (w, h) in zip(sets[name], sizes):
            tag = name[len("k_field_"):].replace("<float>", "").replace("<float,true>", "_wr")
            out.append(Role("%s_%dx%d" % (tag, w, h), list(flags), w, h, name))
    return out


ROLES = _roles()
# switch sets that take no role kernel, in float either
NO_ROLE = [Role("xi_svideo_256x100", VHS + ["-comp-phase", "90"] + SV, 256, 100, None),
           Role("tv_catv_cnoise_256x100", ["-comp-catv", "-chroma-noise", "5"], 256, 100, None)]
# device-resident launches in the latency form (ntscsim_set_launch_form): (flags, name) x (fields, w, h)
LATENCY = [(VHS, "k_field_pipe<float>"), ([], "k_field_pipe_tv<float>"), (VHS + ["-comp-catv"], "k_field_pipe_catv<float>")]
LATENCY_SIZES = [(2, 256, 100), (64, 100, 35)]


def all_names():
    s = set(ROLE_NAMES)
    for r in ROWS:
        s.update(r.names)
    return s

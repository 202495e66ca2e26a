"""The table of the BGRA tool's ROLE kernels in double (csrc/ntsc_pipe.hip: k_field_pipe<RT,WR,SV,XA,CATV>, five wavefronts per 63
rows, and k_field_pipe_tv<RT,CATV>, three): every name launch_records() (csrc/ntscsim_hip.hip) can note for a launch in the
latency form, at the widths of the kernels' own loop conditions, with the row packings, head-switch displacements and switch
sets that reach it -- and the rows that must fall back to a one-launch form, with that form's decoder name.  Shared by
tests/test_pipe_forms_host.py (CPU: closure over the launcher's names, coverage of every condition, the oracle's properties
of the rows) and tests/test_pipe_forms_gpu.py (equality with the oracle, row by row).  Test infrastructure only; no GPU import.

A row: (id, flags, w, h, n, source, kernel, fallback, hs)
  source    "noise": the frames are noise (field k reads frame k % 2); "mixed": noise, bars and a ramp in turn
  kernel    the ONE role-kernel name ntscsim_debug_last_kernels() must report, or None
  fallback  where kernel is None: the one-launch decoder's name the launch must report instead
  hs        None, or the head-switch class the row claims (what the oracle's displacements must show):
              "none"   head switching on, the wrap-around form taken, no row of the picture displaced
              "small"  rows displaced, every displacement within W/10
              "fwd"    the largest forward displacement beyond W/10 (wg_reach: mx + 2)
              "wide"   a backward displacement beyond W/10 (wg_reach: W -- the row's first samples come from its end)
              "last"   as "wide", in a launch of two workgroups whose first holds no displaced row
What the columns cannot say stands beside the table, by row id: GHOST (taps of the ghosting extension), DEBUG (bits of
ntscsim_debug_no_fast_decode), UNALIGNED (destination rows that are no multiple of 16 bytes).
Field k of a launch has parity (k & 1) ^ 1 and field number k, as the tool's loop counts them.
"""
import functools
import math
import re
from collections import namedtuple

import numpy as np

Row = namedtuple("Row", "id flags w h n source kernel fallback hs")
Sync = namedtuple("Sync", "id flags w h kernel")
Family = namedtuple("Family", "tag kernel base d sv tv pal hs")

# ------------------------------------------------------------------------------------------------ the kernels' constants
# (tests/test_pipe_forms_host.py reads the same numbers out of csrc/ntsc_pipe.hip)
RING = 16          # stream positions per LDS ring
MAX_FIELDS = 64    # launches of more fields keep the throughput form (NTSC_PIPE_MAX_FIELDS)
WG_ROWS = 63       # rows per workgroup; lane 0 is the halo lane
STEP = 4           # positions per steady trip
CHUNK = 16         # pixels per encoder chunk
HEAD = 4           # pixels the encoder asks for ahead of its chunks
MIN_W = 16         # the C ABI refuses narrower frames (NTSCSIM_E_SIZE)
FULL = 720


def skt(d, sv, tv=False):
    """the depth of the decoder: the position at which the steady loop starts"""
    return 8 if tv else (8 if sv else 15) + d


def t_end(w, d):
    return w - max(d - 7, 0)


def has_steady(w, d, sv, tv=False):
    return skt(d, sv, tv) + STEP <= t_end(w, d)


def steady_first(d, sv, tv=False):
    """the first width with a steady loop: 30 / 36 / 40 for SP / LP / EP, 23 / 29 / 33 with S-Video, 12 without the VCR"""
    return skt(d, sv, tv) + STEP + max(d - 7, 0)


def trips(w, d, sv, tv=False):
    return (t_end(w, d) - skt(d, sv, tv)) // STEP if has_steady(w, d, sv, tv) else 0


def drain_class(w, d, sv, tv=False):
    """guarded positions between the steady loop's end and t_end"""
    return (t_end(w, d) - skt(d, sv, tv)) % STEP


def flush_class(w, d, sv, tv=False):
    """the `sub` at which the output role's steady loop stops: 4 * flush_class pixels wait in ostage for the drain"""
    return ((t_end(w, d) - skt(d, sv, tv)) // STEP) % 4


def enc_chunks(w):
    return (w - HEAD) // CHUNK if w >= HEAD + CHUNK else 0


def enc_tail(w):
    return (w - HEAD) % CHUNK


def enc_more(w):
    """a chunk that requests the next one while it runs: `t + 32 <= W` at t = 4"""
    return w >= HEAD + 2 * CHUNK


def lslot(h):
    return (h + 1) // 2


def workgroups(h, n):
    return (n * lslot(h) + WG_ROWS - 1) // WG_ROWS


def lanes(h, n, wg):
    """(rc, field index, row k of the field, rowok) of the 64 lanes of a workgroup: k_field_pipe's own index arithmetic"""
    R, out = n * lslot(h), []
    for lane in range(64):
        g = wg * WG_ROWS + lane - 1
        rc = 0 if g < 0 else min(g, R - 1)
        f = rc // lslot(h)
        k = rc - f * lslot(h)
        field = (f & 1) ^ 1
        out.append((rc, f, k, field + 2 * k < h))
    return out


# ------------------------------------------------------------------------------------------------ the names and switch sets
K_PLAIN, K_WR, K_SV, K_XI = "k_field_pipe<double>", "k_field_pipe<double,true>", "k_field_pipe_sv<double>", "k_field_pipe_xi<double>"
K_CATV, K_TV, K_TVC = "k_field_pipe_catv<double>", "k_field_pipe_tv<double>", "k_field_pipe_tv_catv<double>"
ROLE_NAMES = [K_PLAIN, K_WR, K_SV, K_XI, K_CATV, K_TV, K_TVC]
FLOAT_NAME = {k: k.replace("double", "float") for k in ROLE_NAMES}
WR_CAPABLE = (K_WR, K_SV, K_XI, K_CATV)          # the instantiations with wrap-around loads (wg_reach<true>)

VHS = ["-vhs"]
LP = ["-vhs", "-vhs-speed", "lp"]
EP = ["-vhs", "-vhs-speed", "ep"]
SV = ["-vhs-svideo", "1"]
PAL = ["-tvstd", "pal"]
P90, P270, OFF1 = ["-comp-phase", "90"], ["-comp-phase", "270"], ["-comp-phase-offset", "1"]
HS_ON = ["-vhs-head-switching", "1"]
NOPN = ["-chroma-phase-noise", "0"]
DROP = ["-chroma-dropout", "50000"]
NOBLEND = ["-vhs-chroma-vblend", "0"]
LOUD = ["-noise", "40", "-chroma-noise", "70"]
LOUD_TV = ["-noise", "30"]

DELAY = {"sp": 9, "lp": 12, "ep": 14}


def hs_flags(w, kind, row=4, pal=False):
    """-vhs-head-switching-point / -phase that put the switch into frame row `row` + field (`row` even: the rows below it are
    displaced) and displace by the class's amount.  The tool's jitter of both (1/500 of a line, four rand() calls per
    field) stays on: the margins are wider than it up to 130 columns; "none" leaves the point where it is (below the
    picture) and keeps the displacement of "wide"."""
    tw = w + w // 10
    lines = 312.5 if pal else 262.5
    line = (row + (48 if pal else 44)) // 2
    near = min(w // 10, max(2, w // 20))
    hx = {"small": near, "back": tw - near, "fwd": w // 10 + max(2, w // 8),
          "wide": tw - (w // 10 + max(3, w // 5))}["wide" if kind in ("none", "last") else kind]
    assert (hx < tw // 2) == (kind in ("small", "fwd"))
    out = ["-vhs-head-switching-phase", "%.9f" % ((tw + hx + 0.5) / (tw * lines))]
    if kind != "none":
        out = ["-vhs-head-switching-point", "%.9f" % ((line + 0.5) / lines)] + out
    return out


# per family: the role name, the base switch set, the chroma delay, S-Video, no VCR, PAL, and the head-switch class its
# width rows carry (their switch set then depends on the width)
FAMILIES = [
    Family("sp", K_PLAIN, VHS, 9, False, False, False, None),
    Family("lp", K_PLAIN, LP, 12, False, False, False, None),
    Family("ep", K_PLAIN, EP, 14, False, False, False, None),
    Family("sv_sp", K_SV, VHS + SV, 9, True, False, False, None),
    Family("sv_lp", K_SV, LP + SV, 12, True, False, False, None),
    Family("sv_ep", K_SV, EP + SV, 14, True, False, False, None),
    Family("wr_sp", K_WR, VHS, 9, False, False, False, "wide"),
    Family("wr_ep", K_WR, EP, 14, False, False, False, "fwd"),
    Family("xi_p90", K_XI, VHS + P90, 9, False, False, False, None),
    Family("xi_off1_ep", K_XI, EP + OFF1, 14, False, False, False, None),
    Family("xi_p270_pal", K_XI, PAL + VHS + P270, 9, False, False, True, None),
    Family("catv", K_CATV, VHS + ["-comp-catv"], 9, False, False, False, None),
    Family("catv3_ep", K_CATV, EP + ["-comp-catv3"], 14, False, False, False, None),
    Family("tv", K_TV, [], 0, False, True, False, None),
    Family("tv_hs", K_TV, HS_ON, 0, False, True, False, "small"),
    Family("tvc2", K_TVC, ["-comp-catv2"], 0, False, True, False, None),
    Family("tvc4_nopn", K_TVC, ["-comp-catv4"] + NOPN, 0, False, True, False, None),
]
FAM = {f.tag: f for f in FAMILIES}


def fam_flags(f, w, h=10):
    """a family's switch set at a width (head-switch families: the switch in frame row 4 + field)"""
    return f.base + (hs_flags(w, f.hs, 4, f.pal) if f.hs else [])


def first_width(f):
    """the first of the twenty consecutive widths: two below the steady threshold, or the narrowest frame the C ABI takes
    (without the VCR the threshold, 12, lies below it: those forms always have a steady loop)"""
    return max(MIN_W, steady_first(f.d, f.sv, f.tv) - 2)


ENC_W = (16, 17, 19, 20, 21, 35, 36, 51, 52, 53, 67, 68)      # no chunk | the first | `more` | the rand() ring half back at 0 | a fourth


def widths(f):
    lo = first_width(f)
    return sorted(set(range(lo, lo + 20)) | set(ENC_W) | {FULL})


def threshold_widths(f):
    """the widths repeated in NTSCSIM_MODE_FAST32"""
    s = steady_first(f.d, f.sv, f.tv)
    return sorted({max(MIN_W, s - 1), max(MIN_W, s), max(MIN_W, s + 1), FULL})


# The listed switches, each with what it does to the parameters: (tag, flags per kind of family, predicate)
SWITCH_W = (21, 44, 100)          # below every VCR family's threshold but S-Video SP's | above all of them | several chunks
SWITCHES = [
    ("drop", lambda f: DROP, lambda p: p.video_chroma_loss == 50000),
    ("noblend", lambda f: None if f.tv else NOBLEND, lambda p: not p.vhs_chroma_vert_blend),
    ("loud", lambda f: LOUD_TV if f.tv else LOUD, lambda p: p.video_noise >= 30),
    ("pal", lambda f: None if f.pal else PAL, lambda p: p.tv_standard == 1),
]
SWITCH_FAMILIES = ("sp", "ep", "sv_sp", "wr_sp", "xi_p90", "catv", "tv", "tvc2")

PACK_FAMILIES = ("sp", "sv_sp", "xi_p90", "tv")
PACK_W = (36, 100)
PACK_H = (124, 125, 126, 127, 128, 130)

GHOST, DEBUG, UNALIGNED = {}, {}, set()

# the one-launch decoders the fallback rows name
D_VHS, D_TV, D_SV, D_XI, D_FO = ("k_decode_fast<true,double>", "k_decode_fast<false,double>", "k_decode_fast_sv<double>",
                                 "k_decode_fast_xi<double>", "k_decode_fast_fo<double>")
D_BK, D_BK_TV = "k_decode_fast_bk<true,double>", "k_decode_fast_bk<false,double>"
G_VHS, G_TV, G_SV, T_VHS = ("k_decode<true,true,1u,double>", "k_decode<false,false,1u,double>", "k_decode<true,false,1u,double>",
                            "k_decode<true,true,6u,double>")
T_TV = "k_decode<false,false,0u,double>"
ONE_LAUNCH = {K_PLAIN: D_VHS, K_WR: "k_decode_fast<true,double,true>", K_SV: D_SV, K_XI: D_XI, K_CATV: D_BK, K_TV: D_TV, K_TVC: D_BK_TV}


def _rows():
    out = []

    def add(name, flags, w, h, n, kernel, fallback=None, source="noise", hs=None):
        assert (kernel is None) != (fallback is None)
        out.append(Row(name, list(flags), w, h, n, source, kernel, fallback, hs))

    for f in FAMILIES:
        # ---- the widths of the loops: two fields of five rows, one workgroup
        for w in widths(f):
            add("%s_w%d" % (f.tag, w), fam_flags(f, w), w, 10, 2, f.kernel, source="mixed" if w == FULL else "noise", hs=f.hs)
    # ---- PAL's default switching point: beyond W/10 at every width, below a picture of 36 rows
    for tag in ("sp", "ep"):
        f = FAM[tag]
        s = steady_first(f.d, False)
        for w in (s - 1, s, s + 1, 100):
            add("wr_pal_%s_w%d" % (tag, w), PAL + f.base, w, 36, 2, K_WR, hs="none")
    # ---- rows through the workgroups
    for tag in PACK_FAMILIES:
        f = FAM[tag]
        for w in PACK_W:
            for h in PACK_H:
                for n in (1, 2, 3):
                    add("%s_pack_%dx%d_n%d" % (tag, w, h, n), f.base, w, h, n, f.kernel)
        add("%s_pack_36x10_n%d" % (tag, MAX_FIELDS), f.base, 36, 10, MAX_FIELDS, f.kernel, source="mixed")
        add("%s_pack_36x10_n%d" % (tag, MAX_FIELDS + 1), f.base, 36, 10, MAX_FIELDS + 1, None, ONE_LAUNCH[f.kernel], source="mixed")
    # ---- head switching on every instantiation with wrap-around loads: each outcome of wg_reach<true>
    for tag, base in (("wr", VHS), ("sv", VHS + SV), ("xi", VHS + P90), ("catv", VHS + ["-comp-catv"])):
        kernel = {"wr": K_WR, "sv": K_SV, "xi": K_XI, "catv": K_CATV}[tag]
        for w in (36, 100):
            for kind in ("none", "fwd", "wide"):
                add("%s_hs_%s_%dx36" % (tag, kind, w), base + hs_flags(w, kind, 10), w, 36, 2, kernel, hs=kind)
            add("%s_hs_last_%dx130" % (tag, w), base + hs_flags(w, "last", 124), w, 130, 1, kernel, hs="last")
        if tag != "wr":       # (within W/10 the plain family takes k_field_pipe<double>: its rows are below)
            add("%s_hs_small_36x36" % tag, base + hs_flags(36, "small", 10), 36, 36, 2, kernel, hs="small")
            add("%s_hs_back_100x36" % tag, base + hs_flags(100, "back", 10), 100, 36, 2, kernel, hs="small")
    add("sp_hs_small_36x36", VHS + hs_flags(36, "small", 10), 36, 36, 2, K_PLAIN, hs="small")
    add("sp_hs_back_100x36", VHS + hs_flags(100, "back", 10), 100, 36, 2, K_PLAIN, hs="small")
    add("tv_hs_back_100x36", HS_ON + hs_flags(100, "back", 10), 100, 36, 2, K_TV, hs="small")
    add("tvc2_hs_small_36x36", ["-comp-catv2"] + HS_ON + hs_flags(36, "small", 10), 36, 36, 2, K_TVC, hs="small")
    # (beyond W/10 the forms without the VCR have no wrap-around loads: they leave)
    add("tv_hs_wide_36x36", HS_ON + hs_flags(36, "wide", 10), 36, 36, 2, None, T_TV, hs="wide")
    # ---- switches each form's condition allows
    for tag in SWITCH_FAMILIES:
        f = FAM[tag]
        for sw, flags_of, _ in SWITCHES:
            extra = flags_of(f)
            if extra is None:
                continue
            for w in SWITCH_W:
                base = fam_flags(f, w)
                flags = extra + base if sw == "pal" else base + extra
                if sw == "pal" and f.hs:       # (the point of the switch counts PAL's lines)
                    flags = PAL + f.base + hs_flags(w, f.hs, 4, True)
                # (PAL's default switching point lies beyond W/10: the plain families take the wrap-around form)
                wr = sw == "pal" and f.kernel == K_PLAIN
                add("%s_%s_w%d" % (tag, sw, w), flags, w, 10, 2, K_WR if wr else f.kernel, hs="none" if wr else f.hs)
    # ---- rows that must fall back although the launch is short and aligned
    for w in (36, 100):
        add("leave_nocolor_w%d" % w, VHS + ["-nocolor-subcarrier"], w, 10, 2, None, G_VHS)
        add("leave_xi_sv_w%d" % w, VHS + P90 + SV, w, 10, 2, None, G_SV)
        add("leave_tvcatv_cnoise_w%d" % w, ["-comp-catv", "-chroma-noise", "5"], w, 10, 2, None, G_TV)
        add("leave_tv_noise0_w%d" % w, ["-noise", "0"], w, 10, 2, None, D_TV)
        add("leave_vhs_noise0_w%d" % w, VHS + ["-noise", "0"], w, 10, 2, None, D_VHS)
        add("leave_full_lp_w%d" % w, VHS + ["-out-composite-lowpass-lite", "0"], w, 10, 2, None, D_FO)
        add("leave_no_lp_w%d" % w, VHS + ["-out-composite-lowpass", "0"], w, 10, 2, None, G_VHS)
        add("leave_tv_full_lp_w%d" % w, ["-out-composite-lowpass-lite", "0"], w, 10, 2, None, G_TV)
        add("leave_ghost_w%d" % w, VHS, w, 10, 2, None, D_VHS)
        GHOST["leave_ghost_w%d" % w] = ((12, 64),)
        add("leave_tv_ghost_w%d" % w, [], w, 10, 2, None, D_TV)
        GHOST["leave_tv_ghost_w%d" % w] = ((3, 64), (9, -32))
        add("leave_debug_w%d" % w, VHS, w, 10, 2, None, T_VHS)
        DEBUG["leave_debug_w%d" % w] = 1
        add("leave_unaligned_w%d" % w, VHS, w, 10, 2, None, T_VHS)
        UNALIGNED.add("leave_unaligned_w%d" % w)
        add("leave_tv_unaligned_w%d" % w, [], w, 10, 2, None, T_TV)
        UNALIGNED.add("leave_tv_unaligned_w%d" % w)
    return out


ROWS = _rows()
assert len({r.id for r in ROWS}) == len(ROWS)
BY_ID = {r.id: r for r in ROWS}


def loop_consts(p):
    """(d, sv, tv) of a parameter set: what the loop conditions above take"""
    tv = not p.emulating_vhs
    return (0 if tv else {0: 9, 1: 12, 2: 14}[p.output_vhs_tape_speed]), bool(p.vhs_svideo_out) and not tv, tv


def _sync():
    """ntscsim_field() call after call: per role name one width below the steady threshold (the narrowest frame where the
    threshold is out of reach), the width at it, and 720x486"""
    out = []
    for tag in ("sp", "wr_sp", "sv_sp", "xi_p90", "catv", "tv", "tvc2"):
        f = FAM[tag]
        s = steady_first(f.d, f.sv, f.tv)
        for w, h in ((max(MIN_W, s - 1), 12), (max(MIN_W + 1, s), 12), (FULL, 486)):
            # (the default switching point, 16 rows above the end of a 486-row picture, displaced by a fifth of a row)
            flags = VHS + ["-vhs-head-switching-phase", "0.003"] if tag == "wr_sp" else f.base
            out.append(Sync("%s_sync_%dx%d" % (tag, w, h), list(flags), w, h, f.kernel))
    return out


SYNC = _sync()
SYNC_OTHER = (48, 14)          # the second geometry of a context, run between two visits of the row's own


# ------------------------------------------------------------------------------------------------ the launcher's rule
def hs_small(p, w):
    """head_switch_is_small() (csrc/ntscsim_hip.hip): every displacement the jitter allows lies within W/10"""
    if not p.vhs_head_switching:
        return True
    tw = w + w // 10
    t = tw * (262.5 if p.tv_standard == 0 else 312.5)
    pn = abs(p.vhs_head_switching_phase_noise)
    lo, hi = p.vhs_head_switching_phase - pn, p.vhs_head_switching_phase + pn
    if lo < 0 or math.trunc(lo) != math.trunc(hi):
        return False
    plo, phi = int((lo - math.trunc(lo)) * t), int((hi - math.trunc(hi)) * t)
    if plo // tw != phi // tw:
        return False
    a, b = plo % tw, phi % tw
    if (a >= tw // 2) != (b >= tw // 2):
        return False
    a, b = (a - tw if a >= tw // 2 else a), (b - tw if b >= tw // 2 else b)
    return max(abs(a), abs(b)) <= tw - w


def launcher_name(p, w, n, aligned=True, latency=True, debug=0, ghost=0):
    """launch_records()'s choice for NTSCSIM_MODE_EXACT in terms of the parameters (planes far below 4 GiB: fast_plane_ok
    holds): (role-kernel name or None, the one-launch decoder's name)"""
    no_fast, split = bool(debug & 1), bool(debug & 2)
    even = p.video_scanline_phase_shift not in (90, 270) and not (p.video_scanline_phase_shift_offset & 1)
    pre_on = p.composite_preemphasis != 0 and p.composite_preemphasis_cut > 0
    out_lp = (1 if p.composite_out_chroma_lowpass_lite else 2) if p.composite_out_chroma_lowpass else 0
    amp, back = p.subcarrier_amplitude, p.subcarrier_amplitude_back
    vhs, sv = bool(p.emulating_vhs), bool(p.vhs_svideo_out)
    cn, pn = p.video_chroma_noise != 0, p.video_chroma_phase_noise != 0
    small = hs_small(p, w)
    enc_preset = bool(p.composite_in_chroma_lowpass) and not pre_on and p.video_noise != 0 and amp == 50
    enc_preset_pre = bool(p.composite_in_chroma_lowpass) and pre_on and p.video_noise != 0 and amp == 50
    short = latency and n <= MAX_FIELDS and not no_fast and aligned and ghost == 0
    common = not p.nocolor_subcarrier and out_lp == 1 and amp == 50
    pipe_xa = not even and not sv
    pipe_catv = enc_preset_pre and back != 50 and back >= 2 and even and not sv
    pipe_form = (short and common and not split and vhs and cn and pn and
                 (pipe_catv or (enc_preset and back == 50 and (even or pipe_xa))))
    pipe_tv = short and enc_preset and even and common and back == 50 and small and not vhs and not cn and not pn
    pipe_tvc = short and enc_preset_pre and even and common and back != 50 and back >= 2 and small and not vhs and not cn
    role = None
    if pipe_tv or pipe_tvc:
        role = K_TVC if pipe_tvc else K_TV
    elif pipe_form:
        role = K_CATV if pipe_catv else K_XI if not even else K_SV if sv else K_WR if not small else K_PLAIN
    # the decoder of the one-launch forms
    back50 = back == 50
    dec_base = not p.nocolor_subcarrier and out_lp == 1 and amp == 50
    dec_common = dec_base and back50
    dec_fast = dec_base and (back50 or back >= 2) and not no_fast and aligned and even
    both = cn and pn
    if (not p.nocolor_subcarrier and out_lp == 2 and amp == 50 and back50 and not no_fast and aligned and even and vhs and not sv
            and both):
        one = D_FO
    elif dec_base and back50 and not no_fast and aligned and not even and vhs and not sv and both:
        one = D_XI
    elif dec_fast and back50 and small and vhs and not sv and both:
        one = D_VHS
    elif dec_fast and back50 and vhs and not sv and both:
        one = ONE_LAUNCH[K_WR]
    elif dec_fast and not back50 and vhs and not sv and both:
        one = D_BK
    elif dec_fast and back50 and vhs and sv and both:
        one = D_SV
    elif dec_fast and back50 and small and not vhs and not cn and not pn:
        one = D_TV
    elif dec_fast and not back50 and small and not vhs and not cn and not pn:
        one = D_BK_TV
    elif not vhs:
        one = T_TV if dec_common and not cn and not pn else G_TV
    elif sv:
        one = G_SV
    else:
        one = T_VHS if dec_common and both else G_VHS
    return role, one


# ------------------------------------------------------------------------------------------------ frames and the oracle
FILL = 0x77


def params(row):
    import _libs as L
    p = L.make_params(row.flags)
    taps = GHOST.get(row.id, ())
    p.ghost_taps = len(taps)
    for k, (d, g) in enumerate(taps):
        p.ghost_delay[k], p.ghost_gain[k] = d, g
    return p


def row_pixels(row):
    """pixels per row of the launch's device frames: at least one pixel of padding behind every row, rows of a multiple of
    16 bytes -- or, for the rows that say so, of 16 bytes + 4"""
    pw = (row.w + 4) // 4 * 4
    return pw + 1 if row.id in UNALIGNED else pw


def sources(kind, w, h):
    import _libs as L
    import _modes as M
    return M.sources(kind, w, h)


def displacements(comp, hsy, w):
    """the displacement of every row of a field from the oracle's composite_y and headswitch_y taps: the s with
    headswitch_y[x] == row[(x + s) mod 1.1 W] over the row padded with zeros (ffmpeg_ntsc.cpp:1647-1713); exactly one fits"""
    tw = w + w // 10
    out = []
    for c, h in zip(comp, hsy):
        if np.array_equal(c, h):
            out.append(0)
            continue
        ext = np.zeros(tw, np.int64)
        ext[:w] = c
        idx = (np.arange(w)[None, :] + np.arange(-(tw // 2), tw // 2 + 1)[:, None]) % tw
        fit = np.flatnonzero((ext[idx] == h[None, :]).all(axis=1))
        assert len(fit) == 1, fit
        out.append(int(fit[0]) - tw // 2)
    return out


def wg_branches(row, shifts):
    """the outcome of wg_reach<true> in every workgroup of a row's launch: "none" (reach 2), "fwd" (mx + 2), "wide" (W)"""
    out = []
    for wg in range(workgroups(row.h, row.n)):
        s = [shifts[f][k] if ok else 0 for (_, f, k, ok) in lanes(row.h, row.n, wg)]
        out.append("wide" if min(s) < -(row.w // 10) else "fwd" if max(s) > 0 else "none")
    return out


Case = namedtuple("Case", "srcs jobs exp rng_pos comp shifts")


@functools.lru_cache(maxsize=2)
def case(row_id):
    """The launch of a row and what the oracle makes of it: n destination frames and a guard frame of row_pixels() pixels per
    row, FILL everywhere, the oracle's field in the rows of each job's parity; the composite_y tap and the displacement of
    every row of every field"""
    import _libs as L
    row = BY_ID[row_id]
    p = params(row)
    w, h, n = row.w, row.h, row.n
    srcs = sources(row.source, w, h)
    jobs = [(k % len(srcs), (k & 1) ^ 1, k) for k in range(n)]
    exp = np.full((n + 1, h, row_pixels(row), 4), FILL, np.uint8)
    o = L.OracleStream(p)
    comp, shifts = [], []
    for k, (si, field, fieldno) in enumerate(jobs):
        d = np.full((h, w, 4), FILL, np.uint8)
        t = o.field(d, srcs[si], field, fieldno, taps=["composite_y", "headswitch_y"])
        exp[k, :, :w] = d
        comp.append(t["composite_y"])
        # (the second tap sits behind the ghosting extension: rows with taps claim no displacement and have none to show)
        moved = p.vhs_head_switching and not p.ghost_taps
        shifts.append(displacements(t["composite_y"], t["headswitch_y"], w) if moved else [0] * len(d[field::2]))
    exp.setflags(write=False)
    return Case(srcs, jobs, exp, o.rng_pos, comp, shifts)


def plane_is_the_tap(row):
    """tests/_fast32_forms.py's rule: the exposed plane is the encoder's, the oracle's tap sits in front of the ghosting
    extension -- they differ where the ghosting is folded into the encoder (every ghosting row of this table: delays below 64)"""
    return row.id not in GHOST


def string_literals(text):
    """the string literals of a C++ source (none of the ones looked for holds an escape)"""
    return re.findall(r'"([^"\\\n]*)"', text)

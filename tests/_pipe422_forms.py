"""The table of the YUV422P tool's ROLE kernels (csrc/ntsc422_fused.hip: k422_pipe<SPEC,DD,SVID>, k422_short_pipe): every name
launch422() (csrc/ntscsim_hip.hip) can note for a launch in the latency form, at the widths of the kernels' own loop
conditions, with the row packings, layouts, sources and switch sets that reach it -- and the rows that must fall back to a
one-wave form, with that form's name.  Shared by tests/test_pipe422_forms_host.py (CPU: closure over the launcher's names,
coverage of every condition, the oracle's properties of the rows) and tests/test_pipe422_forms_gpu.py (equality with the
oracle, row by row).  Test infrastructure only; no GPU import.

A row: (id, flags, w, h, n, layout, source, kernel, fallback, share, hs)
  layout    "padded"     luma rows 16-byte and chroma rows 8-byte aligned, luma linesize >= W + 2 (nothing is excluded)
            "tight"      linesize == W (a multiple of 16): the two bytes behind a luma row are the next row's
            "odd"        luma linesize W + 3: the streamed forms' precondition fails
            "odd-chroma" luma rows aligned, chroma linesize W/2 + 4 (+ 1 where that is a multiple of 8): the precondition fails
                         in chroma alone
            "odd-luma"   luma linesize W + 3, chroma rows 8-byte aligned (the planes start at multiples of 16): it fails in
                         luma alone (tests/_sweep422_forms.py)
  source    "inplace"  the frames hold the pictures; "src" / "src420" / "src-il": through k422_render from progressive 4:2:2,
            progressive 4:2:0 and interlaced (top field first, second field) 4:2:2 sources
  kernel    the ONE role-kernel name ntscsim_debug_last_kernels() must report, or None
  fallback  where kernel is None: the one-wave form's name the launch must report instead
  share     both fields of ONE frame in one launch (n = 2)
  hs        None, or the kind of head-switch displacement the row claims: "fwd", "back" (within W/10), "wide" (far beyond
            W/10), "wide1" (the first row below the switch displaced by exactly W/10 + 1: the gather's `reach` condition)
Field k of a launch has parity (k & 1) ^ 1 and field number k, as the tool's loop counts them.
"""
import functools
import re
from collections import namedtuple

import numpy as np

Row = namedtuple("Row", "id flags w h n layout source kernel fallback share hs")
Sync = namedtuple("Sync", "id flags w h kernel")

# ------------------------------------------------------------------------------------------------ the kernels' constants
# (tests/test_pipe422_forms_host.py reads the same numbers out of csrc/ntsc422_fused.hip)
XR = 32            # iterations of the LDS ring between front and back
EDGE = 8           # guarded iterations in front of the steady loop: `for (; i < 8 && i < NIT; i++) edge(i)`
STEP = 4           # iterations per steady trip
HB = 16            # samples per step of the gather
BURST = 64         # bytes per published group of sweep A and per frame burst
GROUP = 32         # chroma inputs per group of sweep A
MAX_FIELDS = 64    # launches of more fields keep the throughput form (pipe_max_fields)
WG_ROWS = 63       # rows per workgroup; lane 0 is the halo lane


def nit(w, dd):
    """iterations of the streamed pass per row"""
    return w // 2 + dd + 2


def steady(w, dd):
    """`i == 8 && i + 3 <= W2 - 2 - DD`: front and back enter their steady loop"""
    return EDGE + STEP - 1 <= w // 2 - 2 - dd


def steady_first(dd):
    """the first (even) width with a steady loop: 34, 36, 38 for DD = 4, 5, 6"""
    return 2 * (EDGE + STEP - 1 + 2 + dd)


def epilogue_class(w, dd):
    """the residue that sets the number of guarded iterations behind the steady loop"""
    return (w // 2 - dd) % STEP


def ring_wraps(w, dd):
    return nit(w, dd) > XR


def ring_last(dd):
    """the last width whose iterations all fit the ring: 52, 50, 48"""
    return 2 * (XR - 2 - dd)


def a_delay(pal):
    return 2 if pal else 4


def a_groups(w, pal=False):
    """trips of `for (g0 = 0; g0 < W2 + D; g0 += 32)`"""
    return (w // 2 + a_delay(pal) + GROUP - 1) // GROUP


def a_fast_groups(w):
    """groups that take the guard-free form: `g0 >= 32 && g0 + 32 <= W2`"""
    return sum(1 for g0 in range(0, w // 2 + 4, GROUP) if g0 >= GROUP and g0 + GROUP <= w // 2)


def a_publishes_early(w, pal=False):
    """sweep A publishes a byte count before its last one: a group with g0 >= 32 exists (`done = 2 * (g0 - D) > 0`)"""
    return a_groups(w, pal) >= 2


def groups_edge(k, pal=False):
    """the last width with k groups"""
    return 2 * (k * GROUP - a_delay(pal))


def fast_first(k):
    """the first width with k guard-free groups: 128, 192"""
    return 2 * GROUP * (k + 1)


GATHER = (BURST - 2, BURST, BURST + 2)          # W mod 16 in {14, 0, 2} and W mod 64 in {62, 0, 2}
FULL = 720


def widths(dd, pal=False):
    """both sides of every condition for chroma delay dd"""
    s = steady_first(dd)
    ws = {HB, HB + 2, s - 2, s}
    ws.update(s + 2 * k for k in range(5))                       # four consecutive even widths above the threshold
    ws.update((ring_last(dd), ring_last(dd) + 2))
    for k in (1, 2):
        ws.update((groups_edge(k, pal), groups_edge(k, pal) + 2))
    for k in (1, 2):
        ws.update((fast_first(k) - 2, fast_first(k), fast_first(k) + 2))
    ws.update(GATHER)
    ws.add(FULL)
    return sorted(ws)


# ------------------------------------------------------------------------------------------------ the names and switch sets
P_SPEC = "k422_pipe<true,4>"
P_GEN = {4: "k422_pipe<false,4>", 5: "k422_pipe<false,5>", 6: "k422_pipe<false,6>"}
P_SV = {4: "k422_pipe_sv<4>", 5: "k422_pipe_sv<5>", 6: "k422_pipe_sv<6>"}
P_DIRECT = "k422_direct_pipe"
ROLE_NAMES = [P_SPEC] + [P_GEN[d] for d in (4, 5, 6)] + [P_SV[d] for d in (4, 5, 6)] + [P_DIRECT]
# the one-wave form of each role form: what a launch of more than 64 fields reports
ONE_WAVE = {P_SPEC: "k422_fused<true,true,4>", P_DIRECT: "k422_direct_fast"}
ONE_WAVE.update({P_GEN[d]: "k422_fused<false,true,%d>" % d for d in (4, 5, 6)})
ONE_WAVE.update({P_SV[d]: "k422_fused_sv<%d>" % d for d in (4, 5, 6)})
DD = {P_SPEC: 4, P_DIRECT: 4}                   # (the no-VCR form has no delay line; it takes the widths of DD = 4 along)
DD.update({P_GEN[d]: d for d in (4, 5, 6)})
DD.update({P_SV[d]: d for d in (4, 5, 6)})

VHS = ["-vhs"]
LP = ["-vhs", "-vhs-speed", "lp"]
EP = ["-vhs", "-vhs-speed", "ep"]
SV = ["-vhs-svideo", "1"]
PAL = ["-tvstd", "pal"]
LITE = ["-out-composite-lowpass", "0"]                                       # the lite output low-pass
NOLP = ["-out-composite-lowpass", "0", "-out-composite-lowpass-lite", "0"]   # none
FULL_ONLY = ["-out-composite-lowpass-lite", "0"]                             # the full one, its own switch off
CATV = ["-comp-catv"]
DROP = ["-chroma-dropout", "50000"]
NOBLEND = ["-vhs-chroma-vblend", "0"]
AMP30 = ["-subcarrier-amp", "30"]
P90 = ["-comp-phase", "90", "-comp-phase-offset", "1"]
P270 = ["-comp-phase", "270", "-comp-phase-offset", "3"]
N0, CN0, PN0 = ["-noise", "0"], ["-chroma-noise", "0"], ["-chroma-phase-noise", "0"]
HS_ON = ["-vhs-head-switching", "1"]
# the base switch set of each form (the launcher's own conditions: stream, stream_gen, stream_sv, fasta)
BASE = {P_SPEC: VHS, P_GEN[4]: VHS + LITE, P_GEN[5]: LP, P_GEN[6]: EP,
        P_SV[4]: VHS + SV, P_SV[5]: LP + SV, P_SV[6]: EP + SV, P_DIRECT: []}
TAG = {P_SPEC: "spec", P_GEN[4]: "gen4", P_GEN[5]: "gen5", P_GEN[6]: "gen6",
       P_SV[4]: "sv4", P_SV[5]: "sv5", P_SV[6]: "sv6", P_DIRECT: "direct"}

# The switches of the list, each with what it does to the parameters (tests/test_pipe422_forms_host.py looks for them in the
# rows by that, not by their spelling): (tag, flags, predicate over ntscsim_params).  The noises go off singly.
def _out_lp(p):
    return 2 if p.composite_out_chroma_lowpass else (1 if p.composite_out_chroma_lowpass_lite else 0)


def _others_on(p, *names):
    return not p.emulating_vhs or all(getattr(p, n) != 0 for n in names)


FULL_LP = ["-out-composite-lowpass", "1"]
LISTED = [
    ("pal", PAL, lambda p: p.tv_standard == 1),
    ("catv", CATV, lambda p: p.composite_preemphasis != 0 and p.composite_preemphasis_cut > 0),
    ("n0", N0, lambda p: p.video_noise == 0 and _others_on(p, "video_chroma_noise", "video_chroma_phase_noise")),
    ("cn0", CN0, lambda p: p.video_chroma_noise == 0 and _others_on(p, "video_noise", "video_chroma_phase_noise")),
    ("pn0", PN0, lambda p: p.video_chroma_phase_noise == 0 and _others_on(p, "video_noise", "video_chroma_noise")),
    ("p90", P90, lambda p: p.video_scanline_phase_shift == 90 and p.video_scanline_phase_shift_offset & 1),
    ("p270", P270, lambda p: p.video_scanline_phase_shift == 270 and p.video_scanline_phase_shift_offset & 1),
    ("amp30", AMP30, lambda p: p.subcarrier_amplitude == 30),
    ("drop", DROP, lambda p: p.video_chroma_loss == 50000),
    ("full", FULL_LP, lambda p: _out_lp(p) == 2),
    ("lite", LITE, lambda p: _out_lp(p) == 1),
    ("nolp", NOLP, lambda p: _out_lp(p) == 0),
    ("noblend", NOBLEND, lambda p: not p.vhs_chroma_vert_blend),
]
# which of them each form's conditions allow (the host test derives the same sets from launcher_name()): the preset
# instantiation keeps its identities (NTSC, SP, no pre-emphasis, the three noises on, the full output low-pass, even phase,
# amplitude 50), the no-VCR role form keeps fasta (NTSC, no pre-emphasis, luma noise on, even phase, amplitude 50), the
# run-time forms take everything
ALL_LISTED = tuple(t for t, _, _ in LISTED)
PERMITS = {f: ALL_LISTED for f in list(P_GEN.values()) + list(P_SV.values())}
PERMITS[P_SPEC] = ("drop", "full", "noblend")
PERMITS[P_DIRECT] = ("cn0", "pn0", "drop", "full", "lite", "nolp", "noblend")
# the switch sets a listed switch is added to: the form's base -- and, for k422_pipe<false,4>, whose base is the preset
# but for the lite low-pass, the preset but for the phase noise where the switch would put the full low-pass back
BASES = {f: [BASE[f]] for f in ROLE_NAMES}
BASES[P_GEN[4]] = [VHS + LITE, VHS + PN0]


def listed_flags(form, tag):
    """the switch set of a listed switch on a form"""
    sw = dict((t, f) for t, f, _ in LISTED)[tag]
    base = BASES[form][1 if form == P_GEN[4] and tag == "full" else 0]
    return sw + base if tag == "pal" else base + sw


# further switch sets per form: (tag, flags)
EXTRA = {
    P_SPEC: [("fullonly", VHS + FULL_ONLY), ("noise9", VHS + ["-noise", "9"]),
             ("phase0", VHS + ["-comp-phase", "0", "-comp-phase-offset", "1"])],
    P_GEN[4]: [("catv_noblend", VHS + CATV + NOBLEND), ("off1", VHS + ["-comp-phase-offset", "1"]), ("p90_even", VHS + ["-comp-phase", "90"])],
    P_GEN[5]: [], P_GEN[6]: [], P_SV[4]: [], P_SV[5]: [], P_SV[6]: [],
    P_DIRECT: [("cn8", ["-chroma-noise", "8"]), ("pn6", ["-chroma-phase-noise", "6"]), ("noise9_drop", ["-noise", "9"] + DROP),
               ("noise2", ["-noise", "2"])],
}
SWITCHES = {f: [(t, listed_flags(f, t)) for t in PERMITS[f]] + EXTRA[f] for f in ROLE_NAMES}
# switch sets that leave the role forms although the launch is short and aligned: (tag, flags, the one-wave name)
LEAVES = [("direct_n0", N0 + ["-chroma-noise", "8"], "k422_direct"), ("direct_catv", CATV, "k422_direct"), ("direct_p90", P90, "k422_direct"),
          ("direct_amp30", AMP30, "k422_direct"), ("direct_pal", PAL, "k422_direct"),
          ("recomb", VHS + ["-yc-recomb", "1"], "k422_process"), ("nocolor", ["-nocolor-subcarrier"], "k422_process"),
          ("noinlp", VHS + ["-in-composite-lowpass", "0"], "k422_process")]

SWITCH_W = (HB + 2, steady_first(6) + 4, fast_first(1) + 2)          # edge iterations only | steady for every DD | a guard-free group
PAL_W = (groups_edge(1, True), groups_edge(1, True) + 2)             # PAL's own group edge: 60 | 62
ROWS_W = steady_first(6) + 2                                         # the width of the row-packing rows: steady for every DD
HS_LINE = 24                                                         # the switch falls into frame row 4 + field


def hs_flags(w, kind):
    """-vhs-head-switching-point (this tool: the PHASE, ffmpeg_to_composite.cpp:1405) that puts the switch into frame row
    4 + field and displaces the rows below it forwards, backwards within W/10, or backwards beyond W/10.  The tool's own
    jitter of the phase (1/300 of a line, four rand() calls per field) stays on: the margins below are wider than it --
    but for "wide1" at widths where the jitter exceeds half a sample, which switches it off."""
    tw = w + w // 10
    hx = {"fwd": max(4, w // 18), "back": tw - max(2, w // 20), "wide": tw - (w // 10 + max(6, w // 5)),
          "wide1": tw - (w // 10 + 1)}[kind]
    assert (hx < tw // 2) == (kind == "fwd")
    quiet = ["-vhs-head-switching-noise-level", "0"] if kind == "wide1" and tw / 300.0 >= 0.4 else []
    return ["-vhs-head-switching-point", "%.8f" % ((HS_LINE * tw + hx + 0.5) / (tw * 262.5))] + quiet


HS_KINDS = ("fwd", "back", "wide", "wide1")


def hs_widths(dd):
    return (steady_first(dd) - 4, steady_first(dd) + 6, FULL)


def _rows():
    out = []

    def add(name, flags, w, h, n, kernel, fallback=None, layout="padded", source="inplace", share=False, hs=None):
        assert (kernel is None) != (fallback is None)
        out.append(Row(name, list(flags), w, h, n, layout, source, kernel, fallback, share, hs))

    for form in ROLE_NAMES:
        t, base, dd = TAG[form], BASE[form], DD[form]
        # ---- the widths of the loops: two fields of five rows, one workgroup
        for w in widths(dd):
            add("%s_w%d" % (t, w), base, w, 10, 2, form)
        # ---- rows through the workgroups
        for h, n in ((2, 2), (9, 2), (33, 2), (125, 3), (126, 3), (127, 3), (10, MAX_FIELDS)):
            add("%s_rows_%dx%d_n%d" % (t, ROWS_W, h, n), base, ROWS_W, h, n, form)
        add("%s_rows_%dx10_n%d" % (t, ROWS_W, MAX_FIELDS + 1), base, ROWS_W, 10, MAX_FIELDS + 1, None, ONE_WAVE[form])
        add("%s_full_%dx127_n3" % (t, FULL), base, FULL, 127, 3, form)
        add("%s_pair_%dx9" % (t, GATHER[2]), base, GATHER[2], 9, 2, form, share=True)
        add("%s_pair_%dx10_src" % (t, ROWS_W), base, ROWS_W, 10, 2, form, share=True, source="src")
        # ---- switch sets
        for tag, flags in SWITCHES[form]:
            for w in SWITCH_W + (PAL_W if tag == "pal" else ()):
                add("%s_%s_w%d" % (t, tag, w), flags, w, 10, 2, form)
        # ---- head switching: the gather role
        hs_base = base + (HS_ON if form == P_DIRECT else [])
        for kind in HS_KINDS:
            for w in hs_widths(dd):
                add("%s_hs_%s_w%d" % (t, kind, w), hs_base + hs_flags(w, kind), w, 33, 2, form, hs=kind)
        # ---- layouts
        for w in (BURST, 2 * BURST):
            add("%s_tight_w%d" % (t, w), base, w, 10, 2, form, layout="tight")
        add("%s_tight_hs_w%d" % (t, 2 * BURST), hs_base + hs_flags(2 * BURST, "wide"), 2 * BURST, 33, 2, form, layout="tight", hs="wide")
        # (without aligned rows: the four-sweep form with scalar row accesses, the twelve sweeps for S-Video out, the general
        #  sweep A of the no-VCR form)
        off = "k422_direct" if form == P_DIRECT else "k422_process" if form in P_SV.values() else "k422_fused<false,false,4>"
        add("%s_odd_w%d" % (t, ROWS_W), base, ROWS_W, 10, 2, None, off, layout="odd")
        add("%s_oddchroma_w%d" % (t, 2 * BURST), base, 2 * BURST, 10, 2, None, off, layout="odd-chroma")
        # ---- sources through k422_render
        for w in (HB + 2, GATHER[2]):
            add("%s_src_w%d" % (t, w), base, w, 10, 2, form, source="src")
    # one 4:2:0 and one interlaced source per family of kernels, a tight row behind k422_render
    for form in (P_SPEC, P_GEN[6], P_SV[5], P_DIRECT):
        t = TAG[form]
        add("%s_src420_w%d" % (t, ROWS_W), BASE[form], ROWS_W, 12, 2, form, source="src420")
        add("%s_srcil_w%d" % (t, ROWS_W), BASE[form], ROWS_W, 12, 2, form, source="src-il")
        add("%s_src_tight_w%d" % (t, BURST), BASE[form], BURST, 10, 2, form, source="src", layout="tight")
    for tag, flags, name in LEAVES:
        add("leave_%s_w%d" % (tag, ROWS_W), flags, ROWS_W, 10, 2, None, name)
    return out


ROWS = _rows()
assert len({r.id for r in ROWS}) == len(ROWS)
BY_ID = {r.id: r for r in ROWS}


def _sync():
    """ntscsim_field422() call after call: below the steady threshold, at it, and full width"""
    out = []
    for form in ROLE_NAMES:
        s = steady_first(DD[form])
        for w, h in ((s - 2, 12), (s, 12), (FULL, 34)):
            out.append(Sync("%s_sync_w%d" % (TAG[form], w), list(BASE[form]), w, h, form))
    return out


SYNC = _sync()
SYNC_OTHER = (GATHER[2], 9)          # the second geometry of a context, run between two visits of the row's own


# ------------------------------------------------------------------------------------------------ the launcher's rule
def launcher_name(p, aligned, n, latency=True):
    """launch422()'s choice (csrc/ntscsim_hip.hip) in terms of the parameters: (role-kernel name or None, one-wave name)"""
    ntsc = p.tv_standard == 0
    pre_on = p.composite_preemphasis != 0 and p.composite_preemphasis_cut > 0
    out_lp = 2 if p.composite_out_chroma_lowpass else (1 if p.composite_out_chroma_lowpass_lite else 0)
    cdelay = {0: 4, 1: 5, 2: 6}[p.output_vhs_tape_speed]
    family = (not p.nocolor_subcarrier and p.composite_in_chroma_lowpass and not p.nocolor_subcarrier_after_yc_sep and
              p.video_yc_recombine == 0)
    vhs, sv = bool(p.emulating_vhs), bool(p.vhs_svideo_out)
    fused, direct, fused_sv = family and vhs and not sv, family and not vhs, family and vhs and sv
    mode, off = p.video_scanline_phase_shift, p.video_scanline_phase_shift_offset
    even = (not off & 1) if mode == 180 else mode not in (90, 270)
    spec = (ntsc and not pre_on and p.video_noise and p.video_chroma_noise and p.video_chroma_phase_noise and out_lp == 2 and
            cdelay == 4 and aligned)
    stream = spec and even and p.subcarrier_amplitude == 50 and p.subcarrier_amplitude_back == 50
    stream_gen = fused and not stream and aligned
    fasta = direct and ntsc and not pre_on and p.video_noise and even and p.subcarrier_amplitude == 50 and aligned
    stream_sv = fused_sv and aligned
    one = ("k422_direct_fast" if fasta else "k422_direct") if direct else \
        "k422_fused_sv<%d>" % cdelay if stream_sv else "k422_process" if not fused else \
        "k422_fused<true,true,4>" if stream else "k422_fused<false,true,%d>" % cdelay if stream_gen else \
        "k422_fused<true,false,4>" if spec else "k422_fused<false,false,4>"
    short = latency and n <= MAX_FIELDS
    if short and direct and fasta:
        return P_DIRECT, one
    if short and ((fused and stream) or stream_gen or stream_sv):
        return (P_SPEC if fused and stream else P_SV[cdelay] if stream_sv else P_GEN[cdelay]), one
    return None, one


# ------------------------------------------------------------------------------------------------ frames
def linesizes(w, layout):
    up = lambda v, a: (v + a - 1) // a * a
    if layout == "tight":
        return [w, w // 2, w // 2]
    if layout == "odd":
        return [w + 3, w // 2 + 3, w // 2 + 3]
    if layout == "odd-chroma":
        c = w // 2 + 4 + (1 if (w // 2 + 4) % 8 == 0 else 0)
        return [up(w + 2, 16), c, c]
    if layout == "odd-luma":
        return [w + 3, up(w // 2 + 2, 8), up(w // 2 + 2, 8)]
    return [up(w + 2, 16), up(w // 2 + 2, 8), up(w // 2 + 2, 8)]


def aligned(w, layout):
    ls = linesizes(w, layout)
    return ls[0] % 16 == 0 and ls[1] % 8 == 0 and ls[2] % 8 == 0


GUARD = 64          # bytes between two frames of a launch's buffer (and behind the last one)


def plane_offsets(w, h, layout):
    """where the three planes start in a frame's bytes: back to back -- behind an unaligned luma plane ("odd-luma") at the
    next multiple of 16, so that the chroma rows are aligned on their own"""
    ls = linesizes(w, layout)
    o1 = ls[0] * h
    if layout == "odd-luma":
        o1 = (o1 + 15) // 16 * 16
    return [0, o1, o1 + ls[1] * h]


def frame_bytes(w, h, layout):
    ls = linesizes(w, layout)
    return (plane_offsets(w, h, layout)[2] + ls[2] * h + GUARD + 63) // 64 * 64


def frame_at(buf, k, w, h, layout):
    """frame k of a launch's buffer as a Yuv422 (tests/_libs.py) over a VIEW of it"""
    import _libs as L
    nb = frame_bytes(w, h, layout)
    f = L.Yuv422.__new__(L.Yuv422)
    f.w, f.h, f.ls = w, h, linesizes(w, layout)
    f.off = plane_offsets(w, h, layout)
    f.buf = buf[k * nb:(k + 1) * nb]
    return f


def fill(buf, frames, seed, bars_every=0):
    """noise in every byte (padding and guards included), legal pixels in the pictures; every bars_every-th frame bars"""
    r = np.random.RandomState(seed)
    buf[:] = r.randint(0, 256, size=buf.size, dtype=np.uint8)
    for j, f in enumerate(frames):
        if bars_every and j % bars_every == bars_every - 1:
            x = np.arange(f.w)
            f.pix(0)[:] = (16 + 27 * ((8 * ((x + 3 * j) % f.w)) // f.w)).astype(np.uint8)
            f.pix(1)[:] = (40 + 23 * ((8 * ((2 * x[:f.w // 2] + 3 * j) % f.w)) // f.w)).astype(np.uint8)
            f.pix(2)[:] = (220 - 21 * ((8 * ((2 * x[:f.w // 2] + 3 * j) % f.w)) // f.w)).astype(np.uint8)
        else:
            f.pix(0)[:] = r.randint(16, 236, size=(f.h, f.w), dtype=np.uint8)
            f.pix(1)[:] = r.randint(16, 241, size=(f.h, f.w // 2), dtype=np.uint8)
            f.pix(2)[:] = r.randint(16, 241, size=(f.h, f.w // 2), dtype=np.uint8)


def margin_mask(frames, total):
    """tests/test_variant422.py: last_row_margin_mask, over a launch's buffer.  True where the product must equal the oracle's
    MEMORY mode: everything, but for the right margin of a frame's LAST luma row and the chroma rows beside it when the two
    bytes behind that row lie outside the luma plane (linesize < W + 2)"""
    m = np.ones(total, bool)
    for j, f in enumerate(frames):
        if f.ls[0] >= f.w + 2:
            continue
        base = j * f.buf.size
        for i, marg in ((0, 24), (1, 14), (2, 14)):
            width = f.w if i == 0 else f.w // 2
            a = base + f.off[i] + (f.h - 1) * f.ls[i]
            m[a + max(0, width - marg):a + width] = False
    return m


SRC_FLAGS = {"inplace": None, "src": 0, "src420": 4, "src-il": 1 | 2 | 8}       # NTSCSIM_422_*: INTERLACED 1, TFF 2, SRC420 4, SECOND 8


def params(row):
    import _libs as L
    return L.make_params_tocomp(row.flags)


Case = namedtuple("Case", "init exp frames srcbuf srcs jobs mask rng_pos calls shifts")


def _seed(row):
    return int.from_bytes(row.id.encode()[-6:], "little") % 100003 + row.w


def hs_shifts(p, g, w, h, field):
    """The displacement of every row of one field (ffmpeg_to_composite.cpp:669-732) from the state g of the rand() stream
    in front of the field: the luma noise takes W draws per row first, the jitter of the switch four"""
    import ctypes as C
    import math
    import _libs as L
    o = L.oracle()
    g = type(g).from_buffer_copy(g)
    rows = len(range(field, h, 2))
    if not p.vhs_head_switching:
        return [0] * rows
    if p.video_noise:
        o.ntsc_oracle_rng_discard(C.byref(g), w * rows)
    noise = 0.0
    if p.vhs_head_switching_phase_noise != 0:
        u = 1
        for _ in range(4):
            u = (u * o.ntsc_oracle_rng_next(C.byref(g))) & 0xFFFFFFFF
        noise = (float(u % 2000000000) / 1000000000 - 1.0) * p.vhs_head_switching_phase_noise
    tw = w + w // 10
    t = tw * (262.5 if p.tv_standard == 0 else 312.5)
    pp = int(math.fmod(p.vhs_head_switching_phase + noise, 1.0) * t)
    hx = pp % tw
    y = (pp // tw) * 2 + field - ((262 - 240) * 2 if p.tv_standard == 0 else (312 - 288) * 2)
    ishif = hx - tw if hx >= tw // 2 else hx
    got, shif, shy = {}, 0, 0
    while y < h:
        if y >= 0:
            got[y] = shif
        shif = ishif if shy == 0 else int(shif * 7 / 8)
        y += 2
        shy += 1
    return [got.get(y, 0) for y in range(field, h, 2)]


@functools.lru_cache(maxsize=2)
def case(row_id):
    """The launch of a row and what the oracle makes of it: one buffer with all frames (guards between them), the oracle in
    MEMORY mode field after field, the descriptors as (frame index, source index or None, field, fieldno, flags)"""
    import ctypes as C
    import _libs as L
    row = BY_ID[row_id]
    p = params(row)
    w, h, n = row.w, row.h, row.n
    nfr = 1 if row.share else n
    init = np.empty(nfr * frame_bytes(w, h, row.layout), np.uint8)
    frames = [frame_at(init, k, w, h, row.layout) for k in range(nfr)]
    fill(init, frames, _seed(row), bars_every=5)
    srcbuf, srcs = None, []
    fl = SRC_FLAGS[row.source]
    if fl is not None:
        nsrc = (n + 1) // 2
        srcbuf = np.empty(nsrc * frame_bytes(w, h, "padded"), np.uint8)
        srcs = [frame_at(srcbuf, k, w, h, "padded") for k in range(nsrc)]
        fill(srcbuf, srcs, _seed(row) + 1)
    exp = init.copy()
    eframes = [frame_at(exp, k, w, h, row.layout) for k in range(nfr)]
    o = L.TocompOracleStream(p, L.OOB_MEMORY)
    lib = L.product()
    jobs, calls, shifts = [], 0, []
    for k in range(n):
        field = (k & 1) ^ 1
        fi = 0 if row.share else k
        if fl is not None:
            L.tocomp_oracle_render_field(eframes[fi], srcs[k // 2], int(bool(fl & 4)), int(bool(fl & 1)), int(bool(fl & 2)),
                                         int(bool(fl & 8)), field)
        shifts.append(hs_shifts(p, o.g, w, h, field))
        o.process(eframes[fi], field, k)
        calls += lib.ntscsim_rng_calls_per_field_422(C.byref(p), w, h, field)
        jobs.append((fi, k // 2 if fl is not None else None, field, k, fl or 0))
    for a in (init, exp) + ((srcbuf,) if srcbuf is not None else ()):
        a.setflags(write=False)
    return Case(init, exp, frames, srcbuf, srcs, jobs, margin_mask(frames, init.size), o.rng_pos, calls, shifts)


def string_literals(text):
    """the string literals of a C++ source (none of the ones looked for holds an escape)"""
    return re.findall(r'"([^"\\\n]*)"', text)

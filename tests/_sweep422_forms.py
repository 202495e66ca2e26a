"""The table of the YUV422P tool's SWEEP kernels: the twelve-sweep body k422_process (csrc/ntsc422_kernels.hip:
process422_body, which as k422_mixed_process also runs every set of ntscsim_mixed_fields422_device), the four-sweep forms
k422_fused<false,false,4> and k422_fused<true,false,4> and the no-VCR form k422_direct = k422_short<false>
(csrc/ntsc422_fused.hip) -- every name launch422() (csrc/ntscsim_hip.hip) can note for a launch in the throughput form that
is neither a role kernel nor a streamed one (those are tests/_pipe422_forms.py's), at the widths of the kernels' own loop
conditions, on every combination of luma and chroma row alignment, with the row packings, sources and switch sets that
reach it.  Shared by tests/test_sweep422_forms_host.py (CPU: closure over the launcher's names, coverage of every
condition, the oracle's properties of the rows) and tests/test_sweep422_forms_gpu.py (equality with the oracle, row by
row).  Test infrastructure only; no GPU import.

A row: (id, fam, reach, flags, bits, w, h, n, layout, source, kernel, share, hs)
  fam       what the row is in the table for: "w" (the even-width sweep), "edge" (the widths of the conditions on the
            other layouts and reaches), "rows" (row packings), "sw:<tag>" (a listed switch), "hs", "src", "full"
  reach     how the form is reached (REACHES): the dispatcher's own choice for the switch set and the layout, or
  bits      the argument of ntscsim_debug_no_fast_decode(): 1 keeps the twelve sweeps, 2 keeps the forms without
            identities (four sweeps, k422_direct), 4 keeps the four-sweep form of the switch set
  layout    tests/_pipe422_forms.py's four and "odd-luma"; (luma rows 16-byte aligned, chroma rows 8-byte aligned) is
            padded (1, 1), odd (0, 0), odd-chroma (1, 0), odd-luma (0, 1), tight (1, 1) at W = 0 mod 16 and (0, 0) else
  source    "inplace", "src" / "src420" / "src-il" (through k422_render), "bkey" (in place behind k422_bkey)
  kernel    the ONE name ntscsim_debug_last_kernels() must report among the k422_fused*, k422_process and k422_direct*
            names
  share     both fields of ONE frame in one launch (n = 2)
  hs        None, or the kind of head-switch displacement the row claims (tests/_pipe422_forms.py)
Field k of a launch has parity (k & 1) ^ 1 and field number k, as the tool's loop counts them.
"""
import functools
from collections import OrderedDict, namedtuple

import numpy as np

import _pipe422_forms as T

Row = namedtuple("Row", "id fam reach flags bits w h n layout source kernel share hs")
Reach = namedtuple("Reach", "tag form flags bits layouts")
Mixed = namedtuple("Mixed", "id w h layout")

# ------------------------------------------------------------------------------------------------ the kernels' constants
# (tests/test_sweep422_forms_host.py reads the same numbers out of the two .hip files)
VEC_Y, VEC_C = 16, 8        # bytes per vector in-copy of k422_process: `x0 + 16 <= W`, `c0 + 8 <= W2`
BURST_Y, BURST_C = 64, 32   # bytes per burst of its out-copy: `x0 + 64 <= W`, `c0 + 32 <= W2`
BK = 8                      # samples per block of Reader422 / SWEEP_BEGIN and per step of k422_process's gather
HB = 16                     # samples per step of the gather in the fused file
SB = 16                     # samples per block of sweep_blocks<4> (B = 4 * NWB), which runs over W + 2
GROUP = 32                  # chroma inputs per group of sweep A
WG_ROWS = 63                # rows per workgroup; lane 0 is the halo lane
DELAYS = {"sp": 4, "lp": 5, "ep": 6}      # the VCR's chroma delay per tape speed (wu[2], wu[1], wu[0])
LP_DELAYS = (1, 2, 4)       # the output low-passes: lite, full U, full V (NTSC); Packer422::finish(W2 - delay)
MIN_W = 16                  # the smallest width the call accepts
MARGIN_Y, MARGIN_C = 24, 14  # tests/test_variant422.py: what a tight frame's last row may differ in


# ---- the conditions, one function each (w: the luma width; the chroma width is w // 2)
def finish_class(n):
    """Packer422::finish(n): the bytes of the partial last word, `n & 3` (n = W, W/2, W/2 - delay)"""
    return n & 3


def ragged(n, block=BK):
    """SWEEP_BEGIN over N = W, W/2, W/2 + d and the gathers over W: the samples of the ragged last block"""
    return n % block


def raw_window(w, d):
    """`xo < W2 - d`: the outputs of the VCR's chroma low-pass that are filtered; the d behind them take the raw tap"""
    return w // 2 - d


def vec_tail(w):
    """the scalar tail behind the vector in-copy (`x0 + 16 <= W`; `c0 + 8 <= W2` is the same class)"""
    return w % VEC_Y != 0


def bursts(w):
    """trips of `x0 + 64 <= W` (and of `c0 + 32 <= W2`)"""
    return w // BURST_Y


def pieces(w):
    """trips of `x0 + 16 <= W` behind the bursts (and of `c0 + 8 <= W2`)"""
    return w % BURST_Y // VEC_Y


def blocks_ragged(w):
    """sweep_blocks<4>(R.Y, W + 2): does the second copy of the body run"""
    return (w + 2) % SB != 0


def byte_block(w):
    """load_block16 / load_block8, `al && x0 + 16 <= n`: a block that straddles the row end takes the byte path"""
    return w % VEC_Y != 0


def gather_class(w):
    """tw = W + W / 10 against the gather's steps: (W / 10, samples of the ragged step of 8, of 16)"""
    return (w // 10, w % BK, w % HB)


a_groups, groups_edge = T.a_groups, T.groups_edge          # trips of `for (g0 = 0; g0 < W2 + D; g0 += 32)`

EVEN = tuple(range(MIN_W, 148, 2))                 # every residue of W mod 64 and of W/2 mod 32
BIG = (190, 192, 194, 254, 256, 258, 718, 720, 722)
GATHER_W = (16, 18, 20, 30, 40)                    # W / 10 = 1, 1, 2, 3, 4 against the steps of 8 and 16
FULL = 720


def widths():
    """the width sweep of every form and chroma delay"""
    return EVEN + BIG


def edge_widths():
    """both sides of every condition above, for the layouts and reaches beside the sweep"""
    ws = {MIN_W, MIN_W + 2, MIN_W + 4, MIN_W + 6}                          # W/2 mod 4 = 0, 1, 2, 3; the windows of 2 to 4
    ws.update((2 * VEC_Y - 2, 2 * VEC_Y, 2 * VEC_Y + 2, 3 * VEC_Y - 2))   # vector tails: W mod 16 = 14, 0, 2, 14
    for k in (1, 2):
        ws.update((k * BURST_Y - 2, k * BURST_Y, k * BURST_Y + 2))        # 0 | 1 | 2 bursts
    ws.update(BURST_Y + k * VEC_Y for k in range(4))                      # 0 .. 3 pieces behind a burst
    for pal in (False, True):
        for k in (1, 2):
            ws.update((groups_edge(k, pal), groups_edge(k, pal) + 2))     # 1 | 2 | 3 groups of sweep A
    ws.update(GATHER_W)
    ws.add(FULL)
    return tuple(sorted(ws))


def small_h(w, flip=0):
    """H = 5 and H = 6 in turn: each field parity owns the frame's last row once"""
    return 5 + ((w // 2 + flip) & 1)


# ------------------------------------------------------------------------------------------------ the names and switch sets
PROC = "k422_process"
F4 = "k422_fused<false,false,4>"
S4 = "k422_fused<true,false,4>"
DIRECT = "k422_direct"
FORMS = (PROC, F4, S4, DIRECT)
STREAMED = ("k422_fused<true,true,4>", "k422_fused<false,true,4>", "k422_fused<false,true,5>", "k422_fused<false,true,6>",
            "k422_fused_sv<4>", "k422_fused_sv<5>", "k422_fused_sv<6>", "k422_direct_fast")
MIXED_NAME = "k422_mixed_process"

VHS, LP, EP, SV, PAL = T.VHS, T.LP, T.EP, T.SV, T.PAL
PALVHS = PAL + VHS
RECOMB1, RECOMB2 = ["-yc-recomb", "1"], ["-yc-recomb", "2"]
NOCOLOR, AFTER, NOINLP = ["-nocolor-subcarrier"], ["-nocolor-subcarrier-after-yc-sep"], ["-in-composite-lowpass", "0"]
CN8PN6 = ["-chroma-noise", "8", "-chroma-phase-noise", "6"]
CN8 = ["-chroma-noise", "8"]                       # (beside `-noise 0` without the VCR: the launch still draws)
OFF1 = ["-comp-phase-offset", "1"]
BKEY = ["-bkey-feedback", "40"]
ANY = ("padded", "tight", "odd", "odd-chroma", "odd-luma")
UNALIGNED = ("odd", "odd-chroma", "odd-luma")          # (and tight rows at W != 0 mod 16)

# how each form is reached: the dispatcher's own choice (bits 0) or a debug bit; `layouts`: where the reach holds
REACHES = [
    Reach("recomb1", PROC, VHS + RECOMB1, 0, ANY), Reach("recomb2", PROC, RECOMB2, 0, ANY),
    Reach("nocolor", PROC, NOCOLOR + CN8PN6, 0, ANY), Reach("nocolor_q", PROC, NOCOLOR + T.CN0 + T.PN0, 0, ANY),
    Reach("aftersep", PROC, VHS + AFTER, 0, ANY), Reach("noinlp", PROC, VHS + NOINLP, 0, ANY),
    Reach("sv_sp", PROC, VHS + SV, 0, UNALIGNED), Reach("sv_lp", PROC, LP + SV, 0, UNALIGNED), Reach("sv_ep", PROC, EP + SV, 0, UNALIGNED),
    Reach("b1_sp", PROC, VHS, 1, ANY), Reach("b1_lp", PROC, LP, 1, ANY), Reach("b1_ep", PROC, EP, 1, ANY),
    Reach("b1_pal", PROC, PALVHS, 1, ANY), Reach("b1_direct", PROC, [], 1, ANY), Reach("b1_sv", PROC, VHS + SV, 1, ANY),
    Reach("f4_sp", F4, VHS, 0, UNALIGNED), Reach("f4_lp", F4, LP, 0, UNALIGNED), Reach("f4_ep", F4, EP, 0, UNALIGNED),
    Reach("f4_pal", F4, PALVHS, 0, UNALIGNED),
    Reach("f4b2_sp", F4, VHS, 2, ANY), Reach("f4b2_lp", F4, LP, 2, ANY), Reach("f4b2_ep", F4, EP, 2, ANY), Reach("f4b2_pal", F4, PALVHS, 2, ANY),
    Reach("f4b4_lp", F4, LP, 4, ANY), Reach("f4b4_ep", F4, EP, 4, ANY), Reach("f4b4_lite", F4, VHS + T.LITE, 4, ANY),
    Reach("s4", S4, VHS, 4, ("padded", "tight")),
    Reach("d_own", DIRECT, [], 0, UNALIGNED), Reach("d_pal", DIRECT, PAL, 0, ANY), Reach("d_catv", DIRECT, T.CATV, 0, ANY),
    Reach("d_n0", DIRECT, T.N0 + CN8, 0, ANY), Reach("d_p90", DIRECT, T.P90, 0, ANY), Reach("d_off1", DIRECT, OFF1, 0, ANY),
    Reach("d_b2", DIRECT, [], 2, ANY),
    # the lite output low-pass (delay 1: chroma_lp_plain422 and its finish(W2 - 1), FrameSink mode 1), no switch set's default
    Reach("b1_lite", PROC, VHS + T.LITE, 1, ANY), Reach("b1_dlite", PROC, T.LITE, 1, ANY), Reach("f4_lite", F4, VHS + T.LITE, 0, UNALIGNED),
    Reach("d_lite", DIRECT, T.LITE, 0, UNALIGNED), Reach("d_lite_b2", DIRECT, T.LITE, 2, ANY),
]
REACH = {r.tag: r for r in REACHES}
assert len(REACH) == len(REACHES)

# the width sweep: per form and chroma delay (PAL: the delay-2 input filter, no blend) one reach on aligned rows and one on
# unaligned rows -- the bit 1 rows are the only way the aligned vector in-copy and the burst out-copy of k422_process run
SWEEPS = [("b1_sp", "padded"), ("b1_lp", "padded"), ("b1_ep", "padded"), ("b1_pal", "padded"),
          ("b1_sp", "odd"), ("b1_lp", "odd"), ("b1_ep", "odd"), ("b1_pal", "odd"),
          ("f4b2_sp", "padded"), ("f4b2_lp", "padded"), ("f4b2_ep", "padded"), ("f4b2_pal", "padded"),
          ("f4_sp", "odd"), ("f4_lp", "odd"), ("f4_ep", "odd"), ("f4_pal", "odd"),
          ("s4", "padded"),
          ("d_b2", "padded"), ("d_own", "odd"), ("d_pal", "padded"), ("d_pal", "odd")]
# the conditions' widths on the remaining alignment combinations, per form and delay ...
EDGE_LAYOUTS = [("b1_sp", "odd-chroma"), ("b1_sp", "odd-luma"), ("b1_sp", "tight"), ("b1_lp", "odd-chroma"), ("b1_lp", "odd-luma"),
                ("b1_lp", "tight"), ("b1_ep", "odd-chroma"), ("b1_ep", "odd-luma"), ("b1_ep", "tight"), ("b1_pal", "odd-chroma"),
                ("b1_pal", "odd-luma"), ("b1_pal", "tight"),
                ("f4_sp", "odd-chroma"), ("f4_sp", "odd-luma"), ("f4b2_sp", "tight"), ("f4_lp", "odd-chroma"), ("f4_lp", "odd-luma"),
                ("f4b2_lp", "tight"), ("f4_ep", "odd-chroma"), ("f4_ep", "odd-luma"), ("f4b2_ep", "tight"), ("f4_pal", "odd-chroma"),
                ("f4_pal", "odd-luma"), ("f4b2_pal", "tight"),
                ("s4", "tight"),
                ("d_own", "odd-chroma"), ("d_own", "odd-luma"), ("d_b2", "tight"), ("d_pal", "odd-chroma"), ("d_pal", "odd-luma"),
                ("d_pal", "tight")]
# ... and on aligned and unaligned rows for the reaches beside the sweep
EDGE_REACHES = [(t, lay) for t in ("recomb1", "recomb2", "nocolor", "nocolor_q", "aftersep", "noinlp", "b1_direct", "b1_sv",
                                          "b1_lite", "b1_dlite")
                for lay in ("padded", "odd")] + \
               [(t, lay) for t in ("sv_sp", "sv_lp", "sv_ep") for lay in ("odd", "odd-chroma", "odd-luma")] + \
               [(t, "padded") for t in ("f4b4_lp", "f4b4_ep", "f4b4_lite", "d_catv", "d_n0", "d_p90", "d_off1", "d_lite_b2")] + \
               [(t, "odd") for t in ("f4_lite", "d_lite")]

# The switches of the list, each with what it does to the parameters (the host test looks for them in the rows by that, not
# by their spelling): tests/_pipe422_forms.py's, and three more
AMP1 = ["-subcarrier-amp", "1"]
CATV3 = ["-comp-catv3"]
P0 = ["-comp-phase", "0", "-comp-phase-offset", "1"]
LISTED = list(T.LISTED) + [
    ("amp1", AMP1, lambda p: p.subcarrier_amplitude == 1),
    ("catv3", CATV3, lambda p: p.composite_preemphasis == 4 and p.video_chroma_phase_noise == 6),
    ("p0", P0, lambda p: p.video_scanline_phase_shift == 0 and p.video_scanline_phase_shift_offset & 1),
]
LISTED[1] = ("catv", T.CATV, lambda p: p.composite_preemphasis == 1.5 and p.composite_preemphasis_cut > 0)
ALL_LISTED = tuple(t for t, _, _ in LISTED)
# the reach each form's switch rows stand on, and which of the switches its launcher rule allows there (the host test
# derives the same sets from launcher_rule()): the twelve sweeps and the forms without identities take everything, the
# preset instantiation keeps its identities but for the scanline phase and the amplitude, which only its streamed pass uses
SWITCH_REACH = ("b1_sp", "b1_direct", "f4b2_sp", "s4", "d_b2")
PERMITS = {t: ALL_LISTED for t in SWITCH_REACH}
PERMITS["s4"] = ("p90", "p270", "amp30", "drop", "full", "noblend", "amp1", "p0")
SWITCH_W = (MIN_W + 2, BURST_Y + 6, FULL)          # below 32 | 32 to 146 | 720; W/2 = 9, 35, 360
DROP_H, HS_H = 12, 12


def listed_flags(reach, tag):
    """the switch set of a listed switch on a reach (the tool reads its switches in order: a preset goes first)"""
    sw = dict((t, f) for t, f, _ in LISTED)[tag]
    base = REACH[reach].flags
    if tag == "n0" and "-vhs" not in base:
        sw = sw + CN8
    return sw + base if tag == "pal" else base + sw


HS_KINDS = T.HS_KINDS
HS_REACH = ("b1_sp", "f4b2_sp", "f4_sp", "s4", "d_b2", "d_own")
HS_W = GATHER_W + (BURST_Y + 6, FULL)


def hs_flags(w, kind):
    """tests/_pipe422_forms.py: hs_flags, with a displacement "back" that stays within W / 10 below 40 as well"""
    tw = w + w // 10
    if kind != "back":
        return T.hs_flags(w, kind)
    hx = tw - min(w // 10, max(2, w // 20))
    assert hx >= tw // 2
    return ["-vhs-head-switching-point", "%.8f" % ((T.HS_LINE * tw + hx + 0.5) / (tw * 262.5))]


ROWS_W = MIN_W + 6                                  # the width of the row-packing rows: W/2 = 11
PACK_H = (124, 125, 127, 130)                       # Lslot 62, 63, 64, 65
PACK_REACH = (("b1_sp", "padded"), ("recomb1", "odd"), ("f4b2_sp", "padded"), ("f4_sp", "odd"), ("s4", "padded"), ("d_b2", "padded"),
              ("d_own", "odd"))
SRC_REACH = (("b1_sp", "padded"), ("f4_sp", "odd"), ("s4", "padded"), ("d_b2", "padded"))
SRC_W = (MIN_W + 2, BURST_Y + 6)


def _rows():
    out = []

    def add(fam, reach, w, h, n, layout, flags=None, source="inplace", share=False, hs=None, tag=""):
        r = REACH[reach]
        assert layout in r.layouts or (layout == "tight" and "odd" in r.layouts and not T.aligned(w, "tight")), (reach, layout)
        name = "%s_%s%s_%s_w%dx%d_n%d%s%s" % (reach, fam.replace(":", "_"), tag, layout, w, h, n, "_" + source if source != "inplace" else "",
                                              "_pair" if share else "")
        out.append(Row(name, fam, reach, list(r.flags if flags is None else flags), r.bits, w, h, n, layout, source, r.form, share, hs))

    # ---- the widths of the loops: three fields of five or six rows, one workgroup
    for k, (reach, layout) in enumerate(SWEEPS):
        for w in widths():
            add("w", reach, w, small_h(w, k), 3, layout)
    for reach, layout in EDGE_LAYOUTS + EDGE_REACHES:
        for w in edge_widths():
            if layout == "tight":
                if "tight" not in REACH[reach].layouts and T.aligned(w, "tight"):
                    continue
                if reach == "s4" and not T.aligned(w, "tight"):
                    continue
                for h in (5, 6):                   # (the last row's two bytes lie outside the plane: both parities own it)
                    add("edge", reach, w, h, 3, layout)
            else:
                add("edge", reach, w, small_h(w), 3, layout)
    # ---- rows through the workgroups: fields that start on every lane class, the halo lane across a workgroup's edge
    for reach, layout in PACK_REACH:
        for h in PACK_H:
            for n in (1, 2, 3):
                add("rows", reach, ROWS_W, h, n, layout)
    for reach in ("b1_sp", "f4b2_sp", "s4", "d_b2"):
        for h in (6, 126, 127):
            add("rows", reach, ROWS_W, h, 2, "padded", share=True)
        add("full", reach, FULL, 127, 3, "padded")
    # ---- switch sets
    for reach in SWITCH_REACH:
        for tag in PERMITS[reach]:
            for w in SWITCH_W:
                add("sw:" + tag, reach, w, DROP_H if tag == "drop" else small_h(w), 3, "padded", flags=listed_flags(reach, tag))
    # ---- head switching in the frame: the gather
    for reach in HS_REACH:
        base = REACH[reach].flags + (T.HS_ON if REACH[reach].form == DIRECT else [])
        for kind in HS_KINDS:
            for w in HS_W:
                add("hs", reach, w, HS_H, 2, "odd" if "padded" not in REACH[reach].layouts else "padded", flags=base + hs_flags(w, kind),
                    hs=kind, tag="_" + kind)
    # ---- sources through k422_render, one black-key row per form
    for reach, layout in SRC_REACH:
        for source in ("src", "src420", "src-il"):
            for w in SRC_W:
                add("src", reach, w, 12, 2, layout, source=source)
        add("src", reach, BURST_Y + 6, 12, 2, layout, flags=REACH[reach].flags + BKEY, source="bkey")
    return out


ROWS = _rows()
assert len({r.id for r in ROWS}) == len(ROWS)
BY_ID = {r.id: r for r in ROWS}

GROUP_ROWS = 50          # launches (each with its companion) per GPU test


def _groups():
    """The rows of a test: one reach and one family of the table, at most GROUP_ROWS of them.  The rows of one switch set
    follow each other and share a context; the width families hold one switch set per test, the others one per switch, head
    switch point or source kind"""
    by = OrderedDict()
    for r in ROWS:
        by.setdefault((r.reach, r.fam.split(":")[0]), []).append(r)
    out = OrderedDict()
    for (reach, fam), rows in by.items():
        for k in range(0, len(rows), GROUP_ROWS):
            out["%s_%s_%d" % (reach, fam, k // GROUP_ROWS + 1)] = rows[k:k + GROUP_ROWS]
    return out


GROUPS = _groups()

# ------------------------------------------------------------------------------------------------ the mixed call
# the sets of one call: each owns two fields (one of each parity), no two neighbouring descriptors name one set
MIXED_SETS = [("sp", VHS), ("lp", LP), ("ep", EP), ("palvhs", PALVHS), ("svideo", VHS + SV), ("default", []),
              ("recomb1", VHS + RECOMB1), ("nocolor", NOCOLOR + CN8PN6), ("aftersep", VHS + AFTER), ("noinlp", VHS + NOINLP)]
MIXED_W = tuple(range(MIN_W, 48, 2)) + (BURST_Y, BURST_Y + 2, FULL)
MIXED_TALL = 65          # Lslot 33: a set's two fields are 66 rows, its group's field edge (33) and end (66) inside workgroups


def mixed_h(w):
    """a group (the fields of one set) counts its workgroups of 63 rows from its own first row: small frames put the field
    edges of every group inside its one workgroup, the tall ones a field edge inside the first and the group's end inside
    the second, behind a halo row"""
    return MIXED_TALL if w in (BURST_Y, BURST_Y + 2) else small_h(w)


MIXED_LAYOUTS = ("padded", "tight", "odd")
MIXED = [Mixed("mixed_%s_w%d" % (lay, w), w, mixed_h(w), lay) for lay in MIXED_LAYOUTS for w in MIXED_W]


# ------------------------------------------------------------------------------------------------ the launcher's rule
def delay_key(p):
    """the class of a switch set for the width sweep: the VCR's chroma delay, PAL, or no VCR"""
    if p.tv_standard == 1:
        return "pal"
    return ("sp", "lp", "ep")[p.output_vhs_tape_speed] if p.emulating_vhs else "novcr"


def launcher_rule(p, al_y, al_c, bits):
    """launch422()'s choice (csrc/ntscsim_hip.hip) in the throughput form, in terms of the parameters, the alignment of
    the luma and of the chroma rows and the bits of ntscsim_debug_no_fast_decode()"""
    no_fast, split, no_stream = bool(bits & 1), bool(bits & 2), bool(bits & 4)
    ntsc = p.tv_standard == 0
    pre_on = p.composite_preemphasis != 0 and p.composite_preemphasis_cut > 0
    out_lp = 2 if p.composite_out_chroma_lowpass else (1 if p.composite_out_chroma_lowpass_lite else 0)
    cdelay = {0: 4, 1: 5, 2: 6}[p.output_vhs_tape_speed]
    family = (not no_fast and not p.nocolor_subcarrier and p.composite_in_chroma_lowpass and
              not p.nocolor_subcarrier_after_yc_sep and p.video_yc_recombine == 0)
    vhs, sv = bool(p.emulating_vhs), bool(p.vhs_svideo_out)
    fused, direct, fused_sv = family and vhs and not sv, family and not vhs, family and vhs and sv
    al = al_y and al_c
    mode, off = p.video_scanline_phase_shift, p.video_scanline_phase_shift_offset
    even = (not off & 1) if mode == 180 else mode not in (90, 270)
    spec = (not split and ntsc and not pre_on and p.video_noise and p.video_chroma_noise and p.video_chroma_phase_noise and
            out_lp == 2 and cdelay == 4 and al)
    stream = spec and even and p.subcarrier_amplitude == 50 and p.subcarrier_amplitude_back == 50 and not no_stream
    stream_gen = fused and not stream and not no_stream and not split and al
    fasta = direct and not split and ntsc and not pre_on and p.video_noise and even and p.subcarrier_amplitude == 50 and al
    stream_sv = fused_sv and not no_stream and not split and al
    if direct:
        return "k422_direct_fast" if fasta else DIRECT
    if stream_sv:
        return "k422_fused_sv<%d>" % cdelay
    if not fused:
        return PROC
    if stream:
        return "k422_fused<true,true,4>"
    if stream_gen:
        return "k422_fused<false,true,%d>" % cdelay
    return S4 if spec else F4


def alignment(w, h, layout):
    """(luma rows 16-byte aligned, chroma rows 8-byte aligned) of a launch's frames: linesizes and plane starts"""
    ls, off = T.linesizes(w, layout), T.plane_offsets(w, h, layout)
    return ls[0] % 16 == 0, all(v % 8 == 0 for v in (ls[1], ls[2], off[1], off[2], T.frame_bytes(w, h, layout)))


def companion_bits(row):
    """the second launch of a row's context: the dispatcher's own choice for rows that a debug bit reaches (the streamed
    forms, k422_direct_fast, or the four sweeps on unaligned rows), the twelve sweeps where that is the row's own form"""
    if row.bits and launcher_rule(params(row), *alignment(row.w, row.h, row.layout), 0) != row.kernel:
        return 0
    return 1


# ------------------------------------------------------------------------------------------------ frames and the oracle
def params(row):
    import _libs as L
    return L.make_params_tocomp(row.flags)


def darken(frames, seed):
    """dark, colourless stretches (what black_key_feedback replaces) in the pictures"""
    r = np.random.RandomState(seed)
    for f in frames:
        dark = r.randint(0, 3, size=(f.h, f.w // 2)) == 0
        for s in (0, 1):
            f.pix(0)[:, s::2][dark] = r.randint(10, 40, size=int(dark.sum()), dtype=np.uint8)
        for i in (1, 2):
            f.pix(i)[dark] = r.randint(120, 136, size=int(dark.sum()), dtype=np.uint8)


Case = namedtuple("Case", "init exp frames srcbuf srcs fltinit fltexp jobs mask rng_pos calls shifts")


def _seed(row):
    return int.from_bytes(row.id.encode()[-6:], "little") % 100003 + 7 * row.w + len(row.id)


@functools.lru_cache(maxsize=2)
def case(row_id):
    """The launch of a row and what the oracle makes of it (tests/_pipe422_forms.py: case, with the filter frames of the
    black key): one buffer with all frames (guards between them), the oracle in MEMORY mode field after field, the
    descriptors as (frame index, source index or None, field, fieldno, flags)"""
    import ctypes as C
    import _libs as L
    row = BY_ID[row_id]
    p = params(row)
    w, h, n = row.w, row.h, row.n
    nfr = 1 if row.share else n
    init = np.empty(nfr * T.frame_bytes(w, h, row.layout), np.uint8)
    frames = [T.frame_at(init, k, w, h, row.layout) for k in range(nfr)]
    T.fill(init, frames, _seed(row), bars_every=5)
    srcbuf, srcs, fltinit, fltexp, eflt = None, [], None, None, []
    fl = T.SRC_FLAGS.get(row.source)
    if fl is not None:
        nsrc = (n + 1) // 2
        srcbuf = np.empty(nsrc * T.frame_bytes(w, h, "padded"), np.uint8)
        srcs = [T.frame_at(srcbuf, k, w, h, "padded") for k in range(nsrc)]
        T.fill(srcbuf, srcs, _seed(row) + 1)
    if row.source == "bkey":
        assert p.black_key_level_feedback >= 0
        darken(frames, _seed(row) + 2)
        fltinit = np.empty(nfr * T.frame_bytes(w, h, "padded"), np.uint8)
        T.fill(fltinit, [T.frame_at(fltinit, k, w, h, "padded") for k in range(nfr)], _seed(row) + 3)
        fltexp = fltinit.copy()
        eflt = [T.frame_at(fltexp, k, w, h, "padded") for k in range(nfr)]
    exp = init.copy()
    eframes = [T.frame_at(exp, k, w, h, row.layout) for k in range(nfr)]
    o = L.TocompOracleStream(p, L.OOB_MEMORY)
    lib = L.product()
    jobs, calls, shifts = [], 0, []
    for k in range(n):
        field = (k & 1) ^ 1
        fi = 0 if row.share else k
        if fl is not None:
            L.tocomp_oracle_render_field(eframes[fi], srcs[k // 2], int(bool(fl & 4)), int(bool(fl & 1)), int(bool(fl & 2)),
                                         int(bool(fl & 8)), field)
        if eflt:
            L.tocomp_oracle_black_key(eframes[fi], eflt[fi], field, p.black_key_level_feedback)
        shifts.append(T.hs_shifts(p, o.g, w, h, field))
        o.process(eframes[fi], field, k)
        calls += lib.ntscsim_rng_calls_per_field_422(C.byref(p), w, h, field)
        jobs.append((fi, k // 2 if fl is not None else None, field, k, fl or 0))
    for a in (init, exp, srcbuf, fltinit, fltexp):
        if a is not None:
            a.setflags(write=False)
    return Case(init, exp, frames, srcbuf, srcs, fltinit, fltexp, jobs, T.margin_mask(frames, init.size), o.rng_pos, calls, shifts)


MixedCase = namedtuple("MixedCase", "init exp frames sets set_of jobs mask rng_pos")


@functools.lru_cache(maxsize=2)
def mixed_case(mid):
    """One ntscsim_mixed_fields422_device() call: descriptor i names set i mod 10 and owns frame i; the oracle runs them in
    order, each with the parameters of its set, from the rand() position the one before it left"""
    import ctypes as C
    import _libs as L
    m = {x.id: x for x in MIXED}[mid]
    sets = [L.make_params_tocomp(f) for _, f in MIXED_SETS]
    n = 2 * len(sets)
    init = np.empty(n * T.frame_bytes(m.w, m.h, m.layout), np.uint8)
    frames = [T.frame_at(init, k, m.w, m.h, m.layout) for k in range(n)]
    T.fill(init, frames, 31 * m.w + m.h + len(m.layout), bars_every=7)
    exp = init.copy()
    eframes = [T.frame_at(exp, k, m.w, m.h, m.layout) for k in range(n)]
    lib = L.product()
    cursor, jobs, set_of = 0, [], []
    for i in range(n):
        s = i % len(sets)
        field = ((i // len(sets)) ^ i ^ 1) & 1
        o = L.TocompOracleStream(sets[s], L.OOB_MEMORY)
        o.skip(cursor)
        o.process(eframes[i], field, i)
        assert o.rng_pos - cursor == lib.ntscsim_rng_calls_per_field_422(C.byref(sets[s]), m.w, m.h, field)
        cursor = o.rng_pos
        jobs.append((i, None, field, i, 0))
        set_of.append(s)
    init.setflags(write=False)
    exp.setflags(write=False)
    return MixedCase(init, exp, frames, sets, set_of, jobs, T.margin_mask(frames, init.size), cursor)
